// hostsan_main.hip -- the library's host code under AddressSanitizer and UndefinedBehaviorSanitizer, without a device.
//
// A stand-alone executor: it reads the records tests/hostsancases.py wrote (plain int32 words: function id, word count, words),
// makes each call with every output buffer malloc'ed at exactly the size the library asked for (so that one byte too many lands
// in a redzone), and writes back the return code and the raw bytes of what the library wrote.  It holds no expectation of its
// own, except for the refusal records, which carry the code the entry point has to return before its first HIP call.
// It includes gcnn_capi.hip itself, so the library's static host functions are in reach; only host code is instrumented
// (-Xarch_host), the device code is compiled as always and never runs here.  Nothing is enqueued and no device is needed; the one
// place where these paths touch the HIP runtime is the size query of rocprim's radix sort (sort_temp_bytes, in every layout that
// sizes a sort), which asks the runtime for the current device: the test hides every device so that the answer is the same everywhere.
//
//   hostsan <cases.bin> <results.bin>     run the records
//   hostsan --selftest-asan               write one entry past a malloc of this file's own: ASan has to report it
//   hostsan --selftest-ubsan              add 1 to INT_MAX in this file's own code: UBSan has to report it
//   hostsan --selftest-conversion         narrow 2^40 to int implicitly: -fsanitize=implicit-conversion has to report it
#include "gcnn_capi.hip"

#include <climits>
#include <vector>

namespace hostsan {

static const unsigned char FILL = 0xA5;
static const uintptr_t FAKE = 0x7f0000001000ull;   // a pointer value that is never dereferenced: 256-byte aligned, not null

struct Reader {
    const int32_t* p; const int32_t* end;
    int32_t i() { if (p >= end) { fprintf(stderr, "hostsan: record too short\n"); exit(3); } return *p++; }
};

static FILE* g_out;
static void emit(int64_t rc, const void* bytes, size_t n) {
    const int64_t head[2] = {rc, (int64_t)n};
    fwrite(head, sizeof(head), 1, g_out);
    if (n) fwrite(bytes, 1, n, g_out);
}

template <class T> static T* fresh(size_t count = 1) {   // exactly count * sizeof(T) bytes, filled with the marker
    T* p = (T*)malloc(count * sizeof(T));
    memset((void*)p, FILL, count * sizeof(T));
    return p;
}
static void* fresh_bytes(size_t n) { void* p = malloc(n); memset(p, FILL, n); return p; }

static void read_one(Reader& r, gcnn_dims* d) { d->n_cons = r.i(); d->n_vars = r.i(); d->n_cuts = r.i(); d->n_cons_edges = r.i(); d->n_cut_edges = r.i(); }
static void read_one(Reader& r, gcnn_lp_dims* d) {
    memset(d, 0, sizeof(*d));
    d->n_rows = r.i(); d->n_cols = r.i(); d->n_cuts = r.i(); d->row_nnz = r.i(); d->cut_nnz = r.i(); d->has_incumbent = r.i();
    d->n_model_vars = r.i(); d->n_state_rows = r.i(); d->n_state_edges = r.i(); d->reserved = r.i();
    d->infinity = 1e20; d->sum_epsilon = 1e-6; d->obj_norm = 1.0;
}
static void read_one(Reader& r, gcnn_hybrid_dims* d) {
    memset(d, 0, sizeof(*d));
    d->n_cols = r.i(); d->n_cuts = r.i(); d->cut_nnz = r.i(); d->infinity = 1e20;
}
static void read_one(Reader& r, gcnn_lp_append_dims* b) {
    b->n_rows = r.i(); b->row_nnz = r.i(); b->n_state_rows = r.i(); b->n_state_edges = r.i();
    b->n_lhs_rows = r.i(); b->n_lhs_edges = r.i(); b->res_lhs_rows = r.i(); b->res_lhs_edges = r.i();
}
static void read_one(Reader& r, gcnn_lp_remove_dims* b) {
    b->n_rows = r.i(); b->row_nnz = r.i(); b->n_state_rows = r.i(); b->n_state_edges = r.i();
    b->n_lhs_rows = r.i(); b->n_lhs_edges = r.i(); b->res_lhs_rows = r.i(); b->res_lhs_edges = r.i();
}
static void read_one(Reader& r, gcnn_lp_rounds_member* m) {
    memset(m, 0, sizeof(*m));
    read_one(r, &m->dims);
    m->present = r.i(); m->n_forced = r.i(); m->n_forced_entries = r.i(); m->has_append = r.i();
    read_one(r, &m->block);
}
static void read_one(Reader& r, gcnn_lp_rounds_edit_member* m) {
    memset(m, 0, sizeof(*m));
    read_one(r, &m->dims);
    m->present = r.i(); m->n_forced = r.i(); m->n_forced_entries = r.i(); m->has_append = r.i();
    read_one(r, &m->block);
    m->has_remove = r.i();
    read_one(r, &m->removed);
}

enum { NULL_FIRST = 1, NULL_NF = 2, NULL_NFE = 4, NULL_OUT = 8, NULL_MODEL_OF = 16, NULL_SECOND = 32 };

// a single struct argument: null mask, then its words
template <class D> struct One {
    int mask; D* d;
    explicit One(Reader& r) : mask(r.i()), d(fresh<D>()) { read_one(r, d); }
    ~One() { free(d); }
    const D* ptr() const { return (mask & NULL_FIRST) ? nullptr : d; }
    template <class L> L* out(L* l) const { return (mask & NULL_OUT) ? nullptr : l; }
};

// the arguments every call on several states, snapshots or members starts with: the count as passed, the count the arrays
// really hold, the null mask, the structs, the forced rows and entries (and the model of each, where the call takes one)
template <class D> struct Many {
    int n, n_real, mask; D* d; int32_t *nf, *nfe, *model_of;
    Many(Reader& r, bool forced, bool models) : nf(nullptr), nfe(nullptr), model_of(nullptr) {
        n = r.i(); n_real = r.i(); mask = r.i();
        d = fresh<D>(n_real);
        for (int s = 0; s < n_real; ++s) read_one(r, &d[s]);
        if (forced) {
            nf = fresh<int32_t>(n_real); nfe = fresh<int32_t>(n_real);
            for (int s = 0; s < n_real; ++s) nf[s] = r.i();
            for (int s = 0; s < n_real; ++s) nfe[s] = r.i();
        }
        if (models) { model_of = fresh<int32_t>(n_real); for (int s = 0; s < n_real; ++s) model_of[s] = r.i(); }
    }
    ~Many() { free(d); free(nf); free(nfe); free(model_of); }
    const D* ptr() const { return (mask & NULL_FIRST) ? nullptr : d; }
    const int32_t* f() const { return (mask & NULL_NF) ? nullptr : nf; }
    const int32_t* fe() const { return (mask & NULL_NFE) ? nullptr : nfe; }
    const int32_t* mo() const { return (mask & NULL_MODEL_OF) ? nullptr : model_of; }
    template <class L> L* out(L* l) const { return (mask & NULL_OUT) ? nullptr : l; }
};

template <class L, class F> static void layout_case(F call) {
    L* l = fresh<L>();
    const int rc = call(l);
    emit(rc, l, sizeof(L));
    free(l);
}

// A table writer: into a buffer of exactly `bytes` (what the accepted layout states), or, when the layout was refused, of
// `refused_bytes` -- the table's constant size where it has one, else 16 bytes the writer must leave alone.
static const size_t TABLE_CAP = (size_t)64 << 20;
template <class F> static void table_case(int layout_rc, size_t bytes, size_t refused_bytes, bool null_table, F call) {
    if (null_table) { emit(call((void*)nullptr), nullptr, 0); return; }
    const size_t n = layout_rc == 0 ? bytes : refused_bytes;
    if (n > TABLE_CAP) { emit(INT32_MIN, nullptr, 0); return; }   // too large to allocate: skipped, and said so
    void* t = fresh_bytes(n);
    const int rc = call(t);
    emit(rc, t, n);
    free(t);
}

static void pack_case(Reader& r) {
    const int which = r.i(), n_edges = r.i(), n_left = r.i(), n_real = r.i(), mask = r.i();
    int scratch_entries = r.i();
    if (scratch_entries < 0) scratch_entries = n_left + 1;
    int32_t *rows = fresh<int32_t>(n_real), *cols = fresh<int32_t>(n_real); float* vals = fresh<float>(n_real);
    for (int e = 0; e < n_real; ++e) rows[e] = r.i();
    for (int e = 0; e < n_real; ++e) cols[e] = r.i();
    for (int e = 0; e < n_real; ++e) vals[e] = 1.0f + 0.25f * (float)e;
    // out_inds [2, n_real] and out_vals [n_real] side by side in the result, each its own exact allocation
    int32_t* oi = fresh<int32_t>(2 * (size_t)n_real); float* ov = fresh<float>(n_real); int32_t* sc = fresh<int32_t>(scratch_entries);
    auto pick = [&](int bit, auto* p) { return (mask & (1 << bit)) ? nullptr : p; };
    const int rc = (which ? gcnn_host_sort_edges_by_row : gcnn_host_pack_edges)(pick(0, rows), pick(1, cols), pick(2, vals), n_edges, n_left,
                                                                                 pick(3, oi), pick(4, ov), pick(5, sc));
    std::vector<char> both(12 * (size_t)n_real);
    if (n_real) { memcpy(both.data(), oi, 8 * (size_t)n_real); memcpy(both.data() + 8 * (size_t)n_real, ov, 4 * (size_t)n_real); }
    emit(rc, both.data(), both.size());
    free(rows); free(cols); free(vals); free(oi); free(ov); free(sc);
}

#include "hostsan_refusals.inc"

static void run_case(int fid, Reader& r) {
    switch (fid) {
    // ---- size functions
    case 0: { One<gcnn_dims> a(r); const size_t v = gcnn_workspace_floats(a.ptr()); emit(0, &v, sizeof(v)); break; }
    case 1: { const size_t v = gcnn_graph_temp_bytes(r.i()); emit(0, &v, sizeof(v)); break; }
    case 2: { const int a = r.i(), b = r.i(), c = r.i(); const size_t v = gcnn_select_workspace_bytes(a, b, c); emit(0, &v, sizeof(v)); break; }
    case 3: {
        const int n = r.i(), mask = r.i();
        size_t* v = fresh<size_t>();
        emit(gcnn_group_table_bytes(n, (mask & NULL_OUT) ? nullptr : v), v, sizeof(*v));
        free(v);
        break;
    }
    case 4: {
        const int index = r.i(), mask = r.i();
        int* v = fresh<int>(4);
        auto pick = [&](int k) { return (mask & (1 << k)) ? nullptr : v + k; };
        emit(gcnn_param_info(index, pick(0), pick(1), pick(2), pick(3)), v, 4 * sizeof(int));
        free(v);
        break;
    }
    case 5: { const int v = r.i() ? gcnn_param_total_floats() : gcnn_param_count(); emit(0, &v, sizeof(v)); break; }
    case 6: { One<gcnn_dims> a(r); const int v = edges_without_nodes(*a.d); emit(0, &v, sizeof(v)); break; }   // static, host only
    // ---- layouts of one state or snapshot
    case 10: { One<gcnn_dims> a(r); layout_case<gcnn_infer_layout>([&](auto* l) { return gcnn_infer_layout_for(a.ptr(), a.out(l)); }); break; }
    case 11: {
        One<gcnn_dims> a(r); const int nf = r.i(), nfe = r.i();
        layout_case<gcnn_select_layout>([&](auto* l) { return gcnn_infer_select_layout_for(a.ptr(), nf, nfe, a.out(l)); });
        break;
    }
    case 14: {
        One<gcnn_dims> a(r); const int nf = r.i(), nfe = r.i(), mode = r.i(), nm = r.i();
        layout_case<gcnn_ensemble_layout>([&](auto* l) { return gcnn_infer_ensemble_layout_for(a.ptr(), nf, nfe, mode, nm, a.out(l)); });
        break;
    }
    case 16: {
        One<gcnn_lp_dims> a(r); const int nf = r.i(), nfe = r.i();
        layout_case<gcnn_lp_layout>([&](auto* l) { return gcnn_lp_layout_for(a.ptr(), nf, nfe, a.out(l)); });
        break;
    }
    case 19: {
        One<gcnn_lp_dims> a(r); const int nf = r.i(), nfe = r.i();
        layout_case<gcnn_lp_collect_layout>([&](auto* l) { return gcnn_lp_collect_layout_for(a.ptr(), nf, nfe, a.out(l)); });
        break;
    }
    case 20: { One<gcnn_lp_dims> a(r); layout_case<gcnn_lp_rows_layout>([&](auto* l) { return gcnn_lp_rows_layout_for(a.ptr(), a.out(l)); }); break; }
    case 21: {
        One<gcnn_lp_dims> a(r); const int present = r.i(), nf = r.i(), nfe = r.i();
        layout_case<gcnn_lp_round_layout>([&](auto* l) { return gcnn_lp_round_layout_for(a.ptr(), present, nf, nfe, a.out(l)); });
        break;
    }
    case 22: {
        One<gcnn_lp_dims> a(r); One<gcnn_lp_append_dims> b(r); const int present = r.i(), nf = r.i(), nfe = r.i();
        layout_case<gcnn_lp_append_layout>([&](auto* l) { return gcnn_lp_append_layout_for(a.ptr(), b.ptr(), present, nf, nfe, a.out(l)); });
        break;
    }
    case 23: {
        One<gcnn_lp_dims> a(r); One<gcnn_lp_remove_dims> m(r); One<gcnn_lp_append_dims> b(r); const int present = r.i(), nf = r.i(), nfe = r.i();
        layout_case<gcnn_lp_remove_layout>([&](auto* l) { return gcnn_lp_remove_layout_for(a.ptr(), m.ptr(), b.ptr(), present, nf, nfe, a.out(l)); });
        break;
    }
    case 26: {
        One<gcnn_lp_dims> a(r); const int nf = r.i(), nfe = r.i(), mode = r.i(), nm = r.i();
        layout_case<gcnn_lp_ensemble_layout>([&](auto* l) { return gcnn_lp_ensemble_layout_for(a.ptr(), nf, nfe, mode, nm, a.out(l)); });
        break;
    }
    case 28: {
        One<gcnn_lp_rounds_edit_member> a(r); const int mode = r.i(), nm = r.i();
        layout_case<gcnn_lp_round_ensemble_layout>([&](auto* l) { return gcnn_lp_round_ensemble_layout_for(a.ptr(), mode, nm, a.out(l)); });
        break;
    }
    // ---- layouts of several
    case 12: {
        Many<gcnn_dims> a(r, true, false); const int mode = r.i();
        layout_case<gcnn_ibatch_layout>([&](auto* l) { return gcnn_infer_batch_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, a.out(l)); });
        break;
    }
    case 13: {
        Many<gcnn_dims> a(r, true, true); const int mode = r.i(), nm = r.i();
        layout_case<gcnn_mbatch_layout>([&](auto* l) { return gcnn_infer_models_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, nm, a.mo(), a.out(l)); });
        break;
    }
    case 15: {
        Many<gcnn_dims> a(r, true, false); const int mode = r.i(), nm = r.i();
        layout_case<gcnn_ensemble_layout>([&](auto* l) { return gcnn_infer_ensemble_batch_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, nm, a.out(l)); });
        break;
    }
    case 17: {
        Many<gcnn_lp_dims> a(r, true, false); const int mode = r.i();
        layout_case<gcnn_lp_batch_layout>([&](auto* l) { return gcnn_lp_batch_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, a.out(l)); });
        break;
    }
    case 18: {
        Many<gcnn_lp_dims> a(r, true, true); const int mode = r.i(), nm = r.i();
        layout_case<gcnn_lp_models_layout>([&](auto* l) { return gcnn_lp_models_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, nm, a.mo(), a.out(l)); });
        break;
    }
    case 24: {
        Many<gcnn_lp_rounds_member> a(r, false, false); const int mode = r.i();
        layout_case<gcnn_lp_rounds_layout>([&](auto* l) { return gcnn_lp_rounds_layout_for(a.n, a.ptr(), mode, a.out(l)); });
        break;
    }
    case 25: {
        Many<gcnn_lp_rounds_edit_member> a(r, false, false); const int mode = r.i();
        layout_case<gcnn_lp_rounds_edit_layout>([&](auto* l) { return gcnn_lp_rounds_edit_layout_for(a.n, a.ptr(), mode, a.out(l)); });
        break;
    }
    case 27: {
        Many<gcnn_lp_dims> a(r, true, false); const int mode = r.i(), nm = r.i();
        layout_case<gcnn_lp_ensemble_layout>([&](auto* l) { return gcnn_lp_ensemble_batch_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, nm, a.out(l)); });
        break;
    }
    case 29: {
        Many<gcnn_hybrid_dims> a(r, true, false); const int mode = r.i();
        layout_case<gcnn_hybrid_layout>([&](auto* l) { return gcnn_hybrid_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, a.out(l)); });
        break;
    }
    // ---- table writers: the words of the layout's record, then 1 for a null table
    case 30: {
        Many<gcnn_dims> a(r, true, false); const int mode = r.i(), null_table = r.i();
        (void)mode;
        const size_t bytes = 4 * (size_t)GCNN_IBATCH_TABLE_COLS * GCNN_IBATCH_TABLE_STRIDE;
        table_case(0, bytes, bytes, null_table, [&](void* t) { return gcnn_infer_batch_fill_table(a.n, a.ptr(), a.f(), a.fe(), (int32_t*)t); });
        break;
    }
    case 31: {
        Many<gcnn_dims> a(r, true, true); const int mode = r.i(), nm = r.i(), null_table = r.i();
        (void)mode;
        const size_t bytes = 4 * (size_t)GCNN_MBATCH_TABLE_WORDS;
        table_case(0, bytes, bytes, null_table, [&](void* t) { return gcnn_infer_models_fill_table(a.n, a.ptr(), a.f(), a.fe(), nm, a.mo(), (int32_t*)t); });
        break;
    }
    case 32: {
        Many<gcnn_lp_dims> a(r, true, false); const int mode = r.i(), null_table = r.i();
        gcnn_lp_batch_layout* l = fresh<gcnn_lp_batch_layout>();
        const int lrc = gcnn_lp_batch_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, l);
        table_case(lrc, l->table_bytes, 16, null_table, [&](void* t) { return gcnn_lp_batch_fill_table(a.n, a.ptr(), a.f(), a.fe(), mode, t); });
        free(l);
        break;
    }
    case 33: {
        Many<gcnn_lp_dims> a(r, true, true); const int mode = r.i(), nm = r.i(), null_table = r.i();
        gcnn_lp_models_layout* l = fresh<gcnn_lp_models_layout>();
        const int lrc = gcnn_lp_models_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, nm, a.mo(), l);
        table_case(lrc, l->lp.table_bytes, 16, null_table, [&](void* t) { return gcnn_lp_models_fill_table(a.n, a.ptr(), a.f(), a.fe(), mode, nm, a.mo(), t); });
        free(l);
        break;
    }
    case 34: {
        Many<gcnn_hybrid_dims> a(r, true, false); const int mode = r.i(), null_table = r.i();
        gcnn_hybrid_layout* l = fresh<gcnn_hybrid_layout>();
        const int lrc = gcnn_hybrid_layout_for(a.n, a.ptr(), a.f(), a.fe(), mode, l);
        table_case(lrc, l->table_bytes, 16, null_table, [&](void* t) { return gcnn_hybrid_fill_table(a.n, a.ptr(), a.f(), a.fe(), mode, t); });
        free(l);
        break;
    }
    // ---- host packers
    case 40: pack_case(r); break;
    // ---- entry points that launch: refused argument sets only
    case 50: refusal_case(r); break;
    default: fprintf(stderr, "hostsan: unknown function id %d\n", fid); exit(3);
    }
}

static int run(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    if (!f) { perror(in_path); return 3; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<int32_t> words((size_t)bytes / 4);
    if (fread(words.data(), 4, words.size(), f) != words.size()) { perror("read"); return 3; }
    fclose(f);
    g_out = fopen(out_path, "wb");
    if (!g_out) { perror(out_path); return 3; }
    size_t at = 0, n_cases = 0;
    while (at < words.size()) {
        const int fid = words[at], n = words[at + 1];
        Reader r{words.data() + at + 2, words.data() + at + 2 + n};
        run_case(fid, r);
        if (r.p != r.end) { fprintf(stderr, "hostsan: record %zu (function %d) has %d words left over\n", n_cases, fid, (int)(r.end - r.p)); return 3; }
        at += 2 + (size_t)n; ++n_cases;
    }
    fclose(g_out);
    fprintf(stderr, "hostsan: %zu records\n", n_cases);
    return 0;
}

// the two errors the sanitizers must report, committed in this file's own code: a build that lost its instrumentation passes neither
static int selftest_asan() {
    volatile int* p = (volatile int*)malloc(4 * sizeof(int));
    volatile int at = 4;
    p[at] = 1;   // one entry past the allocation
    free((void*)p);
    return 0;
}
static int selftest_ubsan() {
    volatile int big = INT_MAX;
    int sum = big + 1;   // signed overflow
    volatile int sink = sum; (void)sink;
    return 0;
}

static int selftest_conversion() {
    volatile long long big = 1LL << 40;
    int narrow = big;   // implicit 64-to-32-bit narrowing that changes the value
    volatile int sink = narrow; (void)sink;
    return 0;
}

}   // namespace hostsan

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--selftest-asan")) return hostsan::selftest_asan();
    if (argc == 2 && !strcmp(argv[1], "--selftest-ubsan")) return hostsan::selftest_ubsan();
    if (argc == 2 && !strcmp(argv[1], "--selftest-conversion")) return hostsan::selftest_conversion();
    if (argc != 3) { fprintf(stderr, "usage: hostsan <cases.bin> <results.bin> | --selftest-asan | --selftest-ubsan | --selftest-conversion\n"); return 2; }
    return hostsan::run(argv[1], argv[2]);
}
