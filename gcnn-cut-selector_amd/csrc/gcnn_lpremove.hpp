// gcnn_lpremove.hpp -- host side of the removal of rows from a resident LP (k_lpremove.hpp): its layout, check and launches
// (lpd_layout, lpd_check, lpd_enqueue), the byte spans of every overlap rule (LpSpans) and gcnn_lp_rows_remove, the removal alone.
// As the first file that sees both edits it also holds the round with edits -- LpEdit, lpe_plan, lpe_check, lpe_enqueue_edits -- and
// its two solo calls, gcnn_lp_round_append and gcnn_lp_round_remove; gcnn_lpedits.hpp runs several of them in one call.  Included at
// the end of gcnn_capi.hip behind gcnn_lpappend.hpp (it shares lpa_layout / lpa_check / lpa_enqueue and gcnn_lpres.hpp's lpr_check /
// lpr_run), kept apart so that its launch names form their own inventory (tests/test_lpremove_build.py).
#include "k_lpremove.hpp"

// scratch carving: part_a | part_b | vcnt + vpart (one cleared block) | row_map | row_new
struct LpdScratch { size_t part_a, part_b, vcnt, vpart, clear_bytes, row_map, row_new, bytes; };
static LpdScratch lpd_scratch(const gcnn_lp_dims* d) {
    LpdScratch s; Carver c{0};
    const size_t nrc = lp_chunks(d->n_rows), nvc = lp_chunks(d->n_cols);
    s.part_a = c.take(16 * (nrc + 1), 16);
    s.part_b = c.take(16 * (nrc + 1), 16);
    s.vcnt = c.take(4 * (size_t)d->n_cols, 16);
    s.vpart = c.take(4 * (nvc + 1), 16);
    s.clear_bytes = c.off - s.vcnt;
    s.row_map = c.take(4 * (size_t)d->n_state_rows, 16);
    s.row_new = c.take(4 * (size_t)d->n_rows, 16);
    s.bytes = c.off;
    return s;
}

// the resident dims and the removal's counts -> the dims after the removal; false where either is malformed, where a count exceeds
// what is resident, or where the whole edit (b: the block appended behind it, or null) leaves no row at all
static bool lpd_dims_after(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, gcnn_lp_dims* mid) {
    if (!lp_dims_ok(d) || !m) return false;
    if (m->n_rows < 1 || m->row_nnz < 0 || m->n_state_rows < 0 || m->n_state_edges < 0 || m->n_lhs_rows < 0 || m->n_lhs_edges < 0) return false;
    if (m->n_rows > d->n_rows || m->row_nnz > d->row_nnz || m->n_state_rows > d->n_state_rows || m->n_state_edges > d->n_state_edges)
        return false;
    if (m->n_lhs_rows > m->n_rows || m->n_state_rows - m->n_lhs_rows > m->n_rows || m->n_lhs_rows > m->n_state_rows) return false;
    if (m->n_lhs_edges > m->row_nnz || m->n_lhs_edges > m->n_state_edges || (int64_t)m->n_state_edges - m->n_lhs_edges > m->row_nnz) return false;
    if (m->res_lhs_rows < 0 || m->res_lhs_rows > d->n_state_rows || m->res_lhs_edges < 0 || m->res_lhs_edges > d->n_state_edges) return false;
    if (m->n_lhs_rows > m->res_lhs_rows || m->n_lhs_edges > m->res_lhs_edges) return false;
    if (m->n_state_rows - m->n_lhs_rows > d->n_state_rows - m->res_lhs_rows ||
        m->n_state_edges - m->n_lhs_edges > d->n_state_edges - m->res_lhs_edges)
        return false;
    *mid = *d;
    mid->n_rows -= m->n_rows; mid->row_nnz -= m->row_nnz; mid->n_state_rows -= m->n_state_rows; mid->n_state_edges -= m->n_state_edges;
    if (!lp_dims_ok(mid)) return false;
    if (b && (b->res_lhs_rows != m->res_lhs_rows - m->n_lhs_rows || b->res_lhs_edges != m->res_lhs_edges - m->n_lhs_edges)) return false;
    return (int64_t)mid->n_rows + (b ? b->n_rows : 0) >= 1;
}

static int lpd_layout(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, int32_t present, int32_t n_forced,
                      int32_t n_forced_entries, gcnn_lp_remove_layout* L) {
    gcnn_lp_dims mid;
    if (!L || !lpd_dims_after(d, m, b, &mid)) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    L->list_bytes = (4 * (size_t)m->n_rows + 255) & ~(size_t)255;
    size_t inner_in, inner_arena;
    int rc;
    if (b) {                                                    // the fused append's call behind the list, its flags in front of ours
        gcnn_lp_append_layout AL;
        rc = lpa_layout(&mid, b, present, n_forced, n_forced_entries, &AL, 16);
        if (rc == GCNN_E_BADARG) return rc;
        L->block_bytes = AL.block_bytes;
        for (int i = 0; i < 5; ++i) L->block_off[i] = L->list_bytes + AL.block_off[i];
        L->round = AL.round;
        inner_in = AL.in_bytes; inner_arena = AL.arena_bytes;
        L->out_bytes = AL.out_bytes; L->append_flags_off = AL.flags_off;
        L->round_off = L->list_bytes + AL.round_off; L->append_scratch_off = L->list_bytes + AL.scratch_off;
    } else {
        rc = lpr_round_layout(&mid, present, n_forced, n_forced_entries, &L->round, 16);
        if (rc == GCNN_E_BADARG) return rc;
        inner_in = L->round.in_bytes; inner_arena = L->round.arena_bytes;
        L->out_bytes = L->round.out_bytes;
        L->round_off = L->list_bytes;
    }
    L->in_bytes = L->list_bytes + inner_in;
    L->flags_off = L->out_bytes - 16;                           // the removal's four flag words close the download
    L->scratch_bytes = lpd_scratch(d).bytes;
    L->scratch_off = L->list_bytes + ((inner_arena + 255) & ~(size_t)255);
    L->arena_bytes = L->scratch_off + L->scratch_bytes;
    return rc;
}
extern "C" int gcnn_lp_remove_layout_for(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, int32_t present,
                                         int32_t n_forced, int32_t n_forced_entries, gcnn_lp_remove_layout* L) {
    return layout_out(L, [&](gcnn_lp_remove_layout* l) { return lpd_layout(d, m, b, present, n_forced, n_forced_entries, l); });
}

// Byte spans of device memory -- of a set of derived arrays or of the raw rows for given sizes, or single buffers -- and whether any
// span of one list meets one of another.  The one vocabulary of every overlap rule on resident LPs: a removal's sources against its
// destinations (lpd_check), the three sets of a removal with an append (lpe_check), one member of a call of several against another
// (lpes_spans, gcnn_lpedits.hpp).  A null pointer or an empty array is no span.
struct LpSpans {
    struct Span { uintptr_t lo, hi; };
    std::vector<Span> v;
    LpSpans& add(const void* p, size_t bytes) {
        if (p && bytes) v.push_back(Span{(uintptr_t)p, (uintptr_t)p + bytes});
        return *this;
    }
    LpSpans& set(const gcnn_lp_rows_set* s, const gcnn_lp_dims* d) {
        const size_t R = d->n_rows, C = d->n_state_rows, E = d->n_state_edges, V = d->n_cols;
        return add(s->cons_feats, 16 * C).add(s->edge_row, 4 * E).add(s->edge_col, 4 * E).add(s->edge_coef, 4 * E).add(s->l_ptr, 4 * (C + 1))
            .add(s->v_ptr, 4 * (V + 1)).add(s->v_oth, 4 * E).add(s->v_coef, 4 * E).add(s->row_place, 8 * R).add(s->row_scale, 8 * R);
    }
    LpSpans& raw(const void* const raw[5], const gcnn_lp_dims* d) {
        const size_t R = d->n_rows, N = d->row_nnz;
        return add(raw[0], 4 * (R + 1)).add(raw[1], 4 * N).add(raw[2], 8 * N).add(raw[3], 8 * R).add(raw[4], 8 * R);
    }
    bool meets(const LpSpans& o) const {
        for (const Span& x : v)
            for (const Span& y : o.v)
                if (x.lo < y.hi && y.lo < x.hi) return true;
        return false;
    }
};
static bool lpd_raw_ok(const void* const raw[5], const gcnn_lp_dims* d) {
    return raw[0] && (d->n_rows == 0 || (raw[3] && raw[4])) && (d->row_nnz == 0 || (raw[1] && raw[2]));
}

// Everything a removal decides before anything is enqueued.  dst_dims: the sizes the destinations must hold (the dims after the
// removal, or after the append behind it for the raw rows, which the append then extends in place).
static int lpd_check(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, gcnn_lp_dims* mid,
                     const void* const raw_src[5], const void* const raw_dst[5], const gcnn_lp_dims* raw_dst_dims,
                     const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst) {
    if (!lpd_dims_after(d, m, b, mid)) return GCNN_E_BADARG;
    if (!lpd_raw_ok(raw_src, d) || !lpd_raw_ok(raw_dst, raw_dst_dims ? raw_dst_dims : mid)) return GCNN_E_BADARG;
    if (!lpa_set_ok(src, d->n_rows, d->n_state_rows, d->n_state_edges)) return GCNN_E_BADARG;
    if (!lpa_set_ok(dst, mid->n_rows, mid->n_state_rows, mid->n_state_edges)) return GCNN_E_BADARG;
    if (d->n_state_edges > 0 && (d->n_cols == 0 || d->n_state_rows == 0)) return GCNN_E_BADARG;
    if (LpSpans().set(src, d).meets(LpSpans().set(dst, mid))) return GCNN_E_BADARG;
    if (LpSpans().raw(raw_src, d).meets(LpSpans().raw(raw_dst, raw_dst_dims ? raw_dst_dims : mid))) return GCNN_E_BADARG;
    if (d->n_state_rows > (1 << 24) || d->n_cols > (1 << 24)) return GCNN_E_UNSUPPORTED;
    return 0;
}

// Everything the removal enqueues: one fill, three launches.  counts: null, or where the caller keeps the cleared removed counters
// (vcnt + vpart, LpdScratch::clear_bytes) and has enqueued their fill itself (gcnn_lpedits.hpp: one fill for all sessions).
static int lpd_enqueue(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_dims* mid, const int32_t* list,
                       const void* const raw_src[5], void* const raw_dst[5], const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst,
                       char* scratch, int32_t* flags_dev, hipStream_t st, char* counts = nullptr) {
    const LpdScratch s = lpd_scratch(d);
    LpdArgs x; memset(&x, 0, sizeof(x));
    x.src = lpa_set(src); x.dst = lpa_set(dst);
    x.list = list; x.n_list = m->n_rows;
    x.raw_ptr = (const int*)raw_src[0]; x.raw_col = (const int*)raw_src[1]; x.raw_val = (const double*)raw_src[2];
    x.raw_lhs = (const double*)raw_src[3]; x.raw_rhs = (const double*)raw_src[4];
    x.out_ptr = (int*)raw_dst[0]; x.out_col = (int*)raw_dst[1]; x.out_val = (double*)raw_dst[2];
    x.out_lhs = (double*)raw_dst[3]; x.out_rhs = (double*)raw_dst[4];
    x.R0 = d->n_rows; x.N0 = d->row_nnz; x.C0 = d->n_state_rows; x.E0 = d->n_state_edges;
    x.R1 = mid->n_rows; x.N1 = mid->row_nnz; x.C1 = mid->n_state_rows; x.E1 = mid->n_state_edges;
    x.L1 = m->res_lhs_rows - m->n_lhs_rows; x.EL1 = m->res_lhs_edges - m->n_lhs_edges;
    x.V = d->n_cols; x.nvc = lp_chunks(x.V); x.nrc = lp_chunks(x.R0);
    x.part_a = (int*)(scratch + s.part_a); x.part_b = (int*)(scratch + s.part_b);
    char* cnt = counts ? counts : scratch + s.vcnt;
    x.vcnt = (int*)cnt; x.vpart = (int*)(cnt + (s.vpart - s.vcnt)); x.row_map = (int*)(scratch + s.row_map);
    x.row_new = (int*)(scratch + s.row_new);
    x.nb_var = (x.V + LP_NT / LP_SUB - 1) / (LP_NT / LP_SUB); x.nb_edges = lp_chunks(x.E0); x.nb_raw = lp_chunks(x.N0);
    x.flags_out = flags_dev;
    if (!counts) HIPCHK(hipMemsetAsync(cnt, 0, s.clear_bytes, st));      // the removed counters (no launch of the library's own)
    {
        ProfScope prof("k_lpd_mark", st);
        GCNN_LAUNCH(k_lpd_mark, dim3(x.nrc), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_lpd_rows", st);
        GCNN_LAUNCH(k_lpd_rows, dim3(x.nrc + 1 + lp_chunks(x.V + 1)), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    if (x.nb_var + x.nb_edges + x.nb_raw > 0) {
        ProfScope prof("k_lpd_vars", st);
        GCNN_LAUNCH(k_lpd_vars, dim3(x.nb_var + x.nb_edges + x.nb_raw), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    return 0;
}

extern "C" int gcnn_lp_rows_remove(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const int32_t* list, const int32_t* row_ptr,
                                   const int32_t* row_col, const double* row_val, const double* row_lhs, const double* row_rhs,
                                   int32_t* out_ptr, int32_t* out_col, double* out_val, double* out_lhs, double* out_rhs,
                                   const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst, void* scratch, size_t scratch_bytes,
                                   int32_t* flags, void* stream) {
    gcnn_lp_dims mid;
    const void* const raw_src[5] = {row_ptr, row_col, row_val, row_lhs, row_rhs};
    void* const raw_dst[5] = {out_ptr, out_col, out_val, out_lhs, out_rhs};
    const int rc = lpd_check(d, m, nullptr, &mid, raw_src, raw_dst, nullptr, src, dst);
    if (rc) return rc;
    if (!list || !scratch || ((uintptr_t)scratch & 15) || !flags) return GCNN_E_BADARG;
    if (scratch_bytes < lpd_scratch(d).bytes) return GCNN_E_WORKSPACE;
    return lpd_enqueue(d, m, &mid, list, raw_src, raw_dst, src, dst, (char*)scratch, flags, (hipStream_t)stream);
}

// ---- a round with edits ----------------------------------------------------------------------------------------------------------
// Every round of a resident LP has one shape: an optional removal of resident rows, an optional append of a block, the round.  LpEdit
// describes one, whichever call brought it (the solo calls' argument lists below, a member of gcnn_lp_rounds or gcnn_lp_rounds_edit:
// gcnn_lpedits.hpp); lpe_plan lays it out, lpe_check is the ONE statement of what is decided before anything is enqueued, and
// lpe_enqueue_edits the ONE sequence "removal, then append" in front of lpr_run.
struct LpEdit {
    const gcnn_lp_dims* dims;                         // the resident LP BEFORE any edit
    const gcnn_lp_remove_dims* rem;                   // null: no removal
    const gcnn_lp_append_dims* app;                   // null: no append (behind a removal: its res_lhs_* are those after it)
    int32_t present, n_forced, n_forced_entries;
    const void* raw_in[5];                            // rem: the raw rows the removal reads
    void* raw[5];                                     // an edit: the raw rows it leaves -- the removal writes them, the append extends them
    const gcnn_lp_rows_set *src, *transit, *dst;      // an edit: src -> dst; both edits: the removal src -> transit, the append transit -> dst
    const gcnn_lp_resident* resident;                 // what the round runs on (with an edit: on dst)
    const float* params;
};

// The layout of one LpEdit: the dims between and after its edits, and where the solo layout of its kind (lpd_layout, lpa_layout or
// lpr_round_layout) keeps its pieces, relative to the edit's own upload, download block and arena.
struct LpePlan {
    bool degenerate;               // the state after the edits has no constraint rows, columns or cuts (a call of several: gcnn_lpedits.hpp)
    gcnn_lp_dims mid, after;       // after the removal (the dims as given without one), after the append behind it
    gcnn_lp_round_layout RL;       // relative to the round's upload, the download block and the round's arena
    size_t in_bytes, out_bytes, arena_bytes, extra_out;
    size_t block_off[5];           // the block's arrays in the upload
    size_t round_rel;              // the round's upload in the upload, and its arena in the arena: the solo arena opens with the upload
    size_t app_scratch_rel, rem_scratch_rel;
    size_t flags_off, append_flags_off;
    size_t app_counts_bytes, rem_counts_bytes;
};

static int lpe_plan(const LpEdit& e, LpePlan* P) {
    memset(P, 0, sizeof(*P));
    int rc;
    if (e.rem) {
        gcnn_lp_remove_layout D;
        if ((rc = lpd_layout(e.dims, e.rem, e.app, e.present, e.n_forced, e.n_forced_entries, &D))) return rc;
        if (!lpd_dims_after(e.dims, e.rem, e.app, &P->mid)) return GCNN_E_BADARG;
        P->after = P->mid;
        if (e.app && !lpa_dims_after(&P->mid, e.app, &P->after)) return GCNN_E_BADARG;
        P->RL = D.round;
        P->in_bytes = D.in_bytes; P->out_bytes = D.out_bytes; P->arena_bytes = D.arena_bytes; P->extra_out = e.app ? 32 : 16;
        for (int i = 0; i < 5; ++i) P->block_off[i] = D.block_off[i];
        P->round_rel = D.round_off; P->app_scratch_rel = D.append_scratch_off; P->rem_scratch_rel = D.scratch_off;
        P->flags_off = D.flags_off; P->append_flags_off = D.append_flags_off;
        P->rem_counts_bytes = al16(lpd_scratch(e.dims).clear_bytes);
        if (e.app) P->app_counts_bytes = al16(lpa_scratch(&P->mid, e.app).clear_bytes);
    } else if (e.app) {
        gcnn_lp_append_layout Q;
        if ((rc = lpa_layout(e.dims, e.app, e.present, e.n_forced, e.n_forced_entries, &Q))) return rc;
        P->mid = *e.dims;
        if (!lpa_dims_after(e.dims, e.app, &P->after)) return GCNN_E_BADARG;
        P->RL = Q.round;
        P->in_bytes = Q.in_bytes; P->out_bytes = Q.out_bytes; P->arena_bytes = Q.arena_bytes; P->extra_out = 16;
        for (int i = 0; i < 5; ++i) P->block_off[i] = Q.block_off[i];
        P->round_rel = Q.round_off; P->app_scratch_rel = Q.scratch_off;
        P->append_flags_off = Q.flags_off;
        P->app_counts_bytes = al16(lpa_scratch(e.dims, e.app).clear_bytes);
    } else {
        if ((rc = lpr_round_layout(e.dims, e.present, e.n_forced, e.n_forced_entries, &P->RL))) return rc;
        P->mid = P->after = *e.dims;
        P->in_bytes = P->RL.in_bytes; P->out_bytes = P->RL.out_bytes; P->arena_bytes = P->RL.arena_bytes;
    }
    P->degenerate = group_degenerate(lp_state_dims(&P->after));
    return 0;
}

// Everything a round with edits decides before anything is enqueued, in the solo calls' order: the removal, the append, the rule
// that the three sets of a removal with an append are three, the edit's arena (short or misaligned: GCNN_E_BADARG), the round.
static int lpe_check(const LpEdit& e, const LpePlan& P, const void* host_in, void* host_out, void* arena, size_t arena_bytes, int want,
                     double p_max, double p_max_ub) {
    int rc;
    gcnn_lp_dims mid, after;
    const double* col_obj = e.resident ? e.resident->col_obj : nullptr;
    if (e.rem) {
        if ((rc = lpd_check(e.dims, e.rem, e.app, &mid, e.raw_in, e.raw, e.app ? &P.after : nullptr, e.src, e.app ? e.transit : e.dst)))
            return rc;
        if (e.app) {
            if ((rc = lpa_check(&mid, e.app, &after, e.raw[0], e.raw[1], e.raw[2], e.raw[3], e.raw[4], col_obj, e.transit, e.dst))) return rc;
            const LpSpans last = LpSpans().set(e.dst, &after);
            if (LpSpans().set(e.src, e.dims).meets(last) || LpSpans().set(e.transit, &mid).meets(last)) return GCNN_E_BADARG;
        }
    } else if (e.app) {
        if ((rc = lpa_check(e.dims, e.app, &after, e.raw[0], e.raw[1], e.raw[2], e.raw[3], e.raw[4], col_obj, e.src, e.dst))) return rc;
    }
    if (!arena || ((uintptr_t)arena & 255) || arena_bytes < P.arena_bytes) return GCNN_E_BADARG;
    gcnn_lp_round_layout RL;
    return lpr_check(&P.after, e.present, e.n_forced, e.n_forced_entries, e.resident, e.params, host_in, host_out, (char*)arena + P.round_rel,
                     P.RL.arena_bytes, want, p_max, p_max_ub, P.extra_out, &RL);
}

// Where the edits of one LpEdit find their pieces: the edit's upload and download block, the two scratch blocks, and -- in a call of
// several (gcnn_lpedits.hpp), null otherwise -- the cleared counters the caller fills itself and the recorders that take the launches.
struct LpeAt { const char* up; char* out; char* rem_scratch; char* app_scratch; char* rem_counts; char* app_counts; GroupRecorder *rem_rec, *app_rec; };
static int lpe_enqueue_edits(const LpEdit& e, const LpePlan& P, const LpeAt& at, hipStream_t st) {
    int rc;
    if (e.rem) {
        GroupRecScope scope(at.rem_rec);
        if ((rc = lpd_enqueue(e.dims, e.rem, &P.mid, (const int32_t*)at.up, e.raw_in, e.raw, e.src, e.app ? e.transit : e.dst, at.rem_scratch,
                              (int32_t*)(at.out + P.flags_off), st, at.rem_counts)))
            return rc;
    }
    if (e.app) {
        const size_t* bo = P.block_off;
        int32_t* const raw[2] = {(int32_t*)e.raw[0], (int32_t*)e.raw[1]};
        double* const rawd[3] = {(double*)e.raw[2], (double*)e.raw[3], (double*)e.raw[4]};
        GroupRecScope scope(at.app_rec);
        if ((rc = lpa_enqueue(&P.mid, e.app, (const int*)(at.up + bo[0]), (const int*)(at.up + bo[1]), (const double*)(at.up + bo[2]),
                              (const double*)(at.up + bo[3]), (const double*)(at.up + bo[4]), e.app->row_nnz, 0, raw, rawd, e.resident->col_obj,
                              e.rem ? e.transit : e.src, e.dst, at.app_scratch, (int32_t*)(at.out + P.append_flags_off), st, at.app_counts)))
            return rc;
    }
    return 0;
}

// The solo call of a round with edits: ONE upload (the list | the block | the round | forced rows), the edits, the round, ONE download
// with the flags of every edit in it.
static int lpe_call(const LpEdit& e, const void* host_in, void* host_out, void* arena, size_t arena_bytes, int32_t want_order, double p_max,
                    double p_max_ub, void* stream) {
    LpePlan P;
    int rc = lpe_plan(e, &P);
    if (rc) return rc;
    const int want = e.n_forced >= 0 ? 1 : want_order;
    if ((rc = lpe_check(e, P, host_in, host_out, arena, arena_bytes, want, p_max, p_max_ub))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    char* round = A + P.round_rel;
    HIPCHK(hipMemcpyAsync(A, host_in, P.in_bytes, hipMemcpyHostToDevice, st));
    const LpeAt at = {A, round + P.RL.dev_off[6], A + P.rem_scratch_rel, A + P.app_scratch_rel, nullptr, nullptr, nullptr, nullptr};
    if ((rc = lpe_enqueue_edits(e, P, at, st))) return rc;
    return lpr_run(&P.after, P.RL, e.present, e.n_forced, e.resident, e.params, nullptr, host_out, round, want, p_max, p_max_ub, stream);
}

extern "C" int gcnn_lp_round_append(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b, int32_t present, int32_t n_forced,
                                    int32_t n_forced_entries, int32_t* row_ptr, int32_t* row_col, double* row_val, double* row_lhs,
                                    double* row_rhs, const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst,
                                    const gcnn_lp_resident* resident, const float* params, const void* host_in, void* host_out,
                                    void* arena, size_t arena_bytes, int32_t want_order, double p_max, double p_max_ub, void* stream) {
    if (!b) return GCNN_E_BADARG;
    const LpEdit e = {d, nullptr, b, present, n_forced, n_forced_entries, {}, {row_ptr, row_col, row_val, row_lhs, row_rhs},
                      src, nullptr, dst, resident, params};
    return lpe_call(e, host_in, host_out, arena, arena_bytes, want_order, p_max, p_max_ub, stream);
}

extern "C" int gcnn_lp_round_remove(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, int32_t present,
                                    int32_t n_forced, int32_t n_forced_entries, const int32_t* row_ptr, const int32_t* row_col,
                                    const double* row_val, const double* row_lhs, const double* row_rhs, int32_t* out_ptr,
                                    int32_t* out_col, double* out_val, double* out_lhs, double* out_rhs, const gcnn_lp_rows_set* src,
                                    const gcnn_lp_rows_set* transit, const gcnn_lp_rows_set* dst, const gcnn_lp_resident* resident,
                                    const float* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes,
                                    int32_t want_order, double p_max, double p_max_ub, void* stream) {
    if (!m) return GCNN_E_BADARG;
    const LpEdit e = {d, m, b, present, n_forced, n_forced_entries, {row_ptr, row_col, row_val, row_lhs, row_rhs},
                      {out_ptr, out_col, out_val, out_lhs, out_rhs}, src, transit, dst, resident, params};
    return lpe_call(e, host_in, host_out, arena, arena_bytes, want_order, p_max, p_max_ub, stream);
}

