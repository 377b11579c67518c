// gcnn_lpbatch.hpp -- host side of gcnn_lp_batch (include/gcnn_hip.h): 1..64 raw LP snapshots in one upload, their states built in
// the arena by one pair of launches (k_lpbatch.hpp) exactly where gcnn_infer_batch's upload would have put them, then that call's
// run half (ibatch_run) unchanged, one download.  Included from gcnn_capi.hip's list of host files, after gcnn_lpstate.hpp and
// gcnn_ibatch.hpp (it shares their statics), kept apart so that its launch names form their own inventory
// (tests/test_lpbatch_build.py).  What a call that builds its union from snapshots needs whichever union it is -- the layout
// (lpset_layout), the descriptor table (lpset_fill), the builder launches' arguments (lpset_launch) and where the built union lies
// (lpset_at) -- takes the union's layout and the size of its table as parameters: gcnn_lpmodels.hpp, included after this file,
// uses them with gcnn_infer_models' union.
//
// The arena: the union's layout for the built states' sizes (gcnn_ibatch_layout; its table and forced slots stay unused, its zero
// block and seven arrays are written by the device, never uploaded) | the upload | the output block | the snapshots' scratch.
// The upload: the union's table | the descriptor table | the packed snapshots | the forced rows.
#include "k_lpbatch.hpp"

static_assert(LPSET_MAX == GCNN_IBATCH_MAX && LPSET_TS == GCNN_IBATCH_TABLE_STRIDE, "one descriptor per state of the union");
static_assert(GCNN_LP_ARRAYS == 22, "LpSetEntry::snap");

static const size_t LPSET_IB_TABLE = 4 * (size_t)IB_COLS * IB_TS;     // gcnn_lp_batch: the union's table comes first in the upload

// lpset_layout: the layout of a call that builds its union from snapshots.  `front`: the bytes of the union's table, which lie in
// front of the descriptor table in the upload; `union_of(sd, &L->state)`: the union's own layout for the built states' sizes
// (gcnn_infer_batch's here; gcnn_infer_models' in gcnn_lpmodels.hpp, included after this file).
template <class UnionOf>
static int lpset_layout(int n, const gcnn_lp_dims* dims, size_t front, UnionOf union_of, gcnn_lp_batch_layout* L,
                        gcnn_lp_layout* each /* [n], optional */) {
    if (!L || !dims || n < 1 || n > GCNN_IBATCH_MAX) return GCNN_E_BADARG;
    gcnn_dims sd[GCNN_IBATCH_MAX];
    for (int s = 0; s < n; ++s) {
        if (!lp_dims_ok(&dims[s])) return GCNN_E_BADARG;
        sd[s] = lp_state_dims(&dims[s]);
    }
    memset(L, 0, sizeof(*L));
    int rc = union_of(sd, &L->state);
    if (rc) return rc;
    const gcnn_ibatch_layout& S = L->state;
    L->n_snapshots = n;
    L->table_bytes = front + sizeof(LpSetHead) + (size_t)n * sizeof(LpSetEntry);
    Carver in{0}, scratch{0};
    in.take(L->table_bytes, 16);
    for (int s = 0; s < n; ++s) {
        gcnn_lp_layout one;
        if ((rc = lp_layout(&dims[s], -1, 0, &one))) return rc;
        L->snap_base[s] = in.take(one.snap_bytes, 16);
        L->scratch_base[s] = scratch.take(one.scratch_bytes, 256);
        if (each) each[s] = one;
    }
    forced_block(in, S.n_forced, S.n_forced_entries, L->forced_off);
    L->in_bytes = in.off;
    const size_t K = S.total.n_cuts;
    for (int i = 0; i < 4; ++i) L->out_off[i] = S.out_off[i];
    L->out_off[4] = S.out_bytes; L->out_off[5] = L->out_off[4] + 16 * (size_t)n;
    L->out_bytes = L->out_off[5] + al16(4 * K);
    Carver dev{(S.arena_bytes + 255) & ~(size_t)255};
    L->up_off = dev.take(L->in_bytes, 256);
    L->out_dev_off = dev.take(L->out_bytes, 256);
    L->scratch_off = dev.take(scratch.off, 256);
    L->arena_bytes = dev.off;
    return 0;
}

static int lpbatch_layout(int n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode,
                          gcnn_lp_batch_layout* L, gcnn_lp_layout* each) {
    return lpset_layout(n, dims, LPSET_IB_TABLE, [&](const gcnn_dims* sd, gcnn_ibatch_layout* S) {
        return ibatch_layout(n, sd, n_forced, n_forced_entries, mode, S); }, L, each);
}

extern "C" int gcnn_lp_batch_layout_for(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                        int32_t mode, gcnn_lp_batch_layout* L) {
    return layout_out(L, [&](gcnn_lp_batch_layout* l) { return lpbatch_layout(n, dims, n_forced, n_forced_entries, mode, l, nullptr); });
}

static void lpset_blocks(const gcnn_lp_dims& d, int* stats, int* emit) {
    const int nrc = lp_chunks(d.n_rows), ncc = lp_chunks(d.n_cols), nkc = lp_chunks(d.n_cuts);
    *stats = std::max(1, ncc + nrc + nkc); *emit = nrc + nkc + 1;
}

// lpset_fill: the descriptor table behind the union's table (`front` bytes, already written: its columns say where state s lies)
static void lpset_fill(int n, const gcnn_lp_dims* dims, const gcnn_lp_batch_layout& L, const gcnn_lp_layout* each, size_t front,
                       void* table) {
    const int32_t* ib = (const int32_t*)table;
    LpSetHead* h = (LpSetHead*)((char*)table + front);
    LpSetEntry* e = (LpSetEntry*)(h + 1);
    const gcnn_ibatch_layout& S = L.state;
    h->n = n;
    int b_stats = 0, b_emit = 0;
    for (int s = 0; s < n; ++s, ++e) {
        const gcnn_lp_dims& d = dims[s];
        int ns, ne;
        lpset_blocks(d, &ns, &ne);
        h->blk0[0][s] = b_stats; h->blk0[1][s] = b_emit;
        b_stats += ns; b_emit += ne;
        const size_t snap = L.up_off + L.snap_base[s];
        for (int i = 0; i < GCNN_LP_ARRAYS; ++i) e->snap[i] = (long long)(snap + each[s].snap_off[i]);
        const LpScratch sc = lp_scratch(&d);
        const size_t sb = L.scratch_off + L.scratch_base[s];
        const size_t parts[7] = {sc.row_stat, sc.cut_stat, sc.col_part, sc.row_part, sc.cut_part, sc.cut_aux, sc.blk_flags};
        for (int i = 0; i < 7; ++i) e->scratch[i] = (long long)(sb + parts[i]);
        const size_t c0 = ib[IB_C * IB_TS + s], v0 = ib[IB_V * IB_TS + s], k0 = ib[IB_K * IB_TS + s];
        const size_t e1 = ib[IB_E1 * IB_TS + s], e2 = ib[IB_E2 * IB_TS + s];
        // where the union's upload keeps state s: features at the union's rows, each edge list as the state's own [2,E_s] block
        const size_t dst[9] = {S.in_off[2] + 16 * c0, S.in_off[3] + 8 * e1, S.in_off[4] + 4 * e1, S.in_off[5] + 56 * v0,
                               S.in_off[6] + 24 * k0, S.in_off[7] + 8 * e2, S.in_off[8] + 4 * e2,
                               L.out_dev_off + L.out_off[5] + 4 * k0, L.out_dev_off + L.out_off[4] + 16 * (size_t)s};
        for (int i = 0; i < 9; ++i) e->dst[i] = (long long)dst[i];
        e->infinity = d.infinity; e->eps = d.sum_epsilon; e->obj_norm = d.obj_norm;
        e->R = d.n_rows; e->V = d.n_cols; e->K = d.n_cuts; e->nnz_r = d.row_nnz; e->nnz_k = d.cut_nnz;
        e->has_inc = d.has_incumbent != 0; e->n_model_vars = d.n_model_vars; e->C = d.n_state_rows; e->E1 = d.n_state_edges;
        e->nrc = lp_chunks(d.n_rows); e->ncc = lp_chunks(d.n_cols); e->nkc = lp_chunks(d.n_cuts); e->n_stat_blocks = ns;
    }
    h->blk0[0][n] = b_stats; h->blk0[1][n] = b_emit;
}

extern "C" int gcnn_lp_batch_fill_table(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                        int32_t mode, void* table) {
    if (!table) return GCNN_E_BADARG;
    gcnn_lp_batch_layout L;
    gcnn_lp_layout each[GCNN_IBATCH_MAX];
    int rc = lpbatch_layout(n, dims, n_forced, n_forced_entries, mode, &L, each);
    if (rc) return rc;
    gcnn_dims sd[GCNN_IBATCH_MAX];
    for (int s = 0; s < n; ++s) sd[s] = lp_state_dims(&dims[s]);
    memset(table, 0, L.table_bytes);
    if ((rc = ibatch_sums(n, sd, n_forced, n_forced_entries, mode, nullptr, (int32_t*)table))) return rc;
    lpset_fill(n, dims, L, each, LPSET_IB_TABLE, table);
    return 0;
}

// What the two builder launches take for an upload that lies at L.up_off (`front` as in lpset_layout), and their grids.  They
// clear the union's zero block, whichever union's it is.
static LpSetArgs lpset_launch(int n, const gcnn_lp_dims* dims, const gcnn_lp_batch_layout& L, size_t front, char* A, int* n_stats,
                              int* n_emit) {
    const gcnn_ibatch_layout& S = L.state;
    *n_stats = *n_emit = 0;
    for (int s = 0; s < n; ++s) {
        int a, b;
        lpset_blocks(dims[s], &a, &b);
        *n_stats += a; *n_emit += b;
    }
    LpSetArgs g;
    g.table = A + L.up_off + front; g.base = A;
    g.zero = (int*)(A + S.in_off[1]); g.zero_words = (int)((S.in_off[2] - S.in_off[1]) / 4);
    return g;
}

// where the union lies once they have run: the table and the forced rows in the upload, the zero block and the seven arrays at the
// union's own positions, the output block behind the upload
static IbAt lpset_at(char* A, const gcnn_lp_batch_layout& L) {
    const gcnn_ibatch_layout& S = L.state;
    char* up = A + L.up_off;
    IbAt at;
    at.table = (const int*)up; at.zero = A + S.in_off[1];
    for (int i = 0; i < 7; ++i) at.arr[i] = A + S.in_off[2 + i];
    for (int i = 0; i < 3; ++i) at.forced[i] = up + L.forced_off[i];
    at.out = A + L.out_dev_off;
    return at;
}

extern "C" int gcnn_lp_batch(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int32_t mode,
                             const float* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max,
                             double p_max_ub, void* stream) {
    gcnn_lp_batch_layout L;
    int rc = lpbatch_layout(n, dims, n_forced, n_forced_entries, mode, &L, nullptr);
    if (rc) return rc;
    const gcnn_ibatch_layout& S = L.state;
    if ((rc = call_check(params, host_in, host_out, arena, arena_bytes, L.arena_bytes, mode == GCNN_IBATCH_SELECT, p_max, p_max_ub))) return rc;
    if ((rc = ibatch_precheck(S, params, arena))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    HIPCHK(hipMemcpyAsync(A + L.up_off, host_in, L.in_bytes, hipMemcpyHostToDevice, st));   // ONE upload: tables | snapshots | forced rows
    int n_stats, n_emit;
    const LpSetArgs g = lpset_launch(n, dims, L, LPSET_IB_TABLE, A, &n_stats, &n_emit);
    {
        ProfScope prof("k_lpset_stats", st);
        hipLaunchKernelGGL(k_lpset_stats, dim3(n_stats), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_lpset_emit", st);
        hipLaunchKernelGGL(k_lpset_emit, dim3(n_emit), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    // A flagged snapshot leaves parts of its own state unwritten: they keep what the arena held.  k_ib_unpack confines whatever ids
    // lie there to the state's own ranges, and the caller discards that state's results once an LP flag is set.
    const IbAt at = lpset_at(A, L);
    if ((rc = ibatch_run(n, mode, S, params, A, at, p_max, p_max_ub, st))) return rc;
    // ONE download: scores | order | n_kept | batch flags | LP flags | cut_index
    HIPCHK(hipMemcpyAsync(host_out, at.out, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
