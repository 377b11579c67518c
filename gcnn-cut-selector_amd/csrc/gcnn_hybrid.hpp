// gcnn_hybrid.hpp -- host side of gcnn_hybrid_select (include/gcnn_hip.h): SCIP's hybrid quality and the parallelism filter from the cut
// rows of 1..64 snapshots in one upload, at most four launches (k_hybrid.hpp, k_sel_pairs unchanged) and one download.  No model, no
// LP rows.  Included from gcnn_capi.hip's list of host files, after gcnn_lpbatch.hpp (it shares that file's table conventions,
// gcnn_lpstate.hpp's chunking and gcnn_select.hpp's SelArgs builder and workspace size), kept apart so that its launch names form
// their own inventory (tests/test_hybrid_build.py).
//
// The arena: the upload | the output block | the stacked fp32 rows (row_ptr, row_col, row_val) | the pair bits | the snapshots' scratch.
// The upload: the table (head, one entry per snapshot) | the packed snapshots | the forced rows.
#include "k_hybrid.hpp"

static_assert(GCNN_HYBRID_ARRAYS == 8, "HybEntry::snap");

static bool hyb_dims_ok(const gcnn_hybrid_dims& d) {
    return d.n_cols >= 0 && d.n_cuts >= 0 && d.cut_nnz >= 0 && d.infinity > 0.0;
}
static void hyb_blocks(const gcnn_hybrid_dims& d, int* stats, int* emit) {
    *stats = lp_chunks(d.n_cols) + lp_chunks(d.n_cuts); *emit = lp_chunks(d.n_cuts) + 1;
}
// scratch carving of one snapshot: cut_stat | cut_nint | col_part | blk_flags
struct HybScratch { size_t cut_stat, cut_nint, col_part, blk_flags, bytes; };
static HybScratch hyb_scratch(const gcnn_hybrid_dims& d) {
    HybScratch s; Carver c{0};
    s.cut_stat = c.take(32 * (size_t)d.n_cuts, 16);
    s.cut_nint = c.take(4 * (size_t)d.n_cuts, 16);
    s.col_part = c.take(8 * (size_t)(lp_chunks(d.n_cols) + 1), 16);
    s.blk_flags = c.take(4 * (size_t)(lp_chunks(d.n_cols) + lp_chunks(d.n_cuts) + 1), 16);
    s.bytes = c.off;
    return s;
}

static int hyb_layout(int n, const gcnn_hybrid_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode,
                      gcnn_hybrid_layout* L) {
    if (!L || !dims || n < 1 || n > GCNN_IBATCH_MAX || mode < GCNN_HYBRID_QUALITY || mode > GCNN_HYBRID_SELECT) return GCNN_E_BADARG;
    const bool select = mode == GCNN_HYBRID_SELECT;
    if (select && (n_forced == nullptr) != (n_forced_entries == nullptr)) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    int64_t K = 0, E = 0, F = 0, FE = 0;
    int max_cuts = 0, max_cols = 0;
    for (int s = 0; s < n; ++s) {
        if (!hyb_dims_ok(dims[s])) return GCNN_E_BADARG;
        if (mode != GCNN_HYBRID_QUALITY && dims[s].n_cuts > SEL_MAX_CUTS) return GCNN_E_UNSUPPORTED;
        K += dims[s].n_cuts; E += dims[s].cut_nnz;
        max_cuts = std::max(max_cuts, dims[s].n_cuts); max_cols = std::max(max_cols, dims[s].n_cols);
        if (select && n_forced) {
            if (n_forced[s] < 0 || n_forced_entries[s] < 0 || (n_forced[s] == 0 && n_forced_entries[s] > 0)) return GCNN_E_BADARG;
            F += n_forced[s]; FE += n_forced_entries[s];
        }
    }
    if (K > (1 << 30) || E > (1 << 30) || F > (1 << 30) || FE > (1 << 30)) return GCNN_E_UNSUPPORTED;
    L->n_snapshots = n; L->total_cuts = (int)K; L->total_nnz = (int)E; L->max_cuts = max_cuts; L->max_cols = max_cols;
    L->n_forced = (int)F; L->n_forced_entries = (int)FE;
    L->table_bytes = sizeof(HybHead) + (size_t)n * sizeof(HybEntry);
    Carver in{0}, scratch{0};
    in.take(L->table_bytes, 16);
    for (int s = 0; s < n; ++s) {
        const size_t V = dims[s].n_cols, k = dims[s].n_cuts, e = dims[s].cut_nnz;
        const size_t sizes[GCNN_HYBRID_ARRAYS] = {4 * (k + 1), 4 * e, 8 * e, 8 * k, 8 * k, V, 8 * V, 8 * V};
        for (int i = 0; i < GCNN_HYBRID_ARRAYS; ++i) L->snap_off[s][i] = in.take(sizes[i], 16);
        L->scratch_base[s] = scratch.take(hyb_scratch(dims[s]).bytes, 256);
    }
    forced_block(in, (size_t)F, (size_t)FE, L->forced_off);
    L->in_bytes = in.off;
    Carver out{0};
    L->out_off[0] = out.take(8 * (size_t)K, 16); L->out_off[1] = out.take(24 * (size_t)K, 16); L->out_off[2] = out.take(4 * (size_t)K, 16);
    L->out_off[3] = out.take(4 * (size_t)n, 16); L->out_off[4] = out.take(16 * (size_t)n, 16);
    L->out_bytes = out.off;
    Carver dev{0};
    dev.take(L->in_bytes, 256);
    L->out_dev_off = dev.take(L->out_bytes, 256);
    L->rows_off[0] = dev.take(4 * ((size_t)K + 1), 256); L->rows_off[1] = dev.take(4 * (size_t)E, 256); L->rows_off[2] = dev.take(4 * (size_t)E, 256);
    L->ws_off = dev.take(select ? select_ws_bytes((int)K, (int)F, max_cuts) : 0, 256);
    L->scratch_off = dev.take(scratch.off, 256);
    L->arena_bytes = dev.off;
    return 0;
}

extern "C" int gcnn_hybrid_layout_for(int32_t n, const gcnn_hybrid_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                      int32_t mode, gcnn_hybrid_layout* L) {
    return layout_out(L, [&](gcnn_hybrid_layout* l) { return hyb_layout(n, dims, n_forced, n_forced_entries, mode, l); });
}

extern "C" int gcnn_hybrid_fill_table(int32_t n, const gcnn_hybrid_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                      int32_t mode, void* table) {
    if (!table) return GCNN_E_BADARG;
    gcnn_hybrid_layout L;
    int rc = hyb_layout(n, dims, n_forced, n_forced_entries, mode, &L);
    if (rc) return rc;
    memset(table, 0, L.table_bytes);
    HybHead* h = (HybHead*)table;
    HybEntry* e = (HybEntry*)(h + 1);
    h->n = n;
    int b_stats = 0, b_emit = 0, k0 = 0, e0 = 0, f0 = 0;
    for (int s = 0; s < n; ++s, ++e) {
        const gcnn_hybrid_dims& d = dims[s];
        int ns, ne;
        hyb_blocks(d, &ns, &ne);
        h->blk0[0][s] = b_stats; h->blk0[1][s] = b_emit; h->c_off[s] = k0; h->f_off[s] = f0;
        for (int i = 0; i < GCNN_HYBRID_ARRAYS; ++i) e->snap[i] = (long long)L.snap_off[s][i];   // the upload lies at the arena's start
        const HybScratch sc = hyb_scratch(d);
        const size_t sb = L.scratch_off + L.scratch_base[s];
        e->scratch[0] = (long long)(sb + sc.cut_stat); e->scratch[1] = (long long)(sb + sc.cut_nint);
        e->scratch[2] = (long long)(sb + sc.col_part); e->scratch[3] = (long long)(sb + sc.blk_flags);
        e->dst[0] = (long long)(L.out_dev_off + L.out_off[0] + 8 * (size_t)k0);
        e->dst[1] = (long long)(L.out_dev_off + L.out_off[1] + 24 * (size_t)k0);
        e->dst[2] = (long long)(L.rows_off[0] + 4 * (size_t)k0);
        e->dst[3] = (long long)(L.rows_off[1] + 4 * (size_t)e0);
        e->dst[4] = (long long)(L.rows_off[2] + 4 * (size_t)e0);
        e->dst[5] = (long long)(L.out_dev_off + L.out_off[4] + 16 * (size_t)s);
        e->infinity = d.infinity;
        e->V = d.n_cols; e->K = d.n_cuts; e->nnz = d.cut_nnz; e->ncc = lp_chunks(d.n_cols); e->nkc = lp_chunks(d.n_cuts);
        e->n_stat_blocks = ns; e->e0 = e0;
        b_stats += ns; b_emit += ne; k0 += d.n_cuts; e0 += d.cut_nnz;
        if (mode == GCNN_HYBRID_SELECT && n_forced) f0 += n_forced[s];
    }
    h->blk0[0][n] = b_stats; h->blk0[1][n] = b_emit; h->c_off[n] = k0; h->f_off[n] = f0;
    return 0;
}

extern "C" int gcnn_hybrid_select(int32_t n, const gcnn_hybrid_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                  int32_t mode, const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max,
                                  double p_max_ub, void* stream) {
    gcnn_hybrid_layout L;
    int rc = hyb_layout(n, dims, n_forced, n_forced_entries, mode, &L);
    if (rc) return rc;
    if (!host_in || !host_out || !arena || arena_bytes < L.arena_bytes || ((uintptr_t)arena & 255)) return GCNN_E_BADARG;
    if (mode == GCNN_HYBRID_SELECT && !finite_thresholds(p_max, p_max_ub)) return GCNN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));   // ONE upload: table | snapshots | forced rows
    int n_stats = 0, n_emit = 0;
    for (int s = 0; s < n; ++s) {
        int a, b;
        hyb_blocks(dims[s], &a, &b);
        n_stats += a; n_emit += b;
    }
    HybArgs g;
    g.table = A; g.base = A;
    if (n_stats > 0) {
        ProfScope prof("k_hyb_stats", st);
        hipLaunchKernelGGL(k_hyb_stats, dim3(n_stats), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_hyb_emit", st);
        hipLaunchKernelGGL(k_hyb_emit, dim3(n_emit), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    char* out = A + L.out_dev_off;
    if (mode != GCNN_HYBRID_QUALITY) {
        const HybHead* h = (const HybHead*)A;      // (device addresses of the table's offset columns)
        const bool select = mode == GCNN_HYBRID_SELECT;
        const int F = select ? L.n_forced : 0;
        HybSelArgs a;
        a.sel = sel_args(nullptr, SelRows{(const int*)(A + L.rows_off[0]), (const int*)(A + L.rows_off[1]), (const float*)(A + L.rows_off[2]), h->c_off},
                         SelRows{(const int*)(A + L.forced_off[0]), (const int*)(A + L.forced_off[1]), (const float*)(A + L.forced_off[2]),
                                 F > 0 ? h->f_off : nullptr},
                         n, L.total_cuts, F, L.max_cuts, L.max_cols, p_max, p_max_ub, A + L.ws_off, (int*)(out + L.out_off[2]),
                         (int*)(out + L.out_off[3]));
        a.quality = (const double*)(out + L.out_off[0]); a.filter = select;
        // a flagged snapshot's rows may be partly unwritten: k_hyb_emit keeps its offsets inside its own entries, k_sel_pairs
        // ignores columns outside [0, max_cols), and the caller discards that snapshot's results
        if (select && L.total_cuts > 0) {
            ProfScope prof("k_hyb_pairs", st);   // k_sel_pairs itself, on the rows k_hyb_emit wrote
            hipLaunchKernelGGL(k_sel_pairs, dim3(std::min(L.total_cuts + F, 65535)), dim3(SEL_NT), 0, st, a.sel);
            LAUNCHCHK();
        }
        ProfScope prof("k_hyb_filter", st);
        hipLaunchKernelGGL(k_hyb_filter, dim3(n), dim3(SEL_NT), 0, st, a);
        LAUNCHCHK();
    }
    // ONE download: quality | features | order | n_kept | flags
    HIPCHK(hipMemcpyAsync(host_out, out, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
