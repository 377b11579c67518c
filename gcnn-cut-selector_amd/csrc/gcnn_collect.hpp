// gcnn_collect.hpp -- host side of gcnn_lp_collect (include/gcnn_hip.h): the data collector's expert round (data_collector.py:101-195)
// in one call -- the sample's state from a raw LP snapshot AND the plugin's ranking and parallelism filter over the caller's float64
// quality.  ONE upload, at most six launches, ONE download; it never waits on the host and allocates nothing.  No new kernel: the
// state is lp_launch (gcnn_lpstate.hpp: k_lp_stats, k_lp_emit), the rows in input cut order are k_hyb_stats / k_hyb_emit on a
// one-entry table whose eight array positions point INTO the uploaded LP snapshot (an LP snapshot holds every field of a cut
// snapshot, so nothing goes up twice), the pair bits are k_sel_pairs on those rows, and the filter is k_hyb_filter with its key
// pointer on the uploaded quality instead of the hybrid one.  Included from gcnn_capi.hip's list of host files, after
// gcnn_hybrid.hpp (it uses that file's table and scratch carving, gcnn_lpstate.hpp's layout and launch, gcnn_select.hpp's SelArgs
// builder), kept apart so that its launch names form their own inventory (tests/test_collect_build.py).
//
// The arena: the upload | the output block | the fp32 rows (row_ptr, row_col, row_val) | the pair bits | the LP scratch | the hybrid scratch.
// The upload: the packed LP snapshot | the quality [K] f64 | the forced rows | the table (HybHead, one HybEntry).

static_assert(GCNN_LP_COLLECT_OUTPUTS == 14, "gcnn_lp_collect_layout::out_off");

// where the eight arrays of a cut snapshot (GCNN_HYBRID_* order) lie in a packed LP snapshot
static const int collect_lp_array[GCNN_HYBRID_ARRAYS] = {GCNN_LP_CUT_PTR, GCNN_LP_CUT_COL, GCNN_LP_CUT_VAL, GCNN_LP_CUT_LHS,
                                                         GCNN_LP_CUT_RHS, GCNN_LP_COL_TYPE, GCNN_LP_COL_OBJ, GCNN_LP_COL_LP};

static gcnn_hybrid_dims collect_hyb_dims(const gcnn_lp_dims* d) {
    gcnn_hybrid_dims h; memset(&h, 0, sizeof(h));
    h.n_cols = d->n_cols; h.n_cuts = d->n_cuts; h.cut_nnz = d->cut_nnz; h.infinity = d->infinity;
    return h;
}

static int collect_layout(const gcnn_lp_dims* d, int32_t n_forced, int32_t n_forced_entries, gcnn_lp_collect_layout* L) {
    if (!L || n_forced < 0 || n_forced_entries < 0 || (n_forced == 0 && n_forced_entries > 0)) return GCNN_E_BADARG;
    if (!lp_dims_ok(d)) return GCNN_E_BADARG;
    if (d->n_cuts > SEL_MAX_CUTS || d->n_state_rows > (1 << 24) || d->n_cols > (1 << 24) || n_forced > (1 << 24))
        return GCNN_E_UNSUPPORTED;
    gcnn_lp_layout LL;
    int rc = lp_layout(d, n_forced, n_forced_entries, &LL);     // (its single call's part may stay unfilled: only snap_* and forced_off are read)
    if (rc) return rc;
    memset(L, 0, sizeof(*L));
    const size_t C = d->n_state_rows, V = d->n_cols, K = d->n_cuts, E1 = d->n_state_edges, E2 = d->cut_nnz;
    const size_t q_bytes = al16(8 * K);
    for (int i = 0; i < GCNN_LP_ARRAYS; ++i) L->snap_off[i] = LL.snap_off[i];
    L->quality_off = al16(LL.snap_bytes);
    for (int i = 0; i < 3; ++i) L->forced_off[i] = LL.forced_off[i] + q_bytes;     // the LP call's forced block, moved behind the quality
    L->table_off = al16(LL.in_bytes + q_bytes);
    L->table_bytes = sizeof(HybHead) + sizeof(HybEntry);
    L->in_bytes = L->table_off + L->table_bytes;
    Carver out{0};
    const size_t sizes[GCNN_LP_COLLECT_OUTPUTS] = {16 * C, 8 * E1, 4 * E1, 56 * V, 24 * K, 8 * E2, 4 * E2,     // the seven state arrays
                                                   4 * K, 16,                                                  // cut_index, LP flags
                                                   8 * K, 24 * K, 4 * K, 16, 16};   // hybrid quality, features, order, n_kept, hybrid flags
    for (int i = 0; i < GCNN_LP_COLLECT_OUTPUTS; ++i) L->out_off[i] = out.take(sizes[i], 16);
    L->out_bytes = out.off;
    Carver dev{0};
    dev.take(L->in_bytes, 256);                                // the upload lies at the arena's start
    L->out_dev_off = dev.take(L->out_bytes, 256);
    L->rows_off[0] = dev.take(4 * (K + 1), 256); L->rows_off[1] = dev.take(4 * E2, 256); L->rows_off[2] = dev.take(4 * E2, 256);
    L->ws_off = dev.take(select_ws_bytes((int)K, n_forced, (int)K), 256);
    L->lp_scratch_off = dev.take(LL.scratch_bytes, 256);
    const gcnn_hybrid_dims hd = collect_hyb_dims(d);
    L->hyb_scratch_off = dev.take(hyb_scratch(hd).bytes, 256);
    L->arena_bytes = dev.off;
    for (int i = 0; i < GCNN_HYBRID_ARRAYS; ++i) L->entry_snap[i] = L->snap_off[collect_lp_array[i]];
    return 0;
}

extern "C" int gcnn_lp_collect_layout_for(const gcnn_lp_dims* d, int32_t n_forced, int32_t n_forced_entries, gcnn_lp_collect_layout* L) {
    return layout_out(L, [&](gcnn_lp_collect_layout* l) { return collect_layout(d, n_forced, n_forced_entries, l); });
}

// the one-entry table of k_hyb_stats / k_hyb_emit: the snapshot's arrays where the LP upload put them, the outputs in the download block
static void collect_table(const gcnn_lp_dims* d, const gcnn_lp_collect_layout& L, void* table) {
    memset(table, 0, L.table_bytes);
    HybHead* h = (HybHead*)table;
    HybEntry* e = (HybEntry*)(h + 1);
    const gcnn_hybrid_dims hd = collect_hyb_dims(d);
    int ns, ne;
    hyb_blocks(hd, &ns, &ne);
    h->n = 1;
    h->blk0[0][1] = ns; h->blk0[1][1] = ne; h->c_off[1] = hd.n_cuts;
    for (int i = 0; i < GCNN_HYBRID_ARRAYS; ++i) e->snap[i] = (long long)L.entry_snap[i];
    const HybScratch sc = hyb_scratch(hd);
    e->scratch[0] = (long long)(L.hyb_scratch_off + sc.cut_stat); e->scratch[1] = (long long)(L.hyb_scratch_off + sc.cut_nint);
    e->scratch[2] = (long long)(L.hyb_scratch_off + sc.col_part); e->scratch[3] = (long long)(L.hyb_scratch_off + sc.blk_flags);
    e->dst[0] = (long long)(L.out_dev_off + L.out_off[9]); e->dst[1] = (long long)(L.out_dev_off + L.out_off[10]);
    e->dst[2] = (long long)L.rows_off[0]; e->dst[3] = (long long)L.rows_off[1]; e->dst[4] = (long long)L.rows_off[2];
    e->dst[5] = (long long)(L.out_dev_off + L.out_off[13]);
    e->infinity = hd.infinity;
    e->V = hd.n_cols; e->K = hd.n_cuts; e->nnz = hd.cut_nnz; e->ncc = lp_chunks(hd.n_cols); e->nkc = lp_chunks(hd.n_cuts);
    e->n_stat_blocks = ns; e->e0 = 0;
}

extern "C" int gcnn_lp_collect(const gcnn_lp_dims* d, int32_t n_forced, int32_t n_forced_entries, void* host_in, void* host_out,
                               void* arena, size_t arena_bytes, double p_max, double p_max_ub, void* stream) {
    gcnn_lp_collect_layout L;
    int rc = collect_layout(d, n_forced, n_forced_entries, &L);
    if (rc) return rc;
    if (!host_in || !host_out || !arena || ((uintptr_t)host_in & 15) || arena_bytes < L.arena_bytes || ((uintptr_t)arena & 255))
        return GCNN_E_BADARG;
    if (!finite_thresholds(p_max, p_max_ub)) return GCNN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    collect_table(d, L, (char*)host_in + L.table_off);
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));   // ONE upload: snapshot | quality | forced rows | table
    char* out = A + L.out_dev_off;
    auto at = [&](int i) { return out + L.out_off[i]; };
    // the state, cut_index and the LP flags straight into the download block
    rc = lp_launch(d, L.snap_off, A, A + L.lp_scratch_off, (float*)at(0), (int*)at(1), (float*)at(2), (float*)at(3), (float*)at(4),
                   (int*)at(5), (float*)at(6), (int*)at(7), (int*)at(8), nullptr, 0, st);
    if (rc) return rc;
    // the rows in input cut order, the hybrid quality and the features: the hybrid selection's two launches on the LP snapshot's arrays
    const gcnn_hybrid_dims hd = collect_hyb_dims(d);
    int n_stats, n_emit;
    hyb_blocks(hd, &n_stats, &n_emit);
    HybArgs g;
    g.table = A + L.table_off; g.base = A;
    if (n_stats > 0) {
        ProfScope prof("k_collect_stats", st);       // k_hyb_stats itself
        hipLaunchKernelGGL(k_hyb_stats, dim3(n_stats), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_collect_emit", st);        // k_hyb_emit itself
        hipLaunchKernelGGL(k_hyb_emit, dim3(n_emit), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    // the selection over the UPLOADED quality.  A flagged snapshot's rows may be partly unwritten: k_hyb_emit keeps its offsets inside
    // its own entries, k_sel_pairs ignores columns outside [0, n_cols), and the caller discards the results
    HybSelArgs a;
    a.sel = sel_args(nullptr, SelRows{(const int*)(A + L.rows_off[0]), (const int*)(A + L.rows_off[1]), (const float*)(A + L.rows_off[2]), nullptr},
                     forced_rows(A, L.forced_off), 1, d->n_cuts, n_forced, d->n_cuts, d->n_cols, p_max, p_max_ub, A + L.ws_off,
                     (int*)at(11), (int*)at(12));
    a.quality = (const double*)(A + L.quality_off); a.filter = 1;
    if (d->n_cuts > 0) {
        ProfScope prof("k_collect_pairs", st);       // k_sel_pairs itself, on the rows k_hyb_emit wrote
        hipLaunchKernelGGL(k_sel_pairs, dim3(std::min(d->n_cuts + n_forced, 65535)), dim3(SEL_NT), 0, st, a.sel);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_collect_filter", st);      // k_hyb_filter itself: sel_filter_body<double> with q on the uploaded quality
        hipLaunchKernelGGL(k_hyb_filter, dim3(1), dim3(SEL_NT), 0, st, a);
        LAUNCHCHK();
    }
    // ONE download: the state | cut_index | LP flags | hybrid quality | features | order | n_kept | hybrid flags
    HIPCHK(hipMemcpyAsync(host_out, out, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
