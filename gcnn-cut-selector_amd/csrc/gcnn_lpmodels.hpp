// gcnn_lpmodels.hpp -- host side of gcnn_lp_models (include/gcnn_hip.h): gcnn_lp_batch's contract for 1..64 raw LP snapshots that
// belong to 1..GCNN_GROUP_MAX models -- what a scoring server holds when the evaluators' task farm runs with `seed` as its innermost
// loop (model_evaluator.py:211-219) and the workers send snapshots.  Pure composition, no kernel of its own: the host half of
// gcnn_infer_models (mbatch_prepare: nothing enqueued), one upload, the two builder launches of gcnn_lp_batch (k_lpset_stats /
// k_lpset_emit, recorded here as k_lpm_stats / k_lpm_emit) which leave every state where gcnn_infer_models' upload would have put it
// and clear that union's zero block (the models' larger one), then mbatch_run unchanged, one download.  Included from gcnn_capi.hip's
// list of host files, after gcnn_lpbatch.hpp (lpset_layout, lpset_fill, lpset_launch, lpset_at) and gcnn_mbatch.hpp (mbatch_layout,
// mbatch_prepare, mbatch_run).  Kept apart so that its launch names form their own inventory (tests/test_lpmodels_build.py).
//
// The arena: gcnn_infer_models' layout for the built states' sizes (its table and forced slots stay unused, its zero block and seven
// arrays are written by the device, never uploaded) | the upload | the output block | the snapshots' scratch.
// The upload: the union's table with its model words | the descriptor table | the packed snapshots | the forced rows.

static const size_t LPM_MB_TABLE = 4 * (size_t)MB_TABLE_WORDS;         // the union's table comes first in the upload
static_assert(LPM_MB_TABLE % 16 == 0, "the descriptor table is read as 16-byte records");

static int lpm_layout(int n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode,
                      int n_models, const int32_t* model_of_snapshot, gcnn_lp_models_layout* L, gcnn_lp_layout* each) {
    if (!L) return GCNN_E_BADARG;
    return lpset_layout(n, dims, LPM_MB_TABLE, [&](const gcnn_dims* sd, gcnn_ibatch_layout* S) {
        const int rc = mbatch_layout(n, sd, n_forced, n_forced_entries, mode, n_models, model_of_snapshot, &L->models);
        if (!rc) *S = L->models.u;
        return rc; }, &L->lp, each);
}

extern "C" int gcnn_lp_models_layout_for(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                         int32_t mode, int32_t n_models, const int32_t* model_of_snapshot, gcnn_lp_models_layout* L) {
    return layout_out(L, [&](gcnn_lp_models_layout* l) { return lpm_layout(n, dims, n_forced, n_forced_entries, mode, n_models, model_of_snapshot, l, nullptr); });
}

extern "C" int gcnn_lp_models_fill_table(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                         int32_t mode, int32_t n_models, const int32_t* model_of_snapshot, void* table) {
    if (!table) return GCNN_E_BADARG;
    gcnn_lp_models_layout L;
    gcnn_lp_layout each[GCNN_IBATCH_MAX];
    int rc = lpm_layout(n, dims, n_forced, n_forced_entries, mode, n_models, model_of_snapshot, &L, each);
    if (rc) return rc;
    gcnn_dims sd[GCNN_IBATCH_MAX];
    for (int s = 0; s < n; ++s) sd[s] = lp_state_dims(&dims[s]);
    memset(table, 0, L.lp.table_bytes);
    // (forced rows are counted in selection mode only, as gcnn_lp_batch_fill_table counts them)
    const bool sel = mode == GCNN_IBATCH_SELECT;
    if ((rc = gcnn_infer_models_fill_table(n, sd, sel ? n_forced : nullptr, sel ? n_forced_entries : nullptr, n_models,
                                           model_of_snapshot, (int32_t*)table))) return rc;
    lpset_fill(n, dims, L.lp, each, LPM_MB_TABLE, table);
    return 0;
}

extern "C" int gcnn_lp_models(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int32_t mode,
                              int32_t n_models, const int32_t* model_of_snapshot, const float* const* params, const void* host_in,
                              void* host_out, void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub,
                              void* stream) {
    gcnn_lp_models_layout L;
    int rc = lpm_layout(n, dims, n_forced, n_forced_entries, mode, n_models, model_of_snapshot, &L, nullptr);
    if (rc) return rc;
    if (!params || !host_staging) return GCNN_E_BADARG;
    if ((rc = call_check(params[0], host_in, host_out, arena, arena_bytes, L.lp.arena_bytes, mode == GCNN_IBATCH_SELECT, p_max, p_max_ub))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    const IbAt at = lpset_at(A, L.lp);
    static thread_local MbCall call;
    if ((rc = mbatch_prepare(n, mode, L.models, params, A, at, host_staging, st, &call))) return rc;   // host work only
    HIPCHK(hipMemcpyAsync(A + L.lp.up_off, host_in, L.lp.in_bytes, hipMemcpyHostToDevice, st));   // upload 1: tables | snapshots | forced rows
    int n_stats, n_emit;
    const LpSetArgs g = lpset_launch(n, dims, L.lp, LPM_MB_TABLE, A, &n_stats, &n_emit);
    {
        ProfScope prof("k_lpm_stats", st);
        hipLaunchKernelGGL(k_lpset_stats, dim3(n_stats), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_lpm_emit", st);
        hipLaunchKernelGGL(k_lpset_emit, dim3(n_emit), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    // A flagged snapshot leaves parts of its own state unwritten: the index pass confines whatever ids lie there to the state's own
    // ranges, as in gcnn_lp_batch, and the caller discards that state's results once an LP flag is set.
    if ((rc = mbatch_run(n, mode, L.models, A, at, host_staging, call, p_max, p_max_ub, st))) return rc;
    // ONE download: scores | order | n_kept | batch flags | LP flags | cut_index
    HIPCHK(hipMemcpyAsync(host_out, at.out, L.lp.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
