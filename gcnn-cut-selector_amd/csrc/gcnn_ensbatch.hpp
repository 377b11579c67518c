// gcnn_ensbatch.hpp -- host side of the many-state ensemble calls (include/gcnn_hip.h: gcnn_infer_ensemble_batch_layout_for,
// gcnn_infer_ensemble_batch, gcnn_lp_ensemble_batch_layout_for, gcnn_lp_ensemble_batch): 1..64 states, or LP snapshots, of the
// evaluators' task farm (model_evaluator.py:157-241) scored by ONE ensemble of 1..GCNN_GROUP_MAX models (the five seeds of a
// problem, model_trainer.py:38-49) in one call.  The states form gcnn_infer_batch's disjoint union; the members of the ensemble over
// that union are still the members of one group, so the call is gcnn_ensemble.hpp's with the number of states as a parameter
// (ens_layout, ens_prepare, ens_run, ens_call, lpens_call) and launches what that file launches, under that file's names: one
// upload, the index pass, the by-variable stage once, the launch tables, the M forward passes as one group, the mean, the per-state
// tail, one download.  What is this file's own is the tail of RANK mode: k_eb_mean_rank (k_ensbatch.hpp) forms the mean and ranks
// every state's segment in ONE launch where the single-state call runs two dependent ones.  Scores mode and selection mode keep the
// mean over the whole union; selection mode then runs union_tail's launch pair over all states.  Included from gcnn_capi.hip's list
// of host files after gcnn_ensemble.hpp; the one launch name it spells is its own (tests/test_ensbatch_build.py).
//
// Limits, returned before anything is enqueued: what gcnn_infer_batch / gcnn_lp_batch return for these sizes, GCNN_E_BADARG for
// n_models outside 1..GCNN_GROUP_MAX, a null params entry and a missing host_staging, GCNN_E_UNSUPPORTED for a state of more than
// 4,096 cuts in the two ordering modes and for a forward pass the group recorder cannot take.  There is no variable limit: the
// union's by-variable order is the radix sort's.
#include "k_ensbatch.hpp"

static int eb_rank_tail(const EnsCall& c, const gcnn_ibatch_layout& L, const IbAt& at, hipStream_t st) {
    EbArgs a; memset(&a, 0, sizeof(a));
    for (int m = 0; m < c.n_models; ++m) a.row[m] = c.rows[m];
    a.table = at.table; a.mean = (float*)(at.out + L.out_off[0]); a.order = (int*)(at.out + L.out_off[1]);
    a.n_models = c.n_models;
    ProfScope prof("k_eb_mean_rank", st);
    hipLaunchKernelGGL(k_eb_mean_rank, dim3(L.n_states), dim3(256), 0, st, a);
    LAUNCHCHK();
    return 0;
}

extern "C" int gcnn_infer_ensemble_batch_layout_for(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced,
                                                    const int32_t* n_forced_entries, int32_t mode, int32_t n_models,
                                                    gcnn_ensemble_layout* layout) {
    return layout_out(layout, [&](gcnn_ensemble_layout* l) { return ens_layout(n_states, dims, n_forced, n_forced_entries, mode, n_models, false, l); });
}

extern "C" int gcnn_infer_ensemble_batch(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                         int32_t mode, int32_t n_models, const float* const* params, const void* host_in, void* host_out,
                                         void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream) {
    return ens_call(n_states, dims, n_forced, n_forced_entries, mode, n_models, false, params, host_in, host_out, arena, arena_bytes,
                    host_staging, p_max, p_max_ub, eb_rank_tail, stream);
}

extern "C" int gcnn_lp_ensemble_batch_layout_for(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced,
                                                 const int32_t* n_forced_entries, int32_t mode, int32_t n_models,
                                                 gcnn_lp_ensemble_layout* layout) {
    return layout_out(layout, [&](gcnn_lp_ensemble_layout* l) { return lpens_layout(n, dims, n_forced, n_forced_entries, mode, n_models, false, l, nullptr); });
}

extern "C" int gcnn_lp_ensemble_batch(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                      int32_t mode, int32_t n_models, const float* const* params, void* host_in, void* host_out,
                                      void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream) {
    return lpens_call(n, dims, n_forced, n_forced_entries, mode, n_models, false, params, host_in, host_out, arena, arena_bytes,
                      host_staging, p_max, p_max_ub, eb_rank_tail, stream);
}
