// gcnn_rank.hpp -- host side of the test-set ranking (k_rank.hpp): gcnn_rank_deviations.  Included at the end of gcnn_capi.hip (it
// shares that file's ProfScope), but kept apart so that its launch name forms its own inventory (tests/test_rank_build.py).
#include "k_rank.hpp"

extern "C" int gcnn_rank_deviations(const int32_t* offsets, int32_t n_samples, const float* truth32, const double* truth64,
                                    const float* scores, int32_t n_scores, const double* hybrid, const int32_t* perms,
                                    int32_t n_perms, int32_t* deviations, void* stream) {
    if (n_samples < 1 || !offsets || !deviations) return GCNN_E_BADARG;
    if (n_scores < 0 || n_scores > RM_MAX_SETS || n_perms < 0 || n_perms > RM_MAX_SETS) return GCNN_E_BADARG;
    if (n_scores == 0 && !hybrid && n_perms == 0) return GCNN_E_BADARG;
    if (n_scores > 0 && (!scores || !truth32)) return GCNN_E_BADARG;
    if (n_perms > 0 && !perms) return GCNN_E_BADARG;
    if ((hybrid || n_perms > 0) && !truth64) return GCNN_E_BADARG;
    RankMultiArgs a;
    a.offsets = offsets; a.n_samples = n_samples;
    a.truth32 = n_scores > 0 ? truth32 : nullptr; a.truth64 = (hybrid || n_perms > 0) ? truth64 : nullptr;
    a.scores = n_scores > 0 ? scores : nullptr; a.n_scores = n_scores;
    a.hybrid = hybrid;
    a.perms = n_perms > 0 ? perms : nullptr; a.n_perms = n_perms;
    a.dev = deviations;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("k_rank_multi", st);
    hipLaunchKernelGGL(k_rank_multi, dim3(n_samples), dim3(RM_NT), 0, st, a);
    LAUNCHCHK();
    return 0;
}
