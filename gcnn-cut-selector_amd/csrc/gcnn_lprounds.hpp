// gcnn_lprounds.hpp -- the twins of the LP launches that a call of several resident LPs records (k_lprounds.hpp): every launch of the
// solo append (lpa_enqueue) and of the solo round (lpr_run, the ranking and the selection behind it) has a group twin that runs the
// solo body with the member's arguments.  Included at the end of gcnn_capi.hip behind gcnn_lpappend.hpp and gcnn_group.hpp; the calls
// themselves (gcnn_lp_rounds, gcnn_lp_rounds_edit) share one body in gcnn_lpedits.hpp.  Kept apart so that its launch names form their
// own inventory (tests/test_lprounds_build.py).
#include "k_lprounds.hpp"

static_assert(GCNN_LP_ROUNDS_MAX == GCNN_GROUP_MAX, "include/gcnn_hip.h");
static_assert(sizeof(GPair<LpArgs, LpaArgs>) <= GROUP_REC_BYTES && sizeof(GPair<LpArgs, LprArgs>) <= GROUP_REC_BYTES &&
              sizeof(GPair<LpArgs, LpEmitMore>) <= GROUP_REC_BYTES && sizeof(SelArgs) <= GROUP_REC_BYTES, "k_group.hpp: GROUP_REC_BYTES");

#define LPRS_APPEND_STAGES 4      // launches of one member's append
#define LPRS_STAGES (GCNN_GROUP_MAX_STAGES + LPRS_APPEND_STAGES)

// the LP launches a member's call records, and their twins; every other kernel is the forward pass's (g_group_kernels)
static GroupKernel g_lprounds_kernels[] = {
    {(const void*)k_lpa_stats, (const void*)k_lprs_append_stats, "k_lprs_append_stats", {}},
    {(const void*)k_lpa_scan, (const void*)k_lprs_append_scan, "k_lprs_append_scan", {}},
    {(const void*)k_lpa_move, (const void*)k_lprs_append_move, "k_lprs_append_move", {}},
    {(const void*)k_lpa_order, (const void*)k_lprs_append_order, "k_lprs_append_order", {}},
    {(const void*)k_lpr_stats, (const void*)k_lprs_round_stats, "k_lprs_round_stats", {}},
    {(const void*)k_lpr_emit, (const void*)k_lprs_round_emit, "k_lprs_round_emit", {}},
    {(const void*)k_rank_scores, (const void*)k_lprs_rank_scores, "k_lprs_rank_scores", {}},
    {(const void*)k_sel_pairs, (const void*)k_lprs_sel_pairs, "k_lprs_sel_pairs", {}},
    {(const void*)k_sel_filter, (const void*)k_lprs_sel_filter, "k_lprs_sel_filter", {}},
};
static GroupKernel* lprounds_kernel(const void* solo) {
    for (GroupKernel& g : g_lprounds_kernels) if (g.solo == solo) return &g;
    return group_kernel(solo);
}
