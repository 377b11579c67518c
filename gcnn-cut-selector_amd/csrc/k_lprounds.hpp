// k_lprounds.hpp -- the rounds of several resident LPs in one set of launches (include/gcnn_hip.h: gcnn_lp_rounds; host side in
// gcnn_lprounds.hpp).  The forward passes go out through k_group.hpp's kernels; these are the group twins of the launches around
// them -- the round's two state launches (k_lpres.hpp), the append's four (k_lpappend.hpp) and the ranking / selection tail
// (k_infer.hpp, k_select.hpp).  Each twin has its solo kernel's launch bounds, finds its member in the launch's table (group_member:
// a prefix of block counts read through the constant address space, so the member's arguments land in scalar registers as kernel
// arguments do) and runs the solo body with that member's arguments and its solo (block, blocks) pair: k_lpr_stats' clearing loops
// and k_sel_pairs' pivot loop stride by the member's solo grid, not by the launch's.  A member's bits are therefore its solo call's.
// Nothing here stores on its own: every store is the solo body's, bounds-checked there; no float atomics; the LDS is the bodies'.
#pragma once

__global__ __launch_bounds__(LP_NT) void k_lprs_round_stats(const GroupHead* __restrict__ t) {
    int b, nb;
    const GPair<LpArgs, LprArgs>& p = group_member<GPair<LpArgs, LprArgs>>(t, b, nb);
    lpr_stats_body(p.a, p.b, b, nb);
}
__global__ __launch_bounds__(LP_NT) void k_lprs_round_emit(const GroupHead* __restrict__ t) {
    int b, nb;
    const GPair<LpArgs, LpEmitMore>& p = group_member<GPair<LpArgs, LpEmitMore>>(t, b, nb);
    lp_emit_body(p.a, b, p.b);
}
__global__ __launch_bounds__(LP_NT) void k_lprs_append_stats(const GroupHead* __restrict__ t) {
    int b, nb;
    const GPair<LpArgs, LpaArgs>& p = group_member<GPair<LpArgs, LpaArgs>>(t, b, nb);
    lpa_stats_body(p.a, p.b, b);
}
__global__ __launch_bounds__(LP_NT) void k_lprs_append_scan(const GroupHead* __restrict__ t) {
    int b, nb;
    const LpaArgs& x = group_member<LpaArgs>(t, b, nb);
    lpa_scan_body(x, b);
}
__global__ __launch_bounds__(LP_NT) void k_lprs_append_move(const GroupHead* __restrict__ t) {
    int b, nb;
    const GPair<LpArgs, LpaArgs>& p = group_member<GPair<LpArgs, LpaArgs>>(t, b, nb);
    lpa_move_body(p.a, p.b, b);
}
__global__ __launch_bounds__(LP_NT) void k_lprs_append_order(const GroupHead* __restrict__ t) {
    int b, nb;
    const LpaArgs& x = group_member<LpaArgs>(t, b, nb);
    lpa_order_body(x, b);
}
// the tail: a member is one sample of its own SelArgs (cut column ids are member-local, pairs never cross a member)
__global__ __launch_bounds__(SEL_NT) void k_lprs_sel_pairs(const GroupHead* __restrict__ t) {
    int b, nb;
    const SelArgs& a = group_member<SelArgs>(t, b, nb);
    sel_pairs_body(a, b, nb);
}
__global__ __launch_bounds__(SEL_NT) void k_lprs_sel_filter(const GroupHead* __restrict__ t) {
    int b, nb;
    const SelArgs& a = group_member<SelArgs>(t, b, nb);
    sel_filter_body<float>(a, a.q, b, true);
}
typedef GTriple<const float*, int, int*> RankScoresArgs;
__global__ __launch_bounds__(256) void k_lprs_rank_scores(const GroupHead* __restrict__ t) {   // k_rank_scores: one block a member
    __shared__ float v[4096];
    __shared__ int ix[4096];
    int b, nb;
    const RankScoresArgs& a = group_member<RankScoresArgs>(t, b, nb);
    rank_desc_lds<256>(a.a, a.b, v, ix);
    for (int i = threadIdx.x; i < a.b; i += 256) a.c[i] = ix[i];
}
