// k_lpedits.hpp -- the removals of several resident LPs in one set of launches (include/gcnn_hip.h: gcnn_lp_rounds_edit; host side in
// gcnn_lpedits.hpp).  The appends and rounds of that call go out through k_lprounds.hpp's twins and k_group.hpp's kernels; these
// are the group twins of the removal's three launches (k_lpremove.hpp).  Each twin has its solo kernel's launch bounds, finds its
// member in the launch's table (group_member) and runs the solo body with that member's arguments and its solo block index: no
// removal launch strides by its grid, so the block index is all a body needs.  A member's bits are therefore its solo call's.
// Nothing here stores on its own: every store is the solo body's, bounds-checked there; integer atomics only; the LDS is the bodies'.
#pragma once

__global__ __launch_bounds__(LP_NT) void k_lpes_mark(const GroupHead* __restrict__ t) {
    int b, nb;
    const LpdArgs& x = group_member<LpdArgs>(t, b, nb);
    lpd_mark_body(x, b);
}
__global__ __launch_bounds__(LP_NT) void k_lpes_rows(const GroupHead* __restrict__ t) {
    int b, nb;
    const LpdArgs& x = group_member<LpdArgs>(t, b, nb);
    lpd_rows_body(x, b);
}
__global__ __launch_bounds__(LP_NT) void k_lpes_vars(const GroupHead* __restrict__ t) {
    int b, nb;
    const LpdArgs& x = group_member<LpdArgs>(t, b, nb);
    lpd_vars_body(x, b);
}
