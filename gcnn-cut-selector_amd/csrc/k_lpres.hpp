// k_lpres.hpp -- the state of an LP that stays on the device across separation rounds (include/gcnn_hip.h: gcnn_lp_rows_build,
// gcnn_lp_round).  Of everything get_state derives from the LP rows only two numbers per row depend on the solve (is_tight, dual);
// the rest -- rhs / norm, the objective cosine, the whole constraint edge list -- is built once per row set and kept.
//   the rebuild (open, append; not the hot path): k_lp_stats' and k_lp_emit's row halves through their own bodies (lp_stats_body,
//     lp_emit_body with LpEmitMore: k_lpstate.hpp), so values and places are theirs bit for bit.  Beside the state's constraint half
//     they record per LP row its two state places (row_place) and the dual's divisor norm * obj_norm (row_scale).
//   a round, two launches, no pass over a row entry:
//     k_lpr_stats  column blocks and cut blocks: lp_stats_body on the round's arrays (an optional column array the round carries is
//                  also copied into its resident buffer, one it does not carry is read from there); row blocks: per LP row is_tight
//                  and dual into cons_feats at row_place.  All blocks first clear the cut set's offsets and columns, so that
//                  whatever a flagged round leaves unwritten still points inside the tables.
//     k_lpr_emit   lp_emit_body's cut half and its flag block, plus the cut edges' by-cut offsets (the forward pass runs without a
//                  graph plan here).
// Every store is bounds-checked against the sizes the host computed; no float atomics.
#pragma once

struct LprArgs {
    // a round: where a present optional column array goes (null: the round does not carry it), and the rows' solve-dependent half
    const double* up[4]; double* keep[4];          // col_lb, col_ub, col_primal, col_primal_avg: upload slot -> resident buffer
    const double* row_dual; const signed char* row_basis;
    const int* row_place; const double* row_scale; // [R][2], [R]
    float* cons_feats; int R, C, nrc;
    int first_row_block;                           // = the column and cut blocks in front
    int* clear[3]; int clear_words[3];             // cut l_ptr, the cut edges' columns, the forward's 16 flag bytes
};

__global__ __launch_bounds__(LP_NT) void k_lpr_rows_stats(LpArgs a) { lp_stats_body(a, blockIdx.x); }
__global__ __launch_bounds__(LP_NT) void k_lpr_rows_emit(LpArgs a, LpEmitMore more) { lp_emit_body(a, blockIdx.x, more); }

// one block's share (block `blk` of `nblk`): the solo launch runs it with (blockIdx.x, gridDim.x), a launch of several sessions'
// rounds (k_lprounds.hpp) with the member's solo pair, so that the clearing loops stride as the solo grid does
__device__ __forceinline__ void lpr_stats_body(const LpArgs& a, const LprArgs& x, const int blk, const int nblk) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 3; ++q)
        for (int i = blk * LP_NT + t; i < x.clear_words[q]; i += nblk * LP_NT) x.clear[q][i] = 0;
    if (blk < x.first_row_block) {
        if (blk < a.ncc) {
            const int j = blk * LP_NT + t;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x.up[q] && j < a.V) x.keep[q][j] = x.up[q][j];
        }
        lp_stats_body(a, blk);
        return;
    }
    const int r = (blk - x.first_row_block) * LP_NT + t;
    if (blk - x.first_row_block >= x.nrc || r >= x.R) return;
    const double dual = x.row_dual[r] / x.row_scale[r];
    const int bs = x.row_basis[r];
    const int pl = x.row_place[2 * (size_t)r], pr = x.row_place[2 * (size_t)r + 1];
    if (lp_in(pl, x.C)) { float* f = x.cons_feats + 4 * (size_t)pl; f[1] = bs == 0; f[3] = (float)(-dual); }
    if (lp_in(pr, x.C)) { float* f = x.cons_feats + 4 * (size_t)pr; f[1] = bs == 2; f[3] = (float)dual; }
}
__global__ __launch_bounds__(LP_NT) void k_lpr_stats(LpArgs a, LprArgs x) { lpr_stats_body(a, x, blockIdx.x, gridDim.x); }

__global__ __launch_bounds__(LP_NT) void k_lpr_emit(LpArgs a, LpEmitMore more) { lp_emit_body(a, blockIdx.x, more); }
