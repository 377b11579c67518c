// gcnn_common.hpp -- shared definitions: parameter layout, MFMA wrappers, small device helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/gcnn_hip.h"

#define EMB 64
#define LDW 68  // padded LDS row stride in floats: 272 B keeps 16-B alignment, b128 row reads conflict-free

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------
// parameter layout (checkpoint order, model.py:53-56/215; shapes model.py:174-208, 486-508)
// ---------------------------------------------------------------------------------------------------------------
struct PInfo { int off, rows, cols, trainable; };
static PInfo g_pinfo[GCNN_N_PARAMS];
static int g_ptotal = 0;

enum {  // indices into the 62-array list
    P_CONS = 0, P_CONS_EDGE = 6, P_VAR = 8, P_CUT = 14, P_CUT_EDGE = 20, P_CONV0 = 22, P_CONV1 = 34, P_CONV2 = 46,
    P_OUT = 58
};
enum { E_SHIFT = 0, E_SCALE = 1, E_W1 = 2, E_B1 = 3, E_W2 = 4, E_B2 = 5 };  // embedding block
enum { C_WL = 0, C_BL = 1, C_WE = 2, C_WR = 3, C_S1 = 4, C_WF = 5, C_BF = 6, C_S2 = 7, C_W1 = 8, C_B1 = 9, C_W2 = 10,
       C_B2 = 11 };  // conv block

static void layout_init() {
    if (g_ptotal) return;
    int n = 0, off = 0;
    auto add = [&](int rows, int cols, int tr) {
        g_pinfo[n].off = off; g_pinfo[n].rows = rows; g_pinfo[n].cols = cols; g_pinfo[n].trainable = tr;
        off += (rows * cols + 3) & ~3; ++n;
    };
    auto emb = [&](int f) { add(1, f, 0); add(1, f, 0); add(f, EMB, 1); add(1, EMB, 1); add(EMB, EMB, 1); add(1, EMB, 1); };
    auto conv = [&]() {
        add(EMB, EMB, 1); add(1, EMB, 1); add(1, EMB, 1); add(EMB, EMB, 1); add(1, 1, 0); add(EMB, EMB, 1); add(1, EMB, 1);
        add(1, 1, 0); add(2 * EMB, EMB, 1); add(1, EMB, 1); add(EMB, EMB, 1); add(1, EMB, 1);
    };
    emb(4); add(1, 1, 0); add(1, 1, 0); emb(14); emb(6); add(1, 1, 0); add(1, 1, 0);
    conv(); conv(); conv();
    add(EMB, EMB, 1); add(1, EMB, 1); add(EMB, 1, 1); add(1, 1, 1);
    g_ptotal = off;
}
static inline int poff(int i) { return g_pinfo[i].off; }

// ---------------------------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Blocks b and b+8 share an XCD (round-robin dispatch).  Give every XCD a contiguous range of work items so the
// rows a range gathers stay in that XCD's 4 MiB L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7, i = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ---------------------------------------------------------------------------------------------------------------
// Store policy of result tensors: "store 16 bytes of a result", stated once.
//   ST_PLAIN: an ordinary float4 store.  The line stays dirty in the XCD's L2 until the end-of-kernel release writes it back --
//             serially, after the last wave, with nothing running under it (B / 6 TB/s behind B dirty bytes).
//   ST_WT   : the same 16 bytes as ONE vector store carrying sc1 (write-through): the line leaves L2 while the stores' wave goes on
//             computing, so only what the last stage of a program stored is still on its way when the launch ends.  The address is
//             the full 64-bit pointer (global_store, not a buffer descriptor, whose 32-bit byte offset would reach exactly 4 GiB at
//             the library's 2^24-row limit and drop the last piece silently): it writes what the plain store writes, at any size.
//             The trailing s_nop keeps the data registers intact until the store has read them.
// The policy is a template argument of the row programs, chosen per launch, never globally.  Written ST_WT (tensors of many bytes, 16
// bytes per lane, read by a LATER launch only): rt_store in the programs of k_embed_fwd_wt, k_conv_fwd_wt, k_conv_bwd_wt and
// k_tail_bwd_wt (k_rows.hpp), which the launchers take for row sets of at most GCNN_WT_MAX_ROWS rows (below).
// Left ST_PLAIN on purpose:
//   * anything narrower than 16 bytes per lane -- rt_mask_store's mask16 patterns, scores, the loss head's lane-0 scalars: a short
//     sc1 store is one fabric write each, 6-12x the time per byte;
//   * loss_head_tile's per-tile dws partial (one float4 from 16 of a tile's 64 lanes: 256 B per tile, nothing to hide);
//   * what a block of the SAME launch reads back: the copies fuse_weights leaves behind M | u for fold_block, and the Adam
//     update inside k_reduce (params, m, v are read-modify-write in place);
//   * the edge passes' S / N / dP_send rows (k_edge.hpp) and k_wgrad's partial slabs: see profiles/README.md;
//   * the turnaround launch of the cut rows (k_conv_turn, k_conv_turn_split): 9.12 -> 9.06 us with write-through, inside its spread;
//   * the four-waves-per-tile programs (k_rows_split.hpp), the grouped launches (k_group.hpp), the PreNorm forms (KEEP_A) and the
//     inference kernels (k_infer.hpp, k_ibatch.hpp): at most 256 tiles, or not measured with write-through.
// -DGCNN_STORE_PLAIN makes every ST_WT site plain (the A side of an A/B: tools/mklib.sh base -DGCNN_STORE_PLAIN).
// ---------------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
enum { ST_PLAIN = 0, ST_WT = 1 };
template <int POLICY>
__device__ __forceinline__ void store16(float* p, float x, float y, float z, float w) {
#ifdef GCNN_STORE_PLAIN
    constexpr bool WT = false;
#else
    constexpr bool WT = POLICY == ST_WT;
#endif
    if (WT) {
        const f32x4 v = {x, y, z, w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
    } else {
        *(float4*)p = make_float4(x, y, z, w);
    }
}
// Write-through pays while a launch is ONE resident round with about a tile per wave (setcov x 32, combauc x 32): what plain stores leave
// dirty is then written back after the last wave.  Large row sets lose with it -- a wave's earlier tiles are written back under its
// later ones anyway, every write-through store is waited for ahead of the next tile's operands, and the next launch finds none of
// the rows in L2 (always on: capfac x 32 +5.9 %, indset x 64 +4.5 %, setcov x 128 +2.3 % per step; profiles/README.md).  So the
// launchers take the write-through kernel of a launch only while its largest row set has at most GCNN_WT_MAX_ROWS rows: one 16-row
// tile for each of the 8 waves of one block per CU (256 CUs).  The choice is the launcher's, at compile time inside the kernel: the
// same condition tested per store inside ONE kernel cost 1 % per step with the plain side taken (both store forms in every epilogue).
#ifndef GCNN_WT_MAX_ROWS
#define GCNN_WT_MAX_ROWS (256 * 8 * 16)
#endif
// The two other 16-byte-per-lane writers of the training step, each measured on its own and left plain (profiles/README.md):
// the S / N / dP_send rows of the edge passes' main loops (k_edge.hpp) and k_wgrad's partial slabs.  -DGCNN_ST_EDGE=ST_WT /
// -DGCNN_ST_WGRAD=ST_WT rebuild an experiment library with either side written through.
#ifndef GCNN_ST_EDGE
#define GCNN_ST_EDGE ST_PLAIN
#endif
#ifndef GCNN_ST_WGRAD
#define GCNN_ST_WGRAD ST_PLAIN
#endif

// joint pre-activation of one edge, in the reference's association order: (left + coef*w) + right, model.py:564-565
__device__ __forceinline__ float jointf(float pl, float cw, float pr) { return __fadd_rn(__fadd_rn(pl, cw), pr); }

