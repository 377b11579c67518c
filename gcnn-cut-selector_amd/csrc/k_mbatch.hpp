// k_mbatch.hpp -- device side of gcnn_infer_models: host states of SEVERAL models in one call (gcnn_mbatch.hpp).  The states lie
// stacked as gcnn_infer_batch stacks them; a model's states are contiguous, and each model's forward pass runs on its own
// sub-union, so every id the forward reads is written RELATIVE TO THE STATE'S MODEL.
//
//   k_mb_unpack  k_ib_unpack's duties over all states, by the same body (ib_unpack_body<true>, k_ibatch.hpp; the model words of
//                the table are defined there too): range and order checks per state, bad ids confined to the
//                state's own ranges, by-left offsets by boundary detection inside the state, four flags per state, forced columns
//                shifted.  Row ids, variable ids and edge offsets restart at each model's first state; the arrays stay at the
//                union's positions.  Each model's by-left offsets get their own closing entry: model m's array starts at the
//                union row of its first state + m.  The GLOBAL variable id is written as the sort key of the by-variable stage,
//                and in selection mode the cut rows' offsets once more over the whole union (what k_sel_pairs indexes).
//   k_mb_vptr    the by-variable offsets of the whole union (k_seg_offsets on the global key) -> one array per model: V_m + 1
//                entries rebased to the model's first edge, model m's array at the union variable of its first state + m.
// Models are contiguous in the key space and the sort is stable, so a model's sorted segment is that model's own stable order.
// Integer atomics only (the flags).  wave64.
#pragma once
#include "k_ibatch.hpp"

struct MbArgs {
    IbArgs ib;      // table: MB_TABLE_WORDS words; l_ptr: [C + n_models], [K + n_models]; everything else as k_ib_unpack takes it
    int* key;       // [E1] union variable ids of the constraint edges (keys of the by-variable sort)
    int* sel_ptr;   // [K+1] cut-row offsets over the whole union, zero on entry; null unless the call selects
};

__global__ __launch_bounds__(256) void k_mb_unpack(MbArgs g) {
    __shared__ int tab[IB_COLS][IB_TS];
    __shared__ int mod[MB_HEAD + IB_MAX_STATES];
    ib_unpack_body<true>(g.ib, tab, mod, g.key, g.sel_ptr);
}

// gptr: [V+1] offsets of the union's sorted list by global variable; vptr: [V + n_models]
__global__ __launch_bounds__(256) void k_mb_vptr(const int* __restrict__ table, const int* __restrict__ gptr, int* __restrict__ vptr) {
    __shared__ int v0[GCNN_GROUP_MAX + 1], e0[GCNN_GROUP_MAX + 1];
    const int* mod = table + IB_COLS * IB_TS;
    const int M = mod[0];
    if ((int)threadIdx.x <= M) {
        const int f = mod[1 + threadIdx.x];
        v0[threadIdx.x] = table[IB_V * IB_TS + f]; e0[threadIdx.x] = table[IB_E1 * IB_TS + f];
    }
    __syncthreads();
    const int total = v0[M] + M;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        int m = 0;
        for (int i = 1; i < M; ++i) m += t >= v0[i] + i;   // model m owns the entries [v0[m] + m, v0[m+1] + m + 1)
        vptr[t] = gptr[t - m] - e0[m];
    }
}
