// k_mbatch.hpp -- device side of gcnn_infer_models: host states of SEVERAL models in one call (gcnn_mbatch.hpp).  The states lie
// stacked as gcnn_infer_batch stacks them; a model's states are contiguous, and each model's forward pass runs on its own
// sub-union, so every id the forward reads is written RELATIVE TO THE STATE'S MODEL.
//
//   k_mb_unpack  k_ib_unpack's duties (k_ibatch.hpp) over all states: range and order checks per state, bad ids confined to the
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

// the model words behind the union's table: [0] n_models, [1 + m] the first state of model m (entry n_models: n_states),
// [MB_HEAD + s] the model of state s
#define MB_HEAD 16
#define MB_TABLE_WORDS (IB_COLS * IB_TS + MB_HEAD + IB_MAX_STATES)

struct MbArgs {
    IbArgs ib;      // table: MB_TABLE_WORDS words; l_ptr: [C + n_models], [K + n_models]; everything else as k_ib_unpack takes it
    int* key;       // [E1] union variable ids of the constraint edges (keys of the by-variable sort)
    int* sel_ptr;   // [K+1] cut-row offsets over the whole union, zero on entry; null unless the call selects
};

__global__ __launch_bounds__(256) void k_mb_unpack(MbArgs g) {
    __shared__ int tab[IB_COLS][IB_TS];
    __shared__ int mod[MB_HEAD + IB_MAX_STATES];
    const IbArgs& a = g.ib;
    const int S = a.n_states;
    for (int i = threadIdx.x; i < IB_COLS * IB_TS; i += 256) tab[i / IB_TS][i % IB_TS] = (i % IB_TS) <= S ? a.table[i] : 0;
    for (int i = threadIdx.x; i < MB_HEAD + IB_MAX_STATES; i += 256)
        mod[i] = (i < MB_HEAD || i - MB_HEAD < S) ? a.table[IB_COLS * IB_TS + i] : 0;
    __syncthreads();
    const long long n1 = (long long)tab[IB_E1][S] + S, n2 = (long long)tab[IB_E2][S] + S, nf = tab[IB_FE][S];
    const long long total = n1 + n2 + nf;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
        if (it >= n1 + n2) {   // a forced entry
            const int i = (int)(it - n1 - n2);
            int s = 0, hi = S;
            while (hi - s > 1) { const int mid = (s + hi) >> 1; if (tab[IB_FE][mid] <= i) s = mid; else hi = mid; }
            const int c = a.f_col_in[i], nv = tab[IB_V][s + 1] - tab[IB_V][s];
            a.f_col[i] = (c >= 0 && c < nv) ? c + tab[IB_V][s] - tab[IB_V][mod[1 + mod[MB_HEAD + s]]] : -1;
            continue;
        }
        const int set = it >= n1;
        const int item = (int)(set ? it - n1 : it);
        const int* eoff = tab[set ? IB_E2 : IB_E1];
        int s = 0, hi = S;   // state s owns the items [eoff[s] + s, eoff[s+1] + s + 1): its edges and one closing position
        while (hi - s > 1) { const int mid = (s + hi) >> 1; if (eoff[mid] + mid <= item) s = mid; else hi = mid; }
        const int m = mod[MB_HEAD + s], f = mod[1 + m];   // the state's model and that model's first state
        const int e0 = eoff[s], E = eoff[s + 1] - e0, j = item - e0 - s;
        const int er = e0 - eoff[f];                      // the state's first edge within its model
        const int* loff = tab[set ? IB_K : IB_C];
        const int l0 = loff[s], n_left = loff[s + 1] - l0, lr = l0 - loff[f];
        const int v0 = tab[IB_V][s], nv = tab[IB_V][s + 1] - v0, vr = v0 - tab[IB_V][f];
        const int* src = a.packed[set] + 2 * (size_t)e0;
        int* l_ptr = a.l_ptr[set] + l0 + m;               // the state's rows in its model's array
        int* sel = (set && g.sel_ptr) ? g.sel_ptr + l0 : nullptr;
        if (j == 0) {   // the state's first row starts at its first edge, whatever the list says
            l_ptr[0] = er;
            if (sel) sel[0] = e0;
        }
        // by-left offsets: ptr[k] = first position whose row id >= k, ids clamped; rows 1 .. n_left-1 only (row 0 above, the end of
        // the last row is the next state's row 0 or the model's closing entry)
        const int lo = j == 0 ? -1 : min(max(src[j - 1], -1), n_left);
        const int hb = j == E ? n_left : min(max(src[j], -1), n_left);
        for (int k = max(lo + 1, 1); k <= min(hb, n_left - 1); ++k) {
            l_ptr[k] = er + j;
            if (sel) sel[k] = e0 + j;
        }
        if (j < E) {
            const int l = src[j], v = src[E + j];
            const bool bad_l = l < 0 || l >= n_left, bad_v = v < 0 || v >= nv;
            if (bad_l | bad_v) atomicOr(&a.flags[4 * s], 1);
            if (j + 1 < E && src[j + 1] < l) atomicOr(&a.flags[4 * s + 1 + set], 1);
            a.var[set][e0 + j] = vr + (bad_v ? 0 : v);
            if (set == 0) {
                a.left[e0 + j] = lr + min(max(l, 0), max(n_left - 1, 0));
                a.iota[e0 + j] = e0 + j;
                g.key[e0 + j] = v0 + (bad_v ? 0 : v);
            }
        }
    }
    if (blockIdx.x == 0) {
        const int M = mod[0];
        if ((int)threadIdx.x < M) {   // every model's closing entries: its edge count
            const int m = threadIdx.x, f = mod[1 + m], fn = mod[2 + m];
            a.l_ptr[0][tab[IB_C][fn] + m] = tab[IB_E1][fn] - tab[IB_E1][f];
            a.l_ptr[1][tab[IB_K][fn] + m] = tab[IB_E2][fn] - tab[IB_E2][f];
        }
        if (threadIdx.x == 0 && g.sel_ptr) g.sel_ptr[tab[IB_K][S]] = tab[IB_E2][S];
    }
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
