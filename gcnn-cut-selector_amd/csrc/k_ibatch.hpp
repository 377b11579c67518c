// k_ibatch.hpp -- device side of gcnn_infer_batch: many host states scored as ONE disjoint union (gcnn_ibatch.hpp).
//
//   k_ib_unpack  one pass over every uploaded index.  The states arrive with STATE-LOCAL ids, each edge list packed as its own
//                [2,E_s] block (what gcnn_host_pack_edges writes).  Per state: range check against that state's sizes, order check,
//                bad ids replaced (variable -> the state's variable 0, row -> clamped into the state's rows), ids shifted by the
//                state's offsets in the union and written to the union's lists, by-left offsets of both edge sets by boundary
//                detection INSIDE the state -- the entry a state shares with its neighbour (its first row's start) is written
//                from the table, not from the data, so a state with bad or unsorted ids cannot move a neighbour's segment.
//                Forced rows' columns are shifted the same way (a bad column becomes -1: it takes no part, gcnn_select_cuts).
//                Four flags per state, with the meaning of gcnn_infer's.  Its body (ib_unpack_body) is also k_mb_unpack's, which
//                writes every id relative to the state's model (k_mbatch.hpp).
//   k_ib_rank    one block per state: the stable descending ranking of its own score segment (rank_desc_lds, k_infer.hpp).
// Integer atomics only (the flags).  wave64.
#pragma once
#include "k_misc.hpp"
#include "k_infer.hpp"

#define IB_MAX_STATES 64
#define IB_TS 72   // table stride: IB_MAX_STATES + 1 offsets per column, padded to a multiple of 4 (16-byte columns)
enum { IB_C = 0, IB_V, IB_K, IB_E1, IB_E2, IB_F, IB_FE, IB_COLS };

struct IbArgs {
    const int* table;          // [IB_COLS][IB_TS] offsets of every state in the union (entry n_states = the total)
    int n_states;
    const int* packed[2];      // per edge set: the states' [2,E_s] blocks, state s at 2 * e_off[s]
    int* left;                 // [E1] union row ids of the constraint edges (what the by-variable order gathers)
    int* var[2];               // [E1], [E2] union variable ids = the by-left lists' `oth`
    int* l_ptr[2];             // [C+1], [K+1] zero on entry
    int* iota;                 // [E1] input positions (values of the by-variable sort)
    int* flags;                // [n_states][4] zero on entry
    const int* f_col_in; int* f_col;   // [FE] forced columns, state-local -> union
};

// the model words behind the table of a union whose states belong to several models (gcnn_infer_models, k_mbatch.hpp):
// [0] n_models, [1 + m] the first state of model m (entry n_models: n_states), [MB_HEAD + s] the model of state s
#define MB_HEAD 16
#define MB_TABLE_WORDS (IB_COLS * IB_TS + MB_HEAD + IB_MAX_STATES)

// The index pass of both unions.  MODELS = false: k_ib_unpack, one model whose first state is 0 -- `mod`, `key` and `sel_ptr` are
// not touched.  MODELS = true: k_mb_unpack (k_mbatch.hpp) -- row ids, variable ids and edge offsets restart at the first state of
// the state's model, model m's by-left array starts at the union row of its first state + m and closes with an entry of its own,
// the union's variable id is written as `key`, and where `sel_ptr` is given the cut rows' offsets once more over the whole union.
template <bool MODELS>
__device__ __forceinline__ void ib_unpack_body(const IbArgs& a, int (*tab)[IB_TS], int* mod, int* key, int* sel_ptr) {
    const int S = a.n_states;
    for (int i = threadIdx.x; i < IB_COLS * IB_TS; i += 256) tab[i / IB_TS][i % IB_TS] = (i % IB_TS) <= S ? a.table[i] : 0;
    if constexpr (MODELS)
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
            int vr = tab[IB_V][s];
            if constexpr (MODELS) vr -= tab[IB_V][mod[1 + mod[MB_HEAD + s]]];
            a.f_col[i] = (c >= 0 && c < nv) ? c + vr : -1;
            continue;
        }
        const int set = it >= n1;
        const int item = (int)(set ? it - n1 : it);
        const int* eoff = tab[set ? IB_E2 : IB_E1];
        int s = 0, hi = S;   // state s owns the items [eoff[s] + s, eoff[s+1] + s + 1): its edges and one closing position
        while (hi - s > 1) { const int mid = (s + hi) >> 1; if (eoff[mid] + mid <= item) s = mid; else hi = mid; }
        const int e0 = eoff[s], E = eoff[s + 1] - e0, j = item - e0 - s;
        const int* loff = tab[set ? IB_K : IB_C];
        const int l0 = loff[s], n_left = loff[s + 1] - l0;
        const int v0 = tab[IB_V][s], nv = tab[IB_V][s + 1] - v0;
        int m = 0, er = e0, lr = l0, vr = v0;   // the state's model; its first edge, row and variable within that model
        if constexpr (MODELS) {
            m = mod[MB_HEAD + s];
            const int f = mod[1 + m];           // that model's first state
            er -= eoff[f]; lr -= loff[f]; vr -= tab[IB_V][f];
        }
        const int* src = a.packed[set] + 2 * (size_t)e0;
        int* l_ptr = a.l_ptr[set] + l0 + m;     // the state's rows in its model's array
        int* sel = nullptr;
        if constexpr (MODELS) sel = (set && sel_ptr) ? sel_ptr + l0 : nullptr;
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
                if constexpr (MODELS) key[e0 + j] = v0 + (bad_v ? 0 : v);
            }
        }
    }
    if (blockIdx.x == 0) {
        int M = 1;
        if constexpr (MODELS) M = mod[0];
        if ((int)threadIdx.x < M) {   // every model's closing entries: its edge count
            const int m = threadIdx.x;
            int fn = S, e1 = 0, e2 = 0;
            if constexpr (MODELS) { fn = mod[2 + m]; e1 = tab[IB_E1][mod[1 + m]]; e2 = tab[IB_E2][mod[1 + m]]; }
            a.l_ptr[0][tab[IB_C][fn] + m] = tab[IB_E1][fn] - e1;
            a.l_ptr[1][tab[IB_K][fn] + m] = tab[IB_E2][fn] - e2;
        }
        if constexpr (MODELS)
            if (threadIdx.x == 0 && sel_ptr) sel_ptr[tab[IB_K][S]] = tab[IB_E2][S];
    }
}

__global__ __launch_bounds__(256) void k_ib_unpack(IbArgs a) {
    __shared__ int tab[IB_COLS][IB_TS];
    ib_unpack_body<false>(a, tab, nullptr, nullptr, nullptr);
}

// One block per state; states without cuts or with more than RK_MAX cuts are left alone (the host ranks those itself).
__global__ __launch_bounds__(256) void k_ib_rank(const float* __restrict__ scores, const int* __restrict__ table, int* __restrict__ order) {
    __shared__ float v[RK_MAX];
    __shared__ int ix[RK_MAX];
    const int k0 = table[IB_K * IB_TS + blockIdx.x], n = table[IB_K * IB_TS + blockIdx.x + 1] - k0;
    if (n <= 0 || n > RK_MAX) return;
    rank_desc_lds<256>(scores + k0, n, v, ix);
    for (int i = threadIdx.x; i < n; i += 256) order[k0 + i] = ix[i];
}
