// k_ensbatch.hpp -- device side of the many-state ensemble calls (gcnn_ensbatch.hpp): the rank-mode tail of a union in ONE launch.
//
//   k_eb_mean_rank   one block of 256 per state of the union.  For the state's segment [k_off[s], k_off[s+1]) of the M member rows:
//                    the mean in exactly k_ens_mean's arithmetic (k_ensemble.hpp: the members in argument order, __fadd_rn, one
//                    __fdiv_rn by float(M), M == 1 copies the bits, nothing contracted), written to the output block, and the
//                    stable descending ranking of rank_desc_lds (k_infer.hpp: ties in index order, NaN as -inf) of those same
//                    values, written to `order` as state-local cut indices.  The keys of the ranking are the values the block has
//                    just computed: they go from the registers into the LDS the network sorts, and `mean` is never read back.
//                    It stands for k_ens_mean + k_ib_rank, two dependent launches, in a chain that is bound by the number of
//                    dependent launches.  Segments of 0 or more than RK_MAX cuts return without writing (the host never sends
//                    them).  The row pointers and the table pointer travel in the kernel arguments.
// LDS 32 KiB (keys and indices of RK_MAX cuts, static, as k_ib_rank): five blocks per CU, and a call has at most 64.  No atomics,
// no scratch.  wave64.
#pragma once
#include "k_ensemble.hpp"
#include "k_ibatch.hpp"

struct EbArgs {
    const float* row[ENS_MAX];   // [K_total] each; entries from n_models on are not read
    const int* table;            // the union's table: column IB_K holds the states' cut offsets
    float* mean;                 // [K_total]
    int* order;                  // [K_total]
    int n_models;
};

__global__ __launch_bounds__(256) void k_eb_mean_rank(EbArgs a) {
    __shared__ float v[RK_MAX];
    __shared__ int ix[RK_MAX];
    const int k0 = a.table[IB_K * IB_TS + blockIdx.x], n = a.table[IB_K * IB_TS + blockIdx.x + 1] - k0;
    if (n <= 0 || n > RK_MAX) return;      // (uniform over the block: no barrier is skipped by a part of it)
    const int M = a.n_models;
    const float div = (float)M;
    int m = 1;
    while (m < n) m <<= 1;
    for (int i = threadIdx.x; i < m; i += 256) {
        float x = -INFINITY;
        if (i < n) {
            float acc = a.row[0][k0 + i];
#pragma unroll
            for (int r = 1; r < ENS_MAX; ++r)
                if (r < M) acc = __fadd_rn(acc, a.row[r][k0 + i]);
            x = M == 1 ? acc : __fdiv_rn(acc, div);
            a.mean[k0 + i] = x;
        }
        v[i] = x != x ? -INFINITY : x; ix[i] = i < n ? i : 0x7fffffff;
    }
    __syncthreads();
    rank_desc_network<256>(m, v, ix);
    for (int i = threadIdx.x; i < n; i += 256) a.order[k0 + i] = ix[i];
}
