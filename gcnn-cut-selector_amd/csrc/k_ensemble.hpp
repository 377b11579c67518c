// k_ensemble.hpp -- device side of the ensemble calls (gcnn_ensemble.hpp): the mean of up to GCNN_GROUP_MAX score rows.
//
//   k_ens_mean   mean[k] = (((row[0][k] + row[1][k]) + ...) + row[M-1][k]) / float(M): the members in the caller's order, every step
//                fp32 and rounded to nearest, nothing contracted (__fadd_rn, __fdiv_rn), so a float32 loop on the host gives the
//                same bits.  M == 1 copies the row (no division: the bits of a NaN stay too).  A NaN in any member gives a NaN.
//                The row pointers travel in the kernel arguments.  Grid-stride, one element per thread and trip; no LDS, no
//                atomics.  wave64.
#pragma once
#include "gcnn_common.hpp"

#define ENS_MAX 8

struct EnsArgs {
    const float* row[ENS_MAX];   // [n] each; entries from n_models on are not read
    float* mean;                 // [n]
    int n_models, n;
};

__global__ __launch_bounds__(256) void k_ens_mean(EnsArgs a) {
    const int M = a.n_models;
    const float div = (float)M;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
        float acc = a.row[0][i];
#pragma unroll
        for (int m = 1; m < ENS_MAX; ++m)
            if (m < M) acc = __fadd_rn(acc, a.row[m][i]);
        a.mean[i] = M == 1 ? acc : __fdiv_rn(acc, div);
    }
}
