// k_rank.hpp -- the test stage's rankings (model_tester.py:113-153, 205-224) on the device: for every sample of a test set, the
// first position at which each of several candidate rankings deviates from a truth ranking.  One 256-thread block per sample.
//
// Every ranking is the stable descending order of Python's sorted(range(n), key=..., reverse=True): larger key first, equal keys in
// index order, NaN ranked as -inf (the order of k_ranking / rank_desc_lds).  Candidates of one launch, rows of `dev`:
//   0 .. n_scores-1   model scores [n_scores][K_total] fp32            against truth32 (what load_batch_tf feeds the model)
//   n_scores          hybrid quality [K_total] fp64 (when given)       against truth64 (the file's improvements)
//   then n_perms      permutations [n_perms][K_total] int32, perm[r] = the cut at rank r, sample-local   against truth64
// The two truths rank differently when two improvements tie in fp32 but not in fp64: each key is compared in its own type.
// dev[row][s] = the first deviating position, n when the rankings agree, 0 for a sample without cuts, -1 for more than RM_MAX_CUTS.
//
//   n <= 256       rank by counting: thread i counts the entries ranked before its own in every keyed list (LDS copies).  Position
//                  r of a candidate and the truth differ first at min{ rank_c(i) : rank_c(i) != rank_t(i) } (for r below that
//                  minimum the candidate's entry at r has truth rank r).  A permutation deviates at r when rank_t64[perm[r]] != r.
//                  Each truth is ranked once per sample.
//   257 .. 4096    the bitonic network of rank_desc_lds: both truth orders are kept in LDS (16-bit), then the candidates are
//                  sorted one at a time into the same key buffer and compared position by position.
// LDS 64 KiB + a few words: two blocks per CU.  The LDS is static and sized for the sorting path, so the usual sample of a few
// dozen cuts, whose counting path uses about 13 KiB, also runs at two blocks (8 waves) per CU.  A whole test set of 2,000 setcov
// samples takes ~0.17 ms (profiles/test_models.txt); should the launch ever show, split the counting path into a kernel of its
// own with a small LDS footprint (two launches) or size the LDS dynamically from the largest sample.
#pragma once

#define RM_MAX_CUTS 4096   // RK_MAX
#define RM_MAX_SETS 8      // model score rows and permutation rows per launch, each (GCNN_GROUP_MAX)
#define RM_NT 256

struct RankMultiArgs {
    const int* offsets;     // [n_samples+1] first cut of every sample; offsets[n_samples] = K_total, the row stride
    int n_samples;
    const float* truth32;   // [K_total], read when n_scores > 0
    const double* truth64;  // [K_total], read when hybrid or n_perms > 0
    const float* scores;    // [n_scores][K_total]
    int n_scores;
    const double* hybrid;   // [K_total] or null
    const int* perms;       // [n_perms][K_total]
    int n_perms;
    int* dev;               // [n_scores + (hybrid != null) + n_perms][n_samples]
};

__device__ __forceinline__ float rm_key(float x) { return x != x ? -INFINITY : x; }
__device__ __forceinline__ double rm_key(double x) { return x != x ? (double)-INFINITY : x; }

// position of entry i in the stable descending order of v[0..n)
template <typename T>
__device__ __forceinline__ int rm_rank(const T* v, int n, T x, int i) {
    int r = 0;
    for (int j = 0; j < n; ++j) r += v[j] > x || (v[j] == x && j < i);
    return r;
}

__global__ __launch_bounds__(RM_NT) void k_rank_multi(RankMultiArgs a) {
    __shared__ double kv[RM_MAX_CUTS];       // keys: every keyed list (n <= 256), or the list being sorted
    __shared__ int ix[RM_MAX_CUTS];          // truth64 ranks (n <= 256), or the sorted indices
    __shared__ short ord[2][RM_MAX_CUTS];    // truth32 / truth64 orders (n > 256)
    __shared__ int first[2 * RM_MAX_SETS + 1];
    const int s = blockIdx.x, beg = a.offsets[s], n = a.offsets[s + 1] - beg;
    const size_t K = (size_t)a.offsets[a.n_samples];
    const int hyb = a.hybrid ? 1 : 0, rows = a.n_scores + hyb + a.n_perms, row_p = a.n_scores + hyb;
    const bool t64 = a.hybrid || a.n_perms > 0;
    if (n <= 0 || n > RM_MAX_CUTS) {
        for (int r = threadIdx.x; r < rows; r += RM_NT) a.dev[(size_t)r * a.n_samples + s] = n <= 0 ? 0 : -1;
        return;
    }
    for (int r = threadIdx.x; r < rows; r += RM_NT) first[r] = n;
    if (n <= RM_NT) {
        double* k64 = kv;                      // [256] truth64
        double* khy = kv + RM_NT;              // [256] hybrid
        float* k32 = (float*)(kv + 2 * RM_NT); // [256] truth32, then [n_scores][256] scores
        const int i = threadIdx.x;
        const bool in = i < n;
        if (in) {
            if (a.n_scores) k32[i] = rm_key(a.truth32[beg + i]);
            if (t64) k64[i] = rm_key(a.truth64[beg + i]);
            if (hyb) khy[i] = rm_key(a.hybrid[beg + i]);
            for (int c = 0; c < a.n_scores; ++c) k32[(c + 1) * RM_NT + i] = rm_key(a.scores[c * K + beg + i]);
        }
        __syncthreads();
        if (in) {
            if (a.n_scores) {
                const int rt = rm_rank(k32, n, k32[i], i);
                for (int c = 0; c < a.n_scores; ++c) {
                    const float* kc = k32 + (c + 1) * RM_NT;
                    const int rc = rm_rank(kc, n, kc[i], i);
                    if (rc != rt) atomicMin(&first[c], rc);
                }
            }
            if (t64) {
                const int rt = rm_rank(k64, n, k64[i], i);
                ix[i] = rt;
                if (hyb) {
                    const int rh = rm_rank(khy, n, khy[i], i);
                    if (rh != rt) atomicMin(&first[a.n_scores], rh);
                }
            }
        }
        __syncthreads();
        if (in)
            for (int p = 0; p < a.n_perms; ++p) {
                const int c = a.perms[p * K + beg + i];   // thread i: rank i of the permutation
                if ((unsigned)c >= (unsigned)n || ix[c] != i) atomicMin(&first[row_p + p], i);
            }
    } else {
        if (a.n_scores) {
            rank_desc_lds<RM_NT>(a.truth32 + beg, n, (float*)kv, ix);
            for (int i = threadIdx.x; i < n; i += RM_NT) ord[0][i] = (short)ix[i];
            __syncthreads();
        }
        if (t64) {
            rank_desc_lds<RM_NT>(a.truth64 + beg, n, kv, ix);
            for (int i = threadIdx.x; i < n; i += RM_NT) ord[1][i] = (short)ix[i];
            __syncthreads();
        }
        for (int c = 0; c < a.n_scores; ++c) {
            rank_desc_lds<RM_NT>(a.scores + c * K + beg, n, (float*)kv, ix);
            for (int i = threadIdx.x; i < n; i += RM_NT)
                if (ix[i] != ord[0][i]) atomicMin(&first[c], i);
            __syncthreads();   // the next sort rewrites kv / ix
        }
        if (hyb) {
            rank_desc_lds<RM_NT>(a.hybrid + beg, n, kv, ix);
            for (int i = threadIdx.x; i < n; i += RM_NT)
                if (ix[i] != ord[1][i]) atomicMin(&first[a.n_scores], i);
        }
        for (int p = 0; p < a.n_perms; ++p)
            for (int i = threadIdx.x; i < n; i += RM_NT)
                if (a.perms[p * K + beg + i] != ord[1][i]) atomicMin(&first[row_p + p], i);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < rows; r += RM_NT) a.dev[(size_t)r * a.n_samples + s] = first[r];
}
