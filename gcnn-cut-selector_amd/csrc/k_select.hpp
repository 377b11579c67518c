// k_select.hpp -- cut selection on the device: the greedy parallelism filter of the SCIP plugin's cutselselect
// (model_evaluator.py:109-154; the same loop in model_benchmarker.py:112-157 and data_collector.py:150-195) over a scored state.
//
// get_state stores every cut row as coefficient / norm (utils.py:214-236), so SCIP's Euclidean row parallelism |a.b|/(|a||b|) of
// two cuts is the plain |a.b| of their stored rows.  Two launches:
//   k_sel_pairs   one block per pivot row (a cut, or a forced row): the pivot is scattered into an LDS dense vector (fp64, column
//                 chunks of SEL_CH), every partner row is gathered against it by one lane in its stored order with an fp64
//                 accumulator, and a wave ballot turns 64 partners' parallelisms into two 64-bit words: P > p_max, P > p_max_ub.
//                 Cut pivot i covers the partners j > i only (P(i,j) is computed once), a forced row covers every cut.
//   k_sel_filter  one block per state: the bitonic ranking of k_rank_scores, then the forced phase and the main phase over those
//                 bits.  Pivots without a marked partner are skipped in bulk: every wave tests its own candidate pivots with
//                 ballots, without barriers, until one of them has a partner to remove; only such pivots cost block-wide steps.
// The semantics (state order throughout, low-quality flags fixed by position, removed cuts behind the earlier tail) are restated
// in tests/cutsel_restate.py.
#pragma once

#define SEL_MAX_CUTS 4096        // the ranking's limit (RK_MAX)
#define SEL_NT 512               // threads per block of both kernels
#define SEL_NW (SEL_NT / 64)
#define SEL_WPW (SEL_MAX_CUTS / 64 / SEL_NW)   // partner words per wave and pivot: 8
#define SEL_CH 8192              // columns per LDS chunk of the pivot row (64 KiB of doubles: two blocks per CU)

struct SelArgs {
    const float* q;                                        // [total_cuts] quality, state order within each sample
    const int* c_ptr; const int* c_col; const float* c_val;   // cut rows (by-left CSR, rows = stacked cut index)
    const int* c_off;                                      // [n_samples+1] first cut of each sample, or null: one sample
    const int* f_ptr; const int* f_col; const float* f_val;   // forced rows, same column space (rows = stacked forced index)
    const int* f_off;                                      // [n_samples+1] or null: one sample
    int n_samples, total_cuts, total_forced, max_cuts, n_vars, words;   // words = 64-bit words per bit row = ceil(max_cuts/64)
    double p_max, p_max_ub;
    unsigned long long* bits;   // [(total_cuts + total_forced) * words][2]: row of sample s, pivot k at (c_off[s]+f_off[s]+k)
    int* order;                 // [total_cuts] sample-local cut indices
    int* n_kept;                // [n_samples]; -1 for a sample with more than max_cuts cuts (nothing else written for it)
};

__device__ __forceinline__ int sel_off(const int* off, int s, int total) { return off ? off[s] : (s ? total : 0); }

__device__ __forceinline__ int wave_min_i(int x) {
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ int wave_max_i(int x) {
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
    return x;
}

// block `bid` of `nblk`: the solo launch runs it with (blockIdx.x, gridDim.x), a launch of several sessions' selections
// (k_lprounds.hpp) with the member's solo pair
__device__ __forceinline__ void sel_pairs_body(const SelArgs& a, const int bid, const int nblk) {
    __shared__ double x[SEL_CH];
    __shared__ int red[2][SEL_NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < SEL_CH; k += SEL_NT) x[k] = 0.0;   // kept zero between pivots: each pivot clears what it set
    const int n_rows = a.total_cuts + a.total_forced;
    for (int g = bid; g < n_rows; g += nblk) {
        int s = 0, hi_s = a.n_samples;   // the sample: largest s with c_off[s] + f_off[s] <= g
        while (hi_s - s > 1) {
            const int mid = (s + hi_s) >> 1;
            if (sel_off(a.c_off, mid, a.total_cuts) + sel_off(a.f_off, mid, a.total_forced) <= g) s = mid; else hi_s = mid;
        }
        const int c0 = sel_off(a.c_off, s, a.total_cuts), K = sel_off(a.c_off, s + 1, a.total_cuts) - c0;
        const int f0 = sel_off(a.f_off, s, a.total_forced);
        if (K > a.max_cuts || K <= 0) continue;   // k_sel_filter reports a sample that is too large
        const int local = g - c0 - f0;
        const bool is_cut = local < K;
        const int* pcol = is_cut ? a.c_col : a.f_col;
        const float* pval = is_cut ? a.c_val : a.f_val;
        const int prow = is_cut ? c0 + local : f0 + local - K;
        const int pb = (is_cut ? a.c_ptr : a.f_ptr)[prow], pe = (is_cut ? a.c_ptr : a.f_ptr)[prow + 1];
        const int nw = (K + 63) >> 6, w0 = is_cut ? (local + 1) >> 6 : 0;
        if (w0 >= nw) continue;
        // column span of the pivot's entries (entries outside [0, n_vars) take no part)
        int mn = 0x7fffffff, mx = -1;
        for (int e = pb + threadIdx.x; e < pe; e += SEL_NT) {
            const int c = pcol[e];
            if (c >= 0 && c < a.n_vars) { mn = min(mn, c); mx = max(mx, c); }
        }
        mn = wave_min_i(mn); mx = wave_max_i(mx);
        if (lane == 0) { red[0][wave] = mn; red[1][wave] = mx; }
        __syncthreads();
        mn = red[0][0]; mx = red[1][0];
        for (int w = 1; w < SEL_NW; ++w) { mn = min(mn, red[0][w]); mx = max(mx, red[1][w]); }
        double acc[SEL_WPW];
#pragma unroll
        for (int t = 0; t < SEL_WPW; ++t) acc[t] = 0.0;
        for (int base = mn; base <= mx; base += SEL_CH) {   // usually one chunk; none for an empty pivot (P = 0)
            const int top = min(base + SEL_CH, a.n_vars);
            // duplicate (row, col) entries add: two entries give the same fp64 sum in either order
            for (int e = pb + threadIdx.x; e < pe; e += SEL_NT) {
                const int c = pcol[e];
                if (c >= base && c < top) atomicAdd(&x[c - base], (double)pval[e]);
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < SEL_WPW; ++t) {
                const int w = w0 + wave + SEL_NW * t;
                const int j = w * 64 + lane;
                if (w < nw && j < K && (!is_cut || j > local)) {
                    double sum = 0.0;
                    const int q0 = a.c_ptr[c0 + j], q1 = a.c_ptr[c0 + j + 1];
                    // the partner's entries in their stored order; eight loads in flight per lane (a serial chain of
                    // dependent-latency loads was 50-75 us per pivot on rows of up to 200 entries)
                    int f = q0;
                    for (; f + 8 <= q1; f += 8) {
                        int c[8];
                        float v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) { c[u] = a.c_col[f + u]; v[u] = a.c_val[f + u]; }
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (c[u] >= base && c[u] < top) sum += (double)v[u] * x[c[u] - base];
                    }
                    for (; f < q1; ++f) {
                        const int c = a.c_col[f];
                        if (c >= base && c < top) sum += (double)a.c_val[f] * x[c - base];
                    }
                    acc[t] += sum;
                }
            }
            __syncthreads();
            for (int e = pb + threadIdx.x; e < pe; e += SEL_NT) {
                const int c = pcol[e];
                if (c >= base && c < top) x[c - base] = 0.0;
            }
            __syncthreads();
        }
        unsigned long long* row = a.bits + (size_t)g * a.words * 2;
#pragma unroll
        for (int t = 0; t < SEL_WPW; ++t) {
            const int w = w0 + wave + SEL_NW * t;
            if (w < nw) {   // uniform per wave
                const int j = w * 64 + lane;
                const bool valid = j < K && (!is_cut || j > local);
                const double P = fabs(acc[t]);
                const unsigned long long b1 = __ballot(valid && P > a.p_max), b2 = __ballot(valid && P > a.p_max_ub);
                if (lane == 0) { row[2 * w] = b1; row[2 * w + 1] = b2; }
            }
        }
        __syncthreads();   // red[] is rewritten by the next pivot
    }
}
__global__ __launch_bounds__(SEL_NT) void k_sel_pairs(SelArgs a) { sel_pairs_body(a, blockIdx.x, gridDim.x); }

// Stable partition of positions [0, K): those of [0, n) for which flag(p) holds move behind everything else, in position order.
// Returns how many moved.  All threads of the block call it; thread t owns the positions [t*S, t*S+S).
template <class Flag>
__device__ int sel_remove(int* ord, int* tmp, int* scan, int K, int n, Flag flag) {
    const int S = (K + SEL_NT - 1) / SEL_NT;   // <= 8
    const int p0 = threadIdx.x * S, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned m = 0;
    int cnt = 0;
    for (int k = 0; k < S; ++k) {
        const int p = p0 + k;
        if (p < n && flag(p)) { m |= 1u << k; ++cnt; }
    }
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) scan[wave] = incl;
    __syncthreads();
    int before = incl - cnt, total = 0;
    for (int w = 0; w < SEL_NW; ++w) {
        const int c = scan[w];
        total += c;
        if (w < wave) before += c;
    }
    __syncthreads();   // scan[] is rewritten by the next call
    if (total == 0) return 0;
    for (int k = 0; k < S; ++k) {
        const int p = p0 + k;
        if (p >= K) break;
        if ((m >> k) & 1) tmp[K - total + before++] = ord[p];
        else tmp[p - before] = ord[p];
    }
    __syncthreads();
    for (int p = threadIdx.x; p < K; p += SEL_NT) ord[p] = tmp[p];
    __syncthreads();
    return total;
}

// The filter of one sample (block s) over a key of type T: q holds the stacked qualities (a.q is not read), compared as they are --
// an fp64 key is never narrowed.  k_sel_filter runs it on the model's fp32 scores, k_hyb_filter (k_hybrid.hpp) on the fp64 hybrid
// quality.  filter = false stops behind the ranking: order = the ranking, n_kept = K, no pair bit is read.
// LDS: (12 + sizeof(T)) * SEL_MAX_CUTS + a few words -- 52 KiB for fp32, 68 KiB for fp64: two blocks per CU either way.
template <class T>
__device__ __forceinline__ void sel_filter_body(const SelArgs& a, const T* q, const int s, const bool filter) {
    __shared__ T v[SEL_MAX_CUTS];
    __shared__ int ord[SEL_MAX_CUTS];
    __shared__ int tmp[SEL_MAX_CUTS];
    __shared__ unsigned char low[SEL_MAX_CUTS];
    __shared__ int scan[SEL_NW];
    __shared__ int best;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = sel_off(a.c_off, s, a.total_cuts), K = sel_off(a.c_off, s + 1, a.total_cuts) - c0;
    const int f0 = sel_off(a.f_off, s, a.total_forced), F = sel_off(a.f_off, s + 1, a.total_forced) - f0;
    if (K > a.max_cuts || K < 0) {
        if (threadIdx.x == 0) a.n_kept[s] = -1;
        return;
    }
    if (K == 0) {
        if (threadIdx.x == 0) a.n_kept[s] = 0;
        return;
    }
    rank_desc_lds<SEL_NT>(q + c0, K, v, ord);
    if (!filter) {
        for (int p = threadIdx.x; p < K; p += SEL_NT) a.order[c0 + p] = ord[p];
        if (threadIdx.x == 0) a.n_kept[s] = K;
        return;
    }
    // low-quality flags by POSITION, from the raw scores in ranked order: Q[p] < t in T, t = T(0.9 * double(Q[0]))
    // (NumPy 1.22: 0.9 * a float32 scalar is a float64; comparing the float32 array with it rounds it to float32.  A float64
    // array is compared with the float64 product as it is.)
    const T t = (T)(0.9 * (double)q[c0 + ord[0]]);
    for (int p = threadIdx.x; p < K; p += SEL_NT) low[p] = q[c0 + ord[p]] < t;
    __syncthreads();
    const unsigned long long* bits = a.bits + (size_t)(c0 + f0) * a.words * 2;
    const int words = a.words;
    // predicate of the cut at position p against pivot row r (bit row r, column c): P > p_max and (low[p] or P > p_max_ub)
    auto hit = [&](int r, int c, int p) -> bool {
        const unsigned long long* w = bits + ((size_t)r * words + (c >> 6)) * 2;
        const unsigned long long m = 1ull << (c & 63);
        return (w[0] & m) && (low[p] || (w[1] & m));
    };
    auto hit_cut = [&](int piv, int c, int p) { return hit(min(piv, c), max(piv, c), p); };   // P(i,j) lives in row min(i,j)
    int n = K;
    for (int r = 0; r < F; ++r) {   // forced phase
        const int row = K + r;
        n -= sel_remove(ord, tmp, scan, K, n, [&](int p) { return hit(row, ord[p], p); });
    }
    int i = 0;
    for (;;) {   // main phase: the next pivot with a partner to remove, then its removal
        if (threadIdx.x == 0) best = 0x7fffffff;
        __syncthreads();
        for (int c = i + wave; c < n - 1; c += SEL_NW) {
            if (c >= __builtin_amdgcn_readfirstlane(__hip_atomic_load(&best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) break;
            const int piv = ord[c];
            bool any = false;
            for (int q0 = c + 1; q0 < n && !any; q0 += 64) {
                const int p = q0 + lane;
                any = __ballot(p < n && hit_cut(piv, ord[p], p)) != 0;
            }
            if (any) {
                if (lane == 0) atomicMin(&best, c);
                break;
            }
        }
        __syncthreads();
        const int b = best;
        if (b == 0x7fffffff) break;
        const int piv = ord[b];
        n -= sel_remove(ord, tmp, scan, K, n, [&](int p) { return p > b && hit_cut(piv, ord[p], p); });
        i = b + 1;
    }
    for (int p = threadIdx.x; p < K; p += SEL_NT) a.order[c0 + p] = ord[p];
    if (threadIdx.x == 0) a.n_kept[s] = n;
}

__global__ __launch_bounds__(SEL_NT) void k_sel_filter(SelArgs a) { sel_filter_body<float>(a, a.q, blockIdx.x, true); }
