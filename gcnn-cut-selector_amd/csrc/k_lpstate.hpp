// k_lpstate.hpp -- the model's input state from a raw LP snapshot, on the device: the arithmetic of the reference's get_state
// (utils.py:35-238) that is not a walk over solver objects.  Input: the LP rows and the candidate cuts as CSR over LP column
// positions plus per-row / per-column / per-cut vectors, all in the solver's float64 (include/gcnn_hip.h: gcnn_lp_state).  Output:
// the seven arrays of the model's input tuple in fp32 / int32 and cut_index (state position -> input cut).  Two launches:
//   k_lp_stats  column blocks: the 14 variable features, and per 256-column chunk the partial sums of obj^2 and (primal - lp)^2;
//               row blocks: per row sum a^2 and a.obj (16 lanes a row), and per 256-row chunk how many rows list an lhs / rhs side
//               and how many entries those have; cut blocks: per cut sum a^2, a.lp, a.obj, a.(primal - lp), the integer support
//               and the side the cut takes, and the same chunk counts.  Rows are checked on the way (offsets monotone and inside
//               the arrays, columns strictly increasing and in range); a violation is noted in the block's own flag word and such a row is
//               read as empty or as far as it is valid.  The blocks also clear the zero block of the single-state plan that runs behind (gcnn_lp_infer).
//   k_lp_emit   row / cut blocks: every block adds up the chunk counts in front of it (integers: any order), scans its own 256
//               rows, and writes features and (row, col)-sorted edges at their final places: lhs sides first (negated), then rhs
//               sides, each in input order.  Cut blocks first add the column chunks' partial sums in a fixed order (no float
//               atomics anywhere: the same bits from run to run).  One more block compares the totals with the sizes the host
//               computed and publishes the flag words.
// Sums, divisions and square roots are fp64; every output is rounded to fp32 once.  Every store is bounds-checked against the
// sizes the caller allocated, whatever the snapshot holds.  The semantics are restated in tests/lpstate_restate.py.
#pragma once

#define LP_NT 256          // threads per block = rows / columns / cuts per chunk
#define LP_SUB 16          // lanes that share one row or cut
#define LP_F_COLUMN 0      // flag words: a column outside [0, n_cols)
#define LP_F_ORDER 1       //             columns of a row or cut not strictly increasing
#define LP_F_OFFSETS 2     //             row_ptr / cut_ptr not monotone inside [0, nnz]
#define LP_F_SIZES 3       //             the state's sizes differ from the ones the host computed

struct LpArgs {
    // the snapshot
    const int* row_ptr; const int* row_col; const double* row_val;
    const double *row_lhs, *row_rhs, *row_dual; const signed char* row_basis;
    const signed char* col_type; const double *col_obj, *col_lb, *col_ub; const signed char* col_basis;
    const double *col_lp, *col_redcost, *col_primal, *col_avg;
    const int* cut_ptr; const int* cut_col; const double* cut_val; const double *cut_lhs, *cut_rhs;
    int R, V, K, nnz_r, nnz_k, has_inc, n_model_vars;
    int C, E1;                    // the state's constraint rows and edges as the host computed them (they size the outputs)
    double infinity, eps, obj_norm;
    // scratch between the two launches
    double* row_stat;             // [R][2]  sum a^2, a.obj
    int* row_part;                // [nrc][4] per chunk: lhs rows, their entries, rhs rows, their entries
    double* col_part;             // [ncc][2] per chunk: sum obj^2, sum (primal - lp)^2
    double* cut_stat;             // [K][4]  sum a^2, a.lp, a.obj, a.(primal - lp)
    int* cut_aux;                 // [K][2]  integer columns, side (1 = lhs)
    int* cut_part;                // [nkc][4]
    int* blk_flags;               // [blocks of k_lp_stats] the violations each block met, one bit per flag word; k_lp_emit ORs them
    int nrc, ncc, nkc, n_stat_blocks;
    // the state
    float* cons_feats; int* cons_ei; float* cons_ef; float* var_feats; float* cut_feats; int* cut_ei; float* cut_ef;
    int* cut_index; int* flags_out;
    int* zero; int zero_words;    // the plan's zero block (null: none)
};

__device__ __forceinline__ bool lp_finite(double x, double inf) { return !(fabs(x) >= inf); }
__device__ __forceinline__ bool lp_in(int x, int n) { return (unsigned)x < (unsigned)n; }   // 0 <= x < n

// entries [beg, end) of row r, clamped to what is valid; *bad: the offsets were not
__device__ __forceinline__ void lp_row_range(const int* ptr, int r, int nnz, int& beg, int& end, bool& bad) {
    beg = ptr[r]; end = ptr[r + 1];
    bad = beg < 0 || end < beg || end > nnz;
    if (bad) { beg = 0; end = 0; }
}

__device__ __forceinline__ double lp_sub_sum(double x) {      // over the LP_SUB lanes of a row, fixed order
    for (int o = LP_SUB / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ int lp_sub_sum(int x) {
    for (int o = LP_SUB / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__device__ __forceinline__ double lp_block_sum(double x, double* s) {   // fixed tree over the block; s: LP_NT doubles
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = x;
    __syncthreads();
    for (int o = LP_NT / 2; o > 0; o >>= 1) {
        if (t < o) s[t] += s[t + o];
        __syncthreads();
    }
    return s[0];
}

// exclusive scan of four counters over the block; s: 4 * LP_NT ints.  Returns the block totals in tot.
__device__ __forceinline__ void lp_block_scan4(const int (&v)[4], int (&excl)[4], int (&tot)[4], int* s) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q * LP_NT + t] = v[q];
    __syncthreads();
    for (int o = 1; o < LP_NT; o <<= 1) {
        int x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = t >= o ? s[q * LP_NT + t - o] : 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q * LP_NT + t] += x[q];
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { excl[q] = s[q * LP_NT + t] - v[q]; tot[q] = s[q * LP_NT + LP_NT - 1]; }
}

// sum of the chunk counters in front of chunk b (pre) and of all chunks (tot)
__device__ __forceinline__ void lp_chunk_prefix(const int* part, int n_chunks, int b, int (&pre)[4], int (&tot)[4], int* s) {
    int p[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < n_chunks; i += LP_NT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int x = part[4 * i + q]; a[q] += x; if (i < b) p[q] += x; }
    }
    __syncthreads();
    if (threadIdx.x < 8) s[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) { if (p[q]) atomicAdd(&s[q], p[q]); if (a[q]) atomicAdd(&s[4 + q], a[q]); }   // integers in LDS
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) { pre[q] = s[q]; tot[q] = s[4 + q]; }
    __syncthreads();
}

// What the cut-row path (k_hybrid.hpp) shares with this one, so that both hold the same bits.
// The sums of one row or cut over its entries [beg, end): the LP_SUB lanes of the row stride over them and lp_sub_sum adds the
// lanes in its fixed order.  A row takes n2 and dob only; a cut also act, the integer support and, with an incumbent, ddir.
// The violations met on the way are ORed into flag.
struct LpRowSums { double n2, act, dob, ddir; int nint; };
__device__ __forceinline__ LpRowSums lp_row_sums(const int* col, const double* val, int beg, int end, int l, int V, bool rows,
                                                 bool has_inc, const double* col_obj, const double* col_lp,
                                                 const double* col_primal, const signed char* col_type, int& flag) {
    double n2 = 0.0, act = 0.0, dob = 0.0, ddir = 0.0; int nint = 0;
    for (int e = beg + l; e < end; e += LP_SUB) {
        const int c = col[e]; const double v = val[e];
        if (e > beg && col[e - 1] >= c) flag |= 1 << LP_F_ORDER;
        n2 += v * v;
        if (c < 0 || c >= V) { flag |= 1 << LP_F_COLUMN; continue; }
        dob += v * col_obj[c];
        if (!rows) {
            const double x = col_lp[c];
            act += v * x;
            if (has_inc) ddir += v * (col_primal[c] - x);
            nint += col_type[c] != 3;
        }
    }
    LpRowSums s;
    s.n2 = lp_sub_sum(n2); s.dob = lp_sub_sum(dob); s.act = 0.0; s.ddir = 0.0; s.nint = 0;
    if (!rows) { s.act = lp_sub_sum(act); s.ddir = lp_sub_sum(ddir); s.nint = lp_sub_sum(nint); }
    return s;
}

// A column norm from the per-chunk partial sums part[stride * i], i < n_chunks: strided over the threads, then the block tree.  Every
// block that calls it adds the same partials in the same order and holds identical bits.  s: LP_NT doubles.
__device__ __forceinline__ double lp_part_norm(const double* part, int stride, int n_chunks, double* s) {
    double x = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += LP_NT) x += part[(size_t)stride * i];
    return sqrt(lp_block_sum(x, s));
}

// The three fp64 features of a cut that the hybrid rule adds up, from its sums: what cut_feats[:, 3], [:, 2] and [:, 5] round.
struct LpCutTerms { double norm, feas, efficacy, int_support, parallelism; };
__device__ __forceinline__ LpCutTerms lp_cut_terms(double n2, double act, double dob, int nint, int len, double lo, double hi,
                                                   double objn) {
    LpCutTerms f;
    const double raw = sqrt(n2);
    f.norm = raw == 0.0 ? 1.0 : raw;
    f.feas = fmin(hi - act, act - lo);
    f.efficacy = -f.feas / f.norm;
    f.int_support = (double)nint / (double)len;
    const double prod = raw * objn;
    f.parallelism = prod == 0.0 ? 0.0 : fabs(dob) / prod;
    return f;
}

// The two launches' bodies as functions of (arguments, block index within the snapshot's share of the launch): the solo kernels
// below run them on their own grid, k_lpbatch.hpp's kernels on each snapshot's share of one grid.  Everything that depends on the
// block partition -- the chunking in 256s, the pre[] / tot[] terms, the order of the column partials -- is a function of these two
// alone, so a snapshot's state has the same bits in either launch.  The chunk counts are the arguments' nrc / ncc / nkc.
__device__ __forceinline__ void lp_stats_body(const LpArgs& a, const int blk) {
    __shared__ double sd[LP_NT];
    __shared__ int si[5];
    const int t = threadIdx.x;
    int b = blk;
    if (b < a.ncc) {                                            // ---- columns
        const int j = b * LP_NT + t;
        double o2 = 0.0, d2 = 0.0;
        if (j < a.V) {
            const int ty = a.col_type[j], bs = a.col_basis[j];
            const double obj = a.col_obj[j], x = a.col_lp[j];
            float* f = a.var_feats + (size_t)j * 14;
            f[0] = ty == 0; f[1] = ty == 1; f[2] = ty == 2; f[3] = ty == 3;
            f[4] = (float)(obj / a.obj_norm);
            f[5] = lp_finite(a.col_lb[j], a.infinity); f[6] = lp_finite(a.col_ub[j], a.infinity);
            f[7] = bs == 0; f[8] = bs == 2;
            f[9] = ty == 3 ? 0.f : (float)(0.5 - fabs(x - floor(x) - 0.5));
            f[10] = (float)(a.col_redcost[j] / a.obj_norm);
            f[11] = (float)x;
            double pr = 0.0, av = 0.0;
            if (a.has_inc) { pr = a.col_primal[j]; av = a.col_avg[j]; const double d = pr - x; d2 = d * d; }
            f[12] = (float)pr; f[13] = (float)av;
            o2 = obj * obj;
        }
        o2 = lp_block_sum(o2, sd);
        d2 = lp_block_sum(d2, sd);
        if (t == 0) { a.col_part[2 * b] = o2; a.col_part[2 * b + 1] = d2; a.blk_flags[blk] = 0; }
        return;
    }
    b -= a.ncc;
    const bool rows = b < a.nrc;
    if (!rows) b -= a.nrc;
    const int n = rows ? a.R : a.K, nnz = rows ? a.nnz_r : a.nnz_k;
    const int* ptr = rows ? a.row_ptr : a.cut_ptr; const int* col = rows ? a.row_col : a.cut_col;
    const double* val = rows ? a.row_val : a.cut_val;
    const double* lhs = rows ? a.row_lhs : a.cut_lhs; const double* rhs = rows ? a.row_rhs : a.cut_rhs;
    if (t < 5) si[t] = 0;
    __syncthreads();
    const int g = t / LP_SUB, l = t % LP_SUB;
    int cnt[4] = {0, 0, 0, 0}, flag = 0;
    for (int it = 0; it < LP_NT / (LP_NT / LP_SUB); ++it) {
        const int r = b * LP_NT + it * (LP_NT / LP_SUB) + g;
        int beg = 0, end = 0; bool bad = false;
        if (r < n) lp_row_range(ptr, r, nnz, beg, end, bad);
        if (bad) flag |= 1 << LP_F_OFFSETS;
        const LpRowSums m = lp_row_sums(col, val, beg, end, l, a.V, rows, a.has_inc != 0, a.col_obj, a.col_lp, a.col_primal,
                                        a.col_type, flag);
        const double n2 = m.n2, act = m.act, dob = m.dob, ddir = m.ddir; const int nint = m.nint;
        if (l == 0 && r < n) {
            const int len = end - beg;
            const double lo = lhs[r], hi = rhs[r];
            if (rows) {
                a.row_stat[2 * (size_t)r] = n2; a.row_stat[2 * (size_t)r + 1] = dob;
                if (lp_finite(lo, a.infinity)) { cnt[0] += 1; cnt[1] += len; }
                if (lp_finite(hi, a.infinity)) { cnt[2] += 1; cnt[3] += len; }
            } else {
                double* s = a.cut_stat + 4 * (size_t)r;
                s[0] = n2; s[1] = act; s[2] = dob; s[3] = ddir;
                const int side = lp_finite(lo, a.infinity) && (lo - act) > (act - hi);   // most violated side; a tie takes rhs
                a.cut_aux[2 * r] = nint; a.cut_aux[2 * r + 1] = side;
                cnt[side ? 0 : 2] += 1; cnt[side ? 1 : 3] += len;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (cnt[q]) atomicAdd(&si[q], cnt[q]);
    if (flag) atomicOr(&si[4], flag);                          // (LDS)
    __syncthreads();
    if (t < 4) (rows ? a.row_part : a.cut_part)[4 * b + t] = si[t];
    if (t == 0) a.blk_flags[blk] = si[4];               // every block writes its word: nothing to clear, nothing shared
}

__global__ __launch_bounds__(LP_NT) void k_lp_stats(LpArgs a) {
    if (a.zero) for (int i = blockIdx.x * LP_NT + threadIdx.x; i < a.zero_words; i += gridDim.x * LP_NT) a.zero[i] = 0;
    lp_stats_body(a, blockIdx.x);
}

// What the resident-LP path (k_lpres.hpp) takes from the same body, so that both hold the same bits; every member null (the
// default) is this file's own behaviour.  row_place [R][2] and row_scale [R]: the rows are emitted without their solve-dependent half
// (row_dual and row_basis are not read, cons_feats columns 1 and 3 are zero) and every row's two state places (-1: side not listed)
// and its dual divisor norm * obj_norm are recorded.  cut_l_ptr [K+1]: the cut edges' by-cut offsets, at the cuts' state places.
struct LpEmitMore { int* row_place; double* row_scale; int* cut_l_ptr; };
__device__ __forceinline__ void lp_emit_body(const LpArgs& a, const int blk, const LpEmitMore more = LpEmitMore{nullptr, nullptr, nullptr}) {
    __shared__ int si[4 * LP_NT];
    __shared__ double sd[LP_NT];
    __shared__ int s_pos[LP_NT], s_ofs[2][LP_NT];      // per row: state position of the lhs copy (-1: none), edge offsets (-1: none)
    __shared__ int s_pos2[LP_NT];
    const int t = threadIdx.x;
    int b = blk;
    int pre[4], tot[4];
    if (b == a.nrc + a.nkc) {                          // ---- the totals against the host's sizes, and the flag words
        lp_chunk_prefix(a.row_part, a.nrc, 0, pre, tot, si);
        int f = 0;
        for (int i = t; i < a.n_stat_blocks; i += LP_NT) f |= a.blk_flags[i];
        if (t == 0) si[0] = 0;
        __syncthreads();
        if (f) atomicOr(&si[0], f);
        __syncthreads();
        if (t < 4) {
            int w = si[0] >> t & 1;
            if (t == LP_F_SIZES && (tot[0] + tot[2] != a.C || tot[1] + tot[3] != a.E1)) w = 1;
            a.flags_out[t] = w;
        }
        if (more.cut_l_ptr && t == 0) more.cut_l_ptr[a.K] = a.nnz_k;
        return;
    }
    const bool rows = b < a.nrc;
    if (!rows) b -= a.nrc;
    const int n = rows ? a.R : a.K, nnz = rows ? a.nnz_r : a.nnz_k;
    const int n_left = rows ? a.C : a.K, n_edges = rows ? a.E1 : a.nnz_k;
    const int* ptr = rows ? a.row_ptr : a.cut_ptr; const int* col = rows ? a.row_col : a.cut_col;
    const double* val = rows ? a.row_val : a.cut_val;
    int* ei = rows ? a.cons_ei : a.cut_ei; float* ef = rows ? a.cons_ef : a.cut_ef;
    lp_chunk_prefix(rows ? a.row_part : a.cut_part, rows ? a.nrc : a.nkc, b, pre, tot, si);
    double objn = 0.0, dirn = 0.0;
    if (!rows) {                                       // |col_obj| and |primal - lp|: the column chunks' sums in a fixed order.
        // Every cut block recomputes both from the same partials in the same order, so all blocks hold identical bits; nothing
        // is shared between blocks (one block computing them for all would need a third launch).
        objn = lp_part_norm(a.col_part, 2, a.ncc, sd);
        dirn = lp_part_norm(a.col_part + 1, 2, a.ncc, sd);
    }
    const int r = b * LP_NT + t;
    int beg = 0, end = 0; bool bad = false;
    bool has_l = false, has_r = false;
    double lo = 0.0, hi = 0.0;
    if (r < n) {
        lp_row_range(ptr, r, nnz, beg, end, bad);
        lo = (rows ? a.row_lhs : a.cut_lhs)[r]; hi = (rows ? a.row_rhs : a.cut_rhs)[r];
        if (rows) { has_l = lp_finite(lo, a.infinity); has_r = lp_finite(hi, a.infinity); }
        else { has_l = a.cut_aux[2 * r + 1] != 0; has_r = !has_l; }
    }
    const int len = end - beg;
    const int v[4] = {has_l, has_l ? len : 0, has_r, has_r ? len : 0};
    int ex[4], bt[4];
    lp_block_scan4(v, ex, bt, si);
    const int pos_l = pre[0] + ex[0], ofs_l = pre[1] + ex[1];
    const int pos_r = tot[0] + pre[2] + ex[2], ofs_r = tot[1] + pre[3] + ex[3];
    double norm = 1.0;
    if (r < n) {
        const double n2 = rows ? a.row_stat[2 * (size_t)r] : a.cut_stat[4 * (size_t)r];
        const double raw = sqrt(n2);
        norm = raw == 0.0 ? 1.0 : raw;
        if (rows) {
            const double den = norm * a.obj_norm;
            const double cosine = a.row_stat[2 * (size_t)r + 1] / den;
            const bool resident = more.row_place != nullptr;      // the solve-dependent half is left to the rounds: zeros here
            const double dual = resident ? 0.0 : a.row_dual[r] / den;
            const int bs = resident ? 1 : a.row_basis[r];
            if (resident) {
                more.row_place[2 * (size_t)r] = has_l ? pos_l : -1; more.row_place[2 * (size_t)r + 1] = has_r ? pos_r : -1;
                more.row_scale[r] = den;
            }
            if (has_l && lp_in(pos_l, n_left))
                ((float4*)a.cons_feats)[pos_l] = make_float4((float)(-(lo / norm)), bs == 0, (float)(-cosine), (float)(-dual));
            if (has_r && lp_in(pos_r, n_left))
                ((float4*)a.cons_feats)[pos_r] = make_float4((float)(hi / norm), bs == 2, (float)cosine, (float)dual);
        } else {
            const double* s = a.cut_stat + 4 * (size_t)r;
            const LpCutTerms f64 = lp_cut_terms(s[0], s[1], s[2], a.cut_aux[2 * r], len, lo, hi, objn);
            double cutoff = 0.0;
            if (a.has_inc) {
                double d = dirn > 0.0 ? s[3] / dirn : 0.0;
                if (fabs(d) <= a.eps) d = copysign(a.eps, d);
                cutoff = fmin(-f64.feas / fabs(d), a.infinity);
            }
            const int pos = has_l ? pos_l : pos_r;
            if (more.cut_l_ptr && lp_in(pos, n_left)) more.cut_l_ptr[pos] = min(max(has_l ? ofs_l : ofs_r, 0), n_edges);
            if (lp_in(pos, n_left)) {
                float* f = a.cut_feats + (size_t)pos * 6;
                f[0] = (float)(has_l ? -(lo / norm) : hi / norm);
                f[1] = (float)((double)len / (double)a.n_model_vars);
                f[2] = (float)f64.int_support;
                f[3] = (float)f64.efficacy;
                f[4] = (float)cutoff;
                f[5] = (float)f64.parallelism;
                a.cut_index[pos] = r;
            }
        }
    }
    __syncthreads();
    s_pos[t] = has_l ? pos_l : -1; s_ofs[0][t] = has_l ? ofs_l : -1;
    s_pos2[t] = has_r ? pos_r : -1; s_ofs[1][t] = has_r ? ofs_r : -1;
    sd[t] = norm;
    __syncthreads();
    // the edges: LP_SUB lanes a row, a / norm negated for an lhs copy, at (state row, column) in input column order
    const int g = t / LP_SUB, l = t % LP_SUB;
    for (int it = 0; it < LP_SUB; ++it) {
        const int k = it * (LP_NT / LP_SUB) + g, rr = b * LP_NT + k;
        if (rr >= n) continue;
        int rb, re; bool rbad;
        lp_row_range(ptr, rr, nnz, rb, re, rbad);
        const double nr = sd[k];
        const int pl = s_pos[k], ol = s_ofs[0][k], pr = s_pos2[k], orr = s_ofs[1][k];
        for (int e = rb + l; e < re; e += LP_SUB) {
            int c = col[e];
            if (c < 0 || c >= a.V) c = 0;              // flagged by k_lp_stats; keeps every later gather inside its table
            const double x = val[e] / nr;
            const int j = e - rb;
            if (lp_in(pl, n_left) && lp_in(ol + j, n_edges)) {
                ei[ol + j] = pl; ei[n_edges + ol + j] = c; ef[ol + j] = (float)(-x);
            }
            if (lp_in(pr, n_left) && lp_in(orr + j, n_edges)) {
                ei[orr + j] = pr; ei[n_edges + orr + j] = c; ef[orr + j] = (float)x;
            }
        }
    }
}

__global__ __launch_bounds__(LP_NT) void k_lp_emit(LpArgs a) { lp_emit_body(a, blockIdx.x); }
