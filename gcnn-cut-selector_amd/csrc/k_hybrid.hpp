// k_hybrid.hpp -- device side of gcnn_hybrid_select: SCIP's hybrid cut quality and the parallelism filter from the cut rows of up
// to 64 snapshots, with no LP rows and no model (model_evaluator.py:104-154, model_benchmarker.py, data_collector.py:145-195):
//     quality = (efficacy + (0.1 * nint) / nnz) + 0.1 * parallelism          fp64, every operation rounded on its own
//   k_hyb_stats   column blocks: per 256-column chunk the partial sum of obj^2; cut blocks: per cut sum a^2, a.lp, a.obj and the
//                 integer support (16 lanes a cut, lp_row_sums of k_lpstate.hpp).  Rows are checked on the way as k_lp_stats checks them.
//   k_hyb_emit    cut blocks: |obj| from the chunk partials (lp_part_norm), the three fp64 features (lp_cut_terms: the values
//                 k_lp_emit rounds into cut_feats[:, 3], [:, 2] and [:, 5]), the quality, and the cut's row as a / norm in fp32
//                 into the stacked CSR that k_sel_pairs reads -- INPUT cut order, columns as given.  One more block per snapshot
//                 publishes its flag words (LP_F_COLUMN, LP_F_ORDER, LP_F_OFFSETS; word 3 stays 0).
//   k_sel_pairs   (k_select.hpp) unchanged, on those rows
//   k_hyb_filter  sel_filter_body (k_select.hpp) over the fp64 quality: the threshold 0.9 * quality[order[0]] is compared in fp64
// A block finds its snapshot in the table's block-prefix columns, read through the constant address space (k_lpbatch.hpp), and
// works on its block index WITHIN the snapshot: a snapshot's bits depend on neither its neighbours nor its position.
// No float atomics (but the fp64 LDS scatter inside k_sel_pairs); every store is bounds-checked against the host's sizes.
// The semantics are restated in tests/hybrid_restate.py.
#pragma once

struct HybHead {
    int n, pad[3];
    int blk0[2][LPSET_TS];     // first block of snapshot s in k_hyb_stats / k_hyb_emit; entry n = the grid
    int c_off[LPSET_TS];       // first cut of snapshot s in the stacked outputs (k_sel_pairs' cut_offsets); entry n = all cuts
    int f_off[LPSET_TS];       // first forced row of snapshot s (forced_offsets)
};
struct HybEntry {
    long long snap[8];         // GCNN_HYBRID_* order: cut_ptr, cut_col, cut_val, cut_lhs, cut_rhs, col_type, col_obj, col_lp
    long long scratch[4];      // cut_stat [K][4], cut_nint [K], col_part [ncc], blk_flags [n_stat_blocks]
    long long dst[6];          // quality [K] f64, features [K][3] f64, row_ptr, row_col, row_val (at this snapshot's first cut / entry), flags [4]
    double infinity;
    int V, K, nnz, ncc, nkc, n_stat_blocks, e0, pad[3];   // e0: this snapshot's first entry in the stacked rows
};
static_assert(sizeof(HybHead) % 16 == 0 && sizeof(HybEntry) % 16 == 0, "16-byte records");

struct HybArgs {
    const void* table;         // HybHead, then n HybEntry
    char* base;                // the arena
};

struct HybSnap {
    const int* cut_ptr; const int* cut_col; const double* cut_val; const double *cut_lhs, *cut_rhs;
    const signed char* col_type; const double *col_obj, *col_lp;
    double* cut_stat; int* cut_nint; double* col_part; int* blk_flags;
    double* quality; double* features; int* row_ptr; int* row_col; float* row_val; int* flags_out;
    double infinity;
    int V, K, nnz, ncc, nkc, n_stat_blocks, e0;
};

__device__ __forceinline__ int hyb_find(const LPSET_CONST HybHead* h, int which, int x, int& local) {
    const int n = h->n;
    int s = 0;
    for (int i = 1; i < n; ++i) s += x >= h->blk0[which][i];
    local = x - h->blk0[which][s];
    return s;
}

__device__ __forceinline__ HybSnap hyb_snap(const LPSET_CONST HybEntry& e, char* base) {
    HybSnap a;
    a.cut_ptr = (const int*)(base + e.snap[0]); a.cut_col = (const int*)(base + e.snap[1]); a.cut_val = (const double*)(base + e.snap[2]);
    a.cut_lhs = (const double*)(base + e.snap[3]); a.cut_rhs = (const double*)(base + e.snap[4]);
    a.col_type = (const signed char*)(base + e.snap[5]); a.col_obj = (const double*)(base + e.snap[6]);
    a.col_lp = (const double*)(base + e.snap[7]);
    a.cut_stat = (double*)(base + e.scratch[0]); a.cut_nint = (int*)(base + e.scratch[1]); a.col_part = (double*)(base + e.scratch[2]);
    a.blk_flags = (int*)(base + e.scratch[3]);
    a.quality = (double*)(base + e.dst[0]); a.features = (double*)(base + e.dst[1]); a.row_ptr = (int*)(base + e.dst[2]);
    a.row_col = (int*)(base + e.dst[3]); a.row_val = (float*)(base + e.dst[4]); a.flags_out = (int*)(base + e.dst[5]);
    a.infinity = e.infinity;
    a.V = e.V; a.K = e.K; a.nnz = e.nnz; a.ncc = e.ncc; a.nkc = e.nkc; a.n_stat_blocks = e.n_stat_blocks; a.e0 = e.e0;
    return a;
}

// SCIP's hybrid rule in Python's left-to-right evaluation of `efficacy + 0.1 * nint / nnz + 0.1 * parallelism`: four roundings in
// this association and no fused multiply-add (a fused last step differs from NumPy's in the last bit for one value in 64).
__device__ __forceinline__ double hyb_quality(double efficacy, int nint, int nnz, double parallelism) {
#pragma clang fp contract(off)
    const double a = 0.1 * (double)nint;
    const double b = a / (double)nnz;
    const double c = efficacy + b;
    const double d = 0.1 * parallelism;
    return c + d;
}

__global__ __launch_bounds__(LP_NT) void k_hyb_stats(HybArgs g) {
    __shared__ double sd[LP_NT];
    __shared__ int s_flag;
    const LPSET_CONST HybHead* h = (const LPSET_CONST HybHead*)g.table;
    int blk;
    const int s = hyb_find(h, 0, blockIdx.x, blk);
    const HybSnap a = hyb_snap(((const LPSET_CONST HybEntry*)(h + 1))[s], g.base);
    if (blk >= a.n_stat_blocks) return;
    const int t = threadIdx.x;
    if (blk < a.ncc) {                                            // ---- columns: the chunk's share of |obj|^2, as k_lp_stats adds it
        const int j = blk * LP_NT + t;
        double o2 = 0.0;
        if (j < a.V) { const double obj = a.col_obj[j]; o2 = obj * obj; }
        o2 = lp_block_sum(o2, sd);
        if (t == 0) { a.col_part[blk] = o2; a.blk_flags[blk] = 0; }
        return;
    }
    const int b = blk - a.ncc;                                    // ---- cuts
    if (t == 0) s_flag = 0;
    __syncthreads();
    const int grp = t / LP_SUB, l = t % LP_SUB;
    int flag = 0;
    for (int it = 0; it < LP_NT / (LP_NT / LP_SUB); ++it) {
        const int r = b * LP_NT + it * (LP_NT / LP_SUB) + grp;
        int beg = 0, end = 0; bool bad = false;
        if (r < a.K) lp_row_range(a.cut_ptr, r, a.nnz, beg, end, bad);
        if (bad) flag |= 1 << LP_F_OFFSETS;
        const LpRowSums m = lp_row_sums(a.cut_col, a.cut_val, beg, end, l, a.V, false, false, a.col_obj, a.col_lp, nullptr, a.col_type, flag);
        if (l == 0 && r < a.K) {
            double* st = a.cut_stat + 4 * (size_t)r;
            st[0] = m.n2; st[1] = m.act; st[2] = m.dob; st[3] = 0.0;
            a.cut_nint[r] = m.nint;
        }
    }
    if (flag) atomicOr(&s_flag, flag);                            // (LDS)
    __syncthreads();
    if (t == 0) a.blk_flags[blk] = s_flag;                        // every block writes its word: nothing to clear, nothing shared
}

__global__ __launch_bounds__(LP_NT) void k_hyb_emit(HybArgs g) {
    __shared__ double sd[LP_NT];
    __shared__ int s_flag;
    const LPSET_CONST HybHead* h = (const LPSET_CONST HybHead*)g.table;
    int b;
    const int s = hyb_find(h, 1, blockIdx.x, b);
    const HybSnap a = hyb_snap(((const LPSET_CONST HybEntry*)(h + 1))[s], g.base);
    if (b > a.nkc) return;
    const int t = threadIdx.x;
    if (b == a.nkc) {                                             // ---- the snapshot's flag words
        int f = 0;
        for (int i = t; i < a.n_stat_blocks; i += LP_NT) f |= a.blk_flags[i];
        if (t == 0) s_flag = 0;
        __syncthreads();
        if (f) atomicOr(&s_flag, f);
        __syncthreads();
        if (t < 4) a.flags_out[t] = t < LP_F_SIZES ? s_flag >> t & 1 : 0;
        return;
    }
    const double objn = lp_part_norm(a.col_part, 1, a.ncc, sd);   // the same partials in the same order in every block
    const int r = b * LP_NT + t;
    double norm = 1.0;
    if (r < a.K) {
        int beg, end; bool bad;
        lp_row_range(a.cut_ptr, r, a.nnz, beg, end, bad);
        const int len = end - beg, nint = a.cut_nint[r];
        const double* st = a.cut_stat + 4 * (size_t)r;
        const LpCutTerms f = lp_cut_terms(st[0], st[1], st[2], nint, len, a.cut_lhs[r], a.cut_rhs[r], objn);
        norm = f.norm;
        a.quality[r] = hyb_quality(f.efficacy, nint, len, f.parallelism);
        double* o = a.features + 3 * (size_t)r;
        o[0] = f.efficacy; o[1] = f.int_support; o[2] = f.parallelism;
        // k_sel_pairs walks [row_ptr[k], row_ptr[k+1]) without a check of its own: whatever the snapshot's offsets hold, what is
        // stored lies inside this snapshot's entries
        a.row_ptr[r] = a.e0 + min(max(a.cut_ptr[r], 0), a.nnz);
        if (r == a.K - 1) a.row_ptr[a.K] = a.e0 + min(max(a.cut_ptr[a.K], 0), a.nnz);
    }
    __syncthreads();
    sd[t] = norm;
    __syncthreads();
    // the rows: LP_SUB lanes a cut, a / norm in fp32 at the cut's own entries, columns as given
    const int grp = t / LP_SUB, l = t % LP_SUB;
    for (int it = 0; it < LP_SUB; ++it) {
        const int k = it * (LP_NT / LP_SUB) + grp, rr = b * LP_NT + k;
        if (rr >= a.K) continue;
        int rb, re; bool rbad;
        lp_row_range(a.cut_ptr, rr, a.nnz, rb, re, rbad);
        const double nr = sd[k];
        for (int e = rb + l; e < re; e += LP_SUB) {               // 0 <= rb <= e < re <= nnz
            int c = a.cut_col[e];
            if (c < 0 || c >= a.V) c = 0;                         // flagged by k_hyb_stats
            a.row_col[e] = c;
            a.row_val[e] = (float)(a.cut_val[e] / nr);
        }
    }
}

struct HybSelArgs {
    SelArgs sel;               // sel.q is not read
    const double* quality;     // [total_cuts] stacked
    int filter;                // 0: the ranking alone
};

__global__ __launch_bounds__(SEL_NT) void k_hyb_filter(HybSelArgs a) { sel_filter_body<double>(a.sel, a.quality, blockIdx.x, a.filter != 0); }
