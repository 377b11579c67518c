// k_lpbatch.hpp -- device side of gcnn_lp_batch: the states of up to 64 raw LP snapshots built in ONE pair of launches
// (gcnn_lpbatch.hpp), each where gcnn_infer_batch's upload would have put it.
//
//   k_lpset_stats  the blocks of k_lp_stats of every snapshot, back to back; they also clear the union's zero block
//   k_lpset_emit   the blocks of k_lp_emit of every snapshot, back to back
// A block finds its snapshot in the descriptor table's block-prefix column and runs the solo body (k_lpstate.hpp) with that
// snapshot's arguments and its block index WITHIN the snapshot, so every per-snapshot quantity has the solo launch's bits.
//
// The table rides in the upload: a head (the two block-prefix columns), then one entry per snapshot with what LpArgs carries, every
// pointer as a byte position from the arena's start (the host fills the table without knowing where the arena lies).  64 LpArgs do
// not fit kernel arguments; the table is read through the constant address space, as the group kernels read theirs (k_group.hpp):
// the block-uniform loads go to scalar registers as kernel arguments do.
#pragma once

#define LPSET_MAX 64
#define LPSET_TS 72        // block-prefix stride: LPSET_MAX + 1 entries, padded to a multiple of 4
#define LPSET_CONST __attribute__((address_space(4)))

struct LpSetHead {
    int n, pad[3];
    int blk0[2][LPSET_TS];     // first block of snapshot s in k_lpset_stats / k_lpset_emit; entry n = the grid
};
struct LpSetEntry {
    long long snap[22];        // the packed arrays, GCNN_LP_* order ([0]: the reserved header, not read)
    long long scratch[7];      // row_stat, cut_stat, col_part, row_part, cut_part, cut_aux, blk_flags
    long long dst[9];          // cons_feats, cons_ei, cons_ef, var_feats, cut_feats, cut_ei, cut_ef, cut_index, the four LP flags
    double infinity, eps, obj_norm;
    int R, V, K, nnz_r, nnz_k, has_inc, n_model_vars, C, E1;
    int nrc, ncc, nkc, n_stat_blocks, pad[5];
};
static_assert(sizeof(LpSetHead) % 16 == 0 && sizeof(LpSetEntry) % 16 == 0, "16-byte records");

struct LpSetArgs {
    const void* table;         // LpSetHead, then n LpSetEntry
    char* base;                // the arena
    int* zero; int zero_words; // the union's zero block: per-state flags and both by-left offset arrays
};

// the snapshot that owns block x of launch `which`, and x within it.  A snapshot may own no block of a launch: the search takes
// the last snapshot whose first block is <= x, which is the one that has blocks there.
__device__ __forceinline__ int lpset_find(const LPSET_CONST LpSetHead* h, int which, int x, int& local) {
    const int n = h->n;
    int s = 0;
    for (int i = 1; i < n; ++i) s += x >= h->blk0[which][i];
    local = x - h->blk0[which][s];
    return s;
}

__device__ __forceinline__ LpArgs lpset_args(const LPSET_CONST LpSetEntry& e, char* base) {
    LpArgs a;
    a.row_ptr = (const int*)(base + e.snap[1]); a.row_col = (const int*)(base + e.snap[2]); a.row_val = (const double*)(base + e.snap[3]);
    a.row_lhs = (const double*)(base + e.snap[4]); a.row_rhs = (const double*)(base + e.snap[5]);
    a.row_dual = (const double*)(base + e.snap[6]); a.row_basis = (const signed char*)(base + e.snap[7]);
    a.col_type = (const signed char*)(base + e.snap[8]); a.col_obj = (const double*)(base + e.snap[9]);
    a.col_lb = (const double*)(base + e.snap[10]); a.col_ub = (const double*)(base + e.snap[11]);
    a.col_basis = (const signed char*)(base + e.snap[12]); a.col_lp = (const double*)(base + e.snap[13]);
    a.col_redcost = (const double*)(base + e.snap[14]); a.col_primal = (const double*)(base + e.snap[15]);
    a.col_avg = (const double*)(base + e.snap[16]);
    a.cut_ptr = (const int*)(base + e.snap[17]); a.cut_col = (const int*)(base + e.snap[18]); a.cut_val = (const double*)(base + e.snap[19]);
    a.cut_lhs = (const double*)(base + e.snap[20]); a.cut_rhs = (const double*)(base + e.snap[21]);
    a.R = e.R; a.V = e.V; a.K = e.K; a.nnz_r = e.nnz_r; a.nnz_k = e.nnz_k; a.has_inc = e.has_inc; a.n_model_vars = e.n_model_vars;
    a.C = e.C; a.E1 = e.E1;
    a.infinity = e.infinity; a.eps = e.eps; a.obj_norm = e.obj_norm;
    a.row_stat = (double*)(base + e.scratch[0]); a.cut_stat = (double*)(base + e.scratch[1]); a.col_part = (double*)(base + e.scratch[2]);
    a.row_part = (int*)(base + e.scratch[3]); a.cut_part = (int*)(base + e.scratch[4]); a.cut_aux = (int*)(base + e.scratch[5]);
    a.blk_flags = (int*)(base + e.scratch[6]);
    a.nrc = e.nrc; a.ncc = e.ncc; a.nkc = e.nkc; a.n_stat_blocks = e.n_stat_blocks;
    a.cons_feats = (float*)(base + e.dst[0]); a.cons_ei = (int*)(base + e.dst[1]); a.cons_ef = (float*)(base + e.dst[2]);
    a.var_feats = (float*)(base + e.dst[3]); a.cut_feats = (float*)(base + e.dst[4]); a.cut_ei = (int*)(base + e.dst[5]);
    a.cut_ef = (float*)(base + e.dst[6]); a.cut_index = (int*)(base + e.dst[7]); a.flags_out = (int*)(base + e.dst[8]);
    a.zero = nullptr; a.zero_words = 0;
    return a;
}

__global__ __launch_bounds__(LP_NT) void k_lpset_stats(LpSetArgs g) {
    for (int i = blockIdx.x * LP_NT + threadIdx.x; i < g.zero_words; i += gridDim.x * LP_NT) g.zero[i] = 0;
    const LPSET_CONST LpSetHead* h = (const LPSET_CONST LpSetHead*)g.table;
    int b;
    const int s = lpset_find(h, 0, blockIdx.x, b);
    const LpArgs a = lpset_args(((const LPSET_CONST LpSetEntry*)(h + 1))[s], g.base);
    if (b < a.n_stat_blocks) lp_stats_body(a, b);
}

__global__ __launch_bounds__(LP_NT) void k_lpset_emit(LpSetArgs g) {
    const LPSET_CONST LpSetHead* h = (const LPSET_CONST LpSetHead*)g.table;
    int b;
    const int s = lpset_find(h, 1, blockIdx.x, b);
    const LpArgs a = lpset_args(((const LPSET_CONST LpSetEntry*)(h + 1))[s], g.base);
    if (b <= a.nrc + a.nkc) lp_emit_body(a, b);
}
