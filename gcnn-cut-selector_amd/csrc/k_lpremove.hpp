// k_lpremove.hpp -- rows removed from a resident LP (k_lpres.hpp) without deriving anything again (include/gcnn_hip.h:
// gcnn_lp_rows_remove, gcnn_lp_round_remove): the mirror image of k_lpappend.hpp.  No floating-point value is computed: every kept
// value is copied and every kept index is renumbered by a monotone map, so both CSR orders stay stable and no ordering step
// follows.  A row is removed iff a binary search finds it in the uploaded, sorted list of removed LP rows.  With L0 / EL0 resident
// lhs rows / entries the new state is
//   rows          [ kept lhs | kept rhs, ids renumbered ]
//   by-left edges [ kept lhs | kept rhs, at - removed edges in front, row id renumbered ]
//   by-variable   per variable the kept entries of its old segment, in their old order, row ids renumbered;
//                 v_ptr = old v_ptr - exclusive prefix of the removed counts
// The same launches write row_place (kept rows renumbered on both sides, -1 stays -1), row_scale, l_ptr with its last entry, the
// whole 16-byte cons_feats rows and the five raw arrays with row_ptr re-based.  Everything is written out of place: the launches
// read one set of derived arrays and one set of raw rows and write the others, so a rejected call leaves the resident state as
// it was.  Three launches behind one fill of the removed counters (vcnt + vpart):
//   k_lpd_mark  a block per 256 resident LP rows: the chunk's counts of kept rows, kept raw entries and kept lhs / rhs state rows
//               and edges; then the chunk's part of the list (two binary searches), 16 lanes a removed row: per entry of a
//               removed listed side an integer atomic on the variable's counter and one on the counter of the variable's
//               256-chunk.
//   k_lpd_rows  row blocks, one per 256 resident LP rows: the chunk prefix in front (lp_chunk_prefix) plus an in-block scan give
//               every kept row its new LP row, raw offset, state rows and by-left offsets; everything by row goes to its final
//               place (row_place, row_scale, row_ptr, the two sides, cons_feats, l_ptr) and two maps are written: old state row
//               -> new, or -1, and old LP row -> new, or -1.  One block compares the totals with the host's and publishes the
//               four flag words and l_ptr's and row_ptr's last entries.  Variable blocks, one per 256 variables: the new v_ptr
//               (the chunk counters in front summed as lp_chunk_prefix does, plus an in-block scan of the removed counts).
//   k_lpd_vars  variable blocks, 16 lanes a variable: the kept entries of its segment compacted in order with a ballot prefix
//               inside the lane group (__ballot is 64 bits wide: four groups a wave), row ids through the map.  A variable with
//               n entries costs n / 16 steps of its lane group: that serves hub columns of a few thousand rows and is not
//               balanced beyond that.  Edge blocks, a thread per old by-left edge: a kept one goes to the new l_ptr of its new
//               row plus its place in the row.  Raw blocks, a thread per old raw entry: its row by binary search over the old
//               row_ptr, then likewise.  (These copies wait for k_lpd_rows's offsets, so they ride in the last launch; with a
//               thread per entry a small LP with long rows still fills the device, which a block per 256 rows did not.)
// Each kernel is its body (lpd_mark_body, lpd_rows_body, lpd_vars_body) called with blockIdx.x: none strides by its grid, so the
// block index is all the group twins of k_lpedits.hpp need to run the same bodies for one member of a grouped call.
// The maps cost no launch of their own (k_lpd_rows writes them where it has the row in hand); a sorted list of removed state rows
// would need a pass to build.  Integer atomics only; every store is bounds-checked against the sizes the host computed; no scratch
// memory, under 16 KiB of LDS.
#pragma once

struct LpdArgs {
    LpaSet src, dst;
    const int* list; int n_list;                // the removed LP rows, ascending
    const int *raw_ptr, *raw_col; const double *raw_val, *raw_lhs, *raw_rhs;      // the raw rows as they are
    int *out_ptr, *out_col; double *out_val, *out_lhs, *out_rhs;                  // the raw rows without the removed ones
    int R0, N0, C0, E0;                         // resident: rows, raw entries, state rows, state edges
    int R1, N1, C1, E1, L1, EL1;                // after the removal, as the host counted it (L1 / EL1: lhs rows and their entries)
    int V, nvc, nrc;                            // variables, their 256-chunks, the 256-chunks of the resident LP rows
    int nb_var, nb_edges, nb_raw;               // k_lpd_vars's blocks: lane groups of variables | old by-left edges | old raw entries
    int* part_a;              // [nrc][4] per chunk: kept rows, kept raw entries, -, -
    int* part_b;              // [nrc][4] per chunk: kept lhs state rows, their edges, kept rhs state rows, their edges
    int* vcnt;                // [V]   removed entries per variable        } cleared before k_lpd_mark
    int* vpart;               // [nvc] removed entries per variable chunk  }
    int* row_map;             // [C0]  old state row -> new state row, -1 for a removed one
    int* row_new;             // [R0]  old LP row -> new LP row, -1 for a removed one
    int* flags_out;
};

// the first position of the ascending list whose row is not below r
__device__ __forceinline__ int lpd_lower(const int* list, int n, int r) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < r) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ bool lpd_removed(const int* list, int n, int r) {
    const int lo = lpd_lower(list, n, r);
    return lo < n && list[lo] == r;
}

// what the launches know of resident LP row r: its raw range and its two state rows (-1: that side is not listed)
struct LpdRow { int beg, end, p0, p1; };
__device__ __forceinline__ LpdRow lpd_row(const LpdArgs& x, int r) {
    LpdRow w; bool bad;
    lp_row_range(x.raw_ptr, r, x.N0, w.beg, w.end, bad);
    w.p0 = x.src.row_place[2 * (size_t)r]; w.p1 = x.src.row_place[2 * (size_t)r + 1];
    if (!lp_in(w.p0, x.C0)) w.p0 = -1;
    if (!lp_in(w.p1, x.C0)) w.p1 = -1;
    return w;
}

__device__ __forceinline__ void lpd_mark_body(const LpdArgs& x, const int blk) {
    __shared__ int s_cnt[8];
    const int t = threadIdx.x;
    if (t < 8) s_cnt[t] = 0;
    __syncthreads();
    const int r = blk * LP_NT + t;
    if (r < x.R0 && !lpd_removed(x.list, x.n_list, r)) {
        const LpdRow w = lpd_row(x, r);
        const int len = w.end - w.beg;
        atomicAdd(&s_cnt[0], 1);                               // integers in LDS
        if (len) atomicAdd(&s_cnt[1], len);
        if (w.p0 >= 0) { atomicAdd(&s_cnt[4], 1); if (len) atomicAdd(&s_cnt[5], len); }
        if (w.p1 >= 0) { atomicAdd(&s_cnt[6], 1); if (len) atomicAdd(&s_cnt[7], len); }
    }
    __syncthreads();
    if (t < 4) { x.part_a[4 * (size_t)blk + t] = s_cnt[t]; x.part_b[4 * (size_t)blk + t] = s_cnt[4 + t]; }
    // the removed rows of this chunk: a range of the list, LP_SUB lanes a row
    const int row_end = (int)min((long long)(blk + 1) * LP_NT, (long long)x.R0);
    const int first = lpd_lower(x.list, x.n_list, blk * LP_NT), last = lpd_lower(x.list, x.n_list, row_end);
    const int g = t / LP_SUB, l = t % LP_SUB;
    for (int k = first + g; k < last; k += LP_NT / LP_SUB) {
        const int rr = x.list[k];
        if (!lp_in(rr, x.R0)) continue;
        const LpdRow w = lpd_row(x, rr);
        const int sides = (int)(w.p0 >= 0) + (int)(w.p1 >= 0);
        if (!sides) continue;
        for (int e = w.beg + l; e < w.end; e += LP_SUB) {
            const int c = x.raw_col[e];
            if (!lp_in(c, x.V)) continue;
            atomicAdd(&x.vcnt[c], sides);
            atomicAdd(&x.vpart[c / LP_NT], sides);
        }
    }
}

__global__ __launch_bounds__(LP_NT) void k_lpd_mark(LpdArgs x) { lpd_mark_body(x, blockIdx.x); }

__device__ __forceinline__ void lpd_rows_body(const LpdArgs& x, const int blk) {
    __shared__ int si[4 * LP_NT];
    __shared__ int s_front;
    const int t = threadIdx.x;
    if (blk > x.nrc) {                                         // ---- variable blocks: the new v_ptr
        const int b = blk - x.nrc - 1;
        const int j = b * LP_NT + t;
        int n = 0;
        if (j < x.V) n = x.vcnt[j];
        int p = 0;
        for (int i = t; i < b && i < x.nvc; i += LP_NT) p += x.vpart[i];
        if (t == 0) s_front = 0;
        __syncthreads();
        if (p) atomicAdd(&s_front, p);                         // integers in LDS
        __syncthreads();
        const int front = s_front;
        const int v[4] = {n, 0, 0, 0};
        int ex[4], bt[4];
        lp_block_scan4(v, ex, bt, si);
        if (j <= x.V) x.dst.v_ptr[j] = lpa_clamp(lpa_clamp(x.src.v_ptr[j], x.E0) - front - ex[0], x.E1);
        return;
    }
    int pa[4], ta[4], pb[4], tb[4];
    lp_chunk_prefix(x.part_a, x.nrc, blk, pa, ta, si);
    lp_chunk_prefix(x.part_b, x.nrc, blk, pb, tb, si);
    if (blk == x.nrc) {                                        // ---- the totals against the host's, and the flag words
        if (t < 4) {
            int w = 0;
            if (t == LP_F_SIZES && (ta[0] != x.R1 || ta[1] != x.N1 || tb[0] != x.L1 || tb[1] != x.EL1 || tb[0] + tb[2] != x.C1 ||
                                    tb[1] + tb[3] != x.E1))
                w = 1;
            x.flags_out[t] = w;
        }
        if (t == 0) { x.dst.l_ptr[x.C1] = x.E1; x.out_ptr[x.R1] = x.N1; }
        return;
    }
    const int r = blk * LP_NT + t;                             // ---- row blocks: everything by row at its final place
    LpdRow w = {0, 0, -1, -1};
    bool keep = false;
    if (r < x.R0) { w = lpd_row(x, r); keep = !lpd_removed(x.list, x.n_list, r); }
    const int len = w.end - w.beg;
    const bool kl = keep && w.p0 >= 0, kr = keep && w.p1 >= 0;
    const int va[4] = {keep, keep ? len : 0, kl, kl ? len : 0};
    const int vb[4] = {kr, kr ? len : 0, 0, 0};
    int ea[4], eb[4], bt[4];
    lp_block_scan4(va, ea, bt, si);
    lp_block_scan4(vb, eb, bt, si);
    if (r >= x.R0) return;
    const int new_r = pa[0] + ea[0], new_e = pa[1] + ea[1];
    const int pos_l = pb[0] + ea[2], ofs_l = pb[1] + ea[3];
    const int pos_r = tb[0] + pb[2] + eb[0], ofs_r = tb[1] + pb[3] + eb[1];
    x.row_new[r] = keep && lp_in(new_r, x.R1) ? new_r : -1;
    if (w.p0 >= 0) x.row_map[w.p0] = kl && lp_in(pos_l, x.C1) ? pos_l : -1;
    if (w.p1 >= 0) x.row_map[w.p1] = kr && lp_in(pos_r, x.C1) ? pos_r : -1;
    if (keep && lp_in(new_r, x.R1)) {
        x.dst.row_place[2 * (size_t)new_r] = kl ? pos_l : -1; x.dst.row_place[2 * (size_t)new_r + 1] = kr ? pos_r : -1;
        x.dst.row_scale[new_r] = x.src.row_scale[r];
        x.out_ptr[new_r] = lpa_clamp(new_e, x.N1); x.out_lhs[new_r] = x.raw_lhs[r]; x.out_rhs[new_r] = x.raw_rhs[r];
    }
    if (kl && lp_in(pos_l, x.C1)) {
        ((float4*)x.dst.cons_feats)[pos_l] = ((const float4*)x.src.cons_feats)[w.p0];
        x.dst.l_ptr[pos_l] = lpa_clamp(ofs_l, x.E1);
    }
    if (kr && lp_in(pos_r, x.C1)) {
        ((float4*)x.dst.cons_feats)[pos_r] = ((const float4*)x.src.cons_feats)[w.p1];
        x.dst.l_ptr[pos_r] = lpa_clamp(ofs_r, x.E1);
    }
}

__global__ __launch_bounds__(LP_NT) void k_lpd_rows(LpdArgs x) { lpd_rows_body(x, blockIdx.x); }

__device__ __forceinline__ void lpd_vars_body(const LpdArgs& x, int b) {
    const int t = threadIdx.x;
    if (b < x.nb_var) {                                        // ---- variables: LP_SUB lanes each, the segment compacted in order
        const int v = b * (LP_NT / LP_SUB) + t / LP_SUB, l = t % LP_SUB;
        if (v >= x.V) return;
        const int group_shift = (t & 63) & ~(LP_SUB - 1);      // where the lane group's bits start in a 64-bit ballot
        const int beg = lpa_clamp(x.src.v_ptr[v], x.E0), end = max(lpa_clamp(x.src.v_ptr[v + 1], x.E0), beg);
        int at = x.dst.v_ptr[v];
        for (int base = beg; base < end; base += LP_SUB) {
            const int i = base + l;
            int to_row = -1;
            if (i < end) {
                const int row = x.src.v_oth[i];
                if (lp_in(row, x.C0)) to_row = x.row_map[row];
            }
            const bool keep = lp_in(to_row, x.C1);
            const unsigned mask = (unsigned)(__ballot(keep) >> group_shift) & ((1u << LP_SUB) - 1u);
            const int to = at + __popc(mask & ((1u << l) - 1u));
            if (keep && lp_in(to, x.E1)) { x.dst.v_oth[to] = to_row; x.dst.v_coef[to] = x.src.v_coef[i]; }
            at += __popc(mask);
        }
        return;
    }
    b -= x.nb_var;
    if (b < x.nb_edges) {                                      // ---- old by-left edges: a kept one to its new row's offset
        const int i = b * LP_NT + t;
        if (i >= x.E0) return;
        const int p = x.src.e_row[i];
        if (!lp_in(p, x.C0)) return;
        const int q = x.row_map[p];
        if (!lp_in(q, x.C1)) return;
        const int k = i - x.src.l_ptr[p], to = x.dst.l_ptr[q] + k;
        if (k >= 0 && lp_in(to, x.E1)) { x.dst.e_row[to] = q; x.dst.e_col[to] = x.src.e_col[i]; x.dst.e_coef[to] = x.src.e_coef[i]; }
        return;
    }
    b -= x.nb_edges;
    const int e = b * LP_NT + t;                               // ---- old raw entries
    if (e >= x.N0) return;
    int lo = 1, hi = x.R0;                                     // the entry's row: the first j with row_ptr[j] > e, less one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x.raw_ptr[mid] > e) hi = mid; else lo = mid + 1;
    }
    const int r = lo - 1;
    if (!lp_in(r, x.R0)) return;
    const int q = x.row_new[r];
    if (!lp_in(q, x.R1)) return;
    const int k = e - x.raw_ptr[r], to = x.out_ptr[q] + k;
    if (k >= 0 && lp_in(to, x.N1)) { x.out_col[to] = x.raw_col[e]; x.out_val[to] = x.raw_val[e]; }
}
__global__ __launch_bounds__(LP_NT) void k_lpd_vars(LpdArgs x) { lpd_vars_body(x, blockIdx.x); }
