// k_lpappend.hpp -- rows appended to a resident LP (k_lpres.hpp) without deriving the resident rows again (include/gcnn_hip.h:
// gcnn_lp_rows_append, gcnn_lp_round_append).  Everything the state holds of a row is local to that row but its place: the state
// lists the lhs sides first, so a block with dL lhs rows and dEL lhs entries moves every rhs row.  With L0 / EL0 resident lhs rows
// / entries the new state is
//   rows          [ old lhs (L0) | new lhs (dL) | old rhs, ids + dL | new rhs ]
//   by-left edges [ old lhs (EL0) | new lhs (dEL) | old rhs, at + dEL, row id + dL | new rhs ]
//   by-variable   per variable [ old entries of rows < L0 | new lhs entries | old entries of rows >= L0, row id + dL | new rhs entries ],
//                 new entries ascending by row (the stable order gcnn_graph_build gives)
// Old values are copied, shifted and merged, never recomputed; the new rows' sums go through lp_stats_body and their values
// through the expressions of lp_emit_body (k_lpstate.hpp), so the result has the bits of the rebuild.  Everything is written out
// of place: the launches read one set of derived arrays (LpaSet) and write the other, so no block depends on what another has
// already overwritten and a rejected block leaves the resident set as it was.  Four launches behind one fill of the count tables:
//   k_lpa_stats  a block per 256 new rows: lp_stats_body's row half (row_stat, the chunk's side and entry counts, the flag bits),
//                then per entry of a listed side a returning integer atomic on the variable's counter (cnt [V][2]) -- the entry's
//                arrival rank -- and one on the counter of the variable's 256-chunk (vpart).  In the fused call the blocks also copy
//                the block's five raw arrays from the upload slot behind the resident raw rows.
//   k_lpa_scan   a block per 256 variables: new v_ptr = old v_ptr + exclusive scan of the counts (the chunk counters in front are
//                summed as lp_chunk_prefix does), and the split of the variable's old segment at row id L0 (rows ascend within
//                a segment: a binary search).
//   k_lpa_move   new-row blocks: the rows' features, places, scales, by-left offsets and edges at their final places, their
//                by-variable entries in arrival order into a staging list; copy blocks: the old cons_feats, l_ptr, by-left and
//                by-variable entries (its variable by binary search over the old v_ptr), row_place and row_scale, shifted; one
//                block compares the block's totals with the host's and publishes the four flag words.
//   k_lpa_order  16 lanes a variable: its staged new entries to their final places, each at the rank of its row id.  It cannot
//                ride in k_lpa_move: an entry's rank depends on entries other blocks stage.
// No float atomics; every store is bounds-checked against the sizes the host computed; no scratch memory, under 16 KiB of LDS.
#pragma once

struct LpaSet {               // one set of what is derived from the rows (device)
    float* cons_feats;        // [C][4]
    int* e_row; int* e_col; float* e_coef;      // [E] each: the constraint edges by left node (e_col, e_coef: also the graph's l_oth, l_coef)
    int* l_ptr; int* v_ptr; int* v_oth; float* v_coef;
    int* row_place; double* row_scale;          // [R][2], [R]
};

struct LpaArgs {
    LpaSet src, dst;
    int R0, N0, C0, E0, L0, EL0;                // resident: rows, raw entries, state rows, state edges, lhs rows and their entries
    int dR, dN, dC, dE, dL, dEL;                // the block, as the host counted it
    int V, nvc;                                 // variables and their 256-chunks
    int ent_base;                               // index of the block's first entry in LpArgs.row_col (0: the upload slot; N0: the raw rows)
    int *raw_ptr, *raw_col; double *raw_val, *raw_lhs, *raw_rhs;     // the fused call: where the block is copied to (null: it is there)
    int* cnt;                 // [V][2] new lhs / rhs entries per variable  } cleared before k_lpa_stats
    int* vpart;               // [nvc]  new entries per variable chunk       }
    int* vsplit;              // [V]    old entries of rows < L0
    int* ent_rank;            // [dN][2] arrival rank of the entry's lhs / rhs copy within its variable
    int* tmp_row; float* tmp_coef;              // [dE] the new by-variable entries, per variable lhs then rhs, in arrival order
    int nb_new, nb_rows, nb_edges, nb_lprows;   // k_lpa_move's blocks: new rows | old state rows | old edges | old LP rows (then the flag block)
    int* flags_out;
};

__device__ __forceinline__ int lpa_clamp(int x, int n) { return min(max(x, 0), n); }

// Each launch's work as a body over the block index: the solo kernels run it with blockIdx.x, a launch of several sessions' appends
// (k_lprounds.hpp) with the member's own block index.
__device__ __forceinline__ void lpa_stats_body(const LpArgs& a, const LpaArgs& x, const int blk) {
    const int t = threadIdx.x;
    lp_stats_body(a, blk);
    const int g = t / LP_SUB, l = t % LP_SUB;
    for (int it = 0; it < LP_SUB; ++it) {
        const int r = blk * LP_NT + it * (LP_NT / LP_SUB) + g;
        if (r >= x.dR) continue;
        int beg, end; bool bad;
        lp_row_range(a.row_ptr, r, a.nnz_r, beg, end, bad);
        const double lo = a.row_lhs[r], hi = a.row_rhs[r];
        const bool has_l = lp_finite(lo, a.infinity), has_r = lp_finite(hi, a.infinity);
        if (x.raw_ptr && l == 0) {
            x.raw_ptr[x.R0 + 1 + r] = a.row_ptr[r + 1] - x.ent_base + x.N0;
            x.raw_lhs[x.R0 + r] = lo; x.raw_rhs[x.R0 + r] = hi;
        }
        for (int e = beg + l; e < end; e += LP_SUB) {
            const int rel = e - x.ent_base;
            if (!lp_in(rel, x.dN)) continue;
            const int c = a.row_col[e];
            if (x.raw_ptr) { x.raw_col[x.N0 + rel] = c; x.raw_val[x.N0 + rel] = a.row_val[e]; }
            if (!lp_in(c, x.V) || !(has_l || has_r)) continue;
            if (has_l) x.ent_rank[2 * (size_t)rel] = atomicAdd(&x.cnt[2 * (size_t)c], 1);
            if (has_r) x.ent_rank[2 * (size_t)rel + 1] = atomicAdd(&x.cnt[2 * (size_t)c + 1], 1);
            atomicAdd(&x.vpart[c / LP_NT], (int)has_l + (int)has_r);
        }
    }
}

__global__ __launch_bounds__(LP_NT) void k_lpa_stats(LpArgs a, LpaArgs x) { lpa_stats_body(a, x, blockIdx.x); }

__device__ __forceinline__ void lpa_scan_body(const LpaArgs& x, const int b) {
    __shared__ int si[4 * LP_NT];
    __shared__ int s_front;
    const int t = threadIdx.x;
    const int j = b * LP_NT + t;
    int n = 0;
    if (j < x.V) n = x.cnt[2 * (size_t)j] + x.cnt[2 * (size_t)j + 1];
    int p = 0;
    for (int i = t; i < b && i < x.nvc; i += LP_NT) p += x.vpart[i];
    if (t == 0) s_front = 0;
    __syncthreads();
    if (p) atomicAdd(&s_front, p);                             // integers in LDS
    __syncthreads();
    const int front = s_front;
    const int v[4] = {n, 0, 0, 0};
    int ex[4], bt[4];
    lp_block_scan4(v, ex, bt, si);
    if (j > x.V) return;
    const int ob = lpa_clamp(x.src.v_ptr[j], x.E0);
    x.dst.v_ptr[j] = lpa_clamp(ob + front + ex[0], x.E0 + x.dE);
    if (j == x.V) return;
    const int oe = max(lpa_clamp(x.src.v_ptr[j + 1], x.E0), ob);
    int lo = ob, hi = oe;                                      // first entry of the segment whose row is not an lhs row
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x.src.v_oth[mid] >= x.L0) hi = mid; else lo = mid + 1;
    }
    x.vsplit[j] = lo - ob;
}
__global__ __launch_bounds__(LP_NT) void k_lpa_scan(LpaArgs x) { lpa_scan_body(x, blockIdx.x); }

// The new rows of chunk b at their final places: lp_emit_body's row half (resident form: the solve-dependent half zero) with the
// resident counts in front, plus what gcnn_graph_build derives from it -- the by-left offsets, and the by-variable entries (staged).
__device__ __forceinline__ void lpa_emit_body(const LpArgs& a, const LpaArgs& x, const int b) {
    __shared__ int si[4 * LP_NT];
    __shared__ double sd[LP_NT];
    __shared__ int s_pos[LP_NT], s_ofs[2][LP_NT], s_pos2[LP_NT];
    const int t = threadIdx.x;
    const int C1 = x.C0 + x.dC, E1 = x.E0 + x.dE, R1 = x.R0 + x.dR;
    int pre[4], tot[4];
    lp_chunk_prefix(a.row_part, a.nrc, b, pre, tot, si);
    const int r = b * LP_NT + t;
    int beg = 0, end = 0; bool bad = false;
    bool has_l = false, has_r = false;
    double lo = 0.0, hi = 0.0;
    if (r < x.dR) {
        lp_row_range(a.row_ptr, r, a.nnz_r, beg, end, bad);
        lo = a.row_lhs[r]; hi = a.row_rhs[r];
        has_l = lp_finite(lo, a.infinity); has_r = lp_finite(hi, a.infinity);
    }
    const int len = end - beg;
    const int v[4] = {has_l, has_l ? len : 0, has_r, has_r ? len : 0};
    int ex[4], bt[4];
    lp_block_scan4(v, ex, bt, si);
    const int pos_l = x.L0 + pre[0] + ex[0], ofs_l = x.EL0 + pre[1] + ex[1];
    const int pos_r = tot[0] + x.C0 + pre[2] + ex[2], ofs_r = tot[1] + x.E0 + pre[3] + ex[3];
    double norm = 1.0;
    if (r < x.dR) {
        const double raw = sqrt(a.row_stat[2 * (size_t)r]);
        norm = raw == 0.0 ? 1.0 : raw;
        const double den = norm * a.obj_norm;
        const double cosine = a.row_stat[2 * (size_t)r + 1] / den;
        const double dual = 0.0;
        if (lp_in(x.R0 + r, R1)) {
            x.dst.row_place[2 * (size_t)(x.R0 + r)] = has_l ? pos_l : -1; x.dst.row_place[2 * (size_t)(x.R0 + r) + 1] = has_r ? pos_r : -1;
            x.dst.row_scale[x.R0 + r] = den;
        }
        if (has_l && lp_in(pos_l, C1)) {
            ((float4*)x.dst.cons_feats)[pos_l] = make_float4((float)(-(lo / norm)), 0.f, (float)(-cosine), (float)(-dual));
            x.dst.l_ptr[pos_l] = lpa_clamp(ofs_l, E1);
        }
        if (has_r && lp_in(pos_r, C1)) {
            ((float4*)x.dst.cons_feats)[pos_r] = make_float4((float)(hi / norm), 0.f, (float)cosine, (float)dual);
            x.dst.l_ptr[pos_r] = lpa_clamp(ofs_r, E1);
        }
    }
    __syncthreads();
    s_pos[t] = has_l ? pos_l : -1; s_ofs[0][t] = has_l ? ofs_l : -1;
    s_pos2[t] = has_r ? pos_r : -1; s_ofs[1][t] = has_r ? ofs_r : -1;
    sd[t] = norm;
    __syncthreads();
    const int g = t / LP_SUB, l = t % LP_SUB;
    for (int it = 0; it < LP_SUB; ++it) {
        const int k = it * (LP_NT / LP_SUB) + g, rr = b * LP_NT + k;
        if (rr >= x.dR) continue;
        int rb, re; bool rbad;
        lp_row_range(a.row_ptr, rr, a.nnz_r, rb, re, rbad);
        const double nr = sd[k];
        const int pl = s_pos[k], ol = s_ofs[0][k], pr = s_pos2[k], orr = s_ofs[1][k];
        for (int e = rb + l; e < re; e += LP_SUB) {
            const int c0 = a.row_col[e];
            const bool c_ok = lp_in(c0, x.V);
            const int c = c_ok ? c0 : 0;                       // flagged by k_lpa_stats; keeps every later gather inside its table
            const double xv = a.row_val[e] / nr;
            const int j = e - rb, rel = e - x.ent_base;
            int vb = 0, nl = 0;                                // the variable's staging offset and its new lhs entries
            const bool stage = c_ok && lp_in(rel, x.dN);
            if (stage) { vb = x.dst.v_ptr[c] - lpa_clamp(x.src.v_ptr[c], x.E0); nl = x.cnt[2 * (size_t)c]; }
            if (lp_in(pl, C1) && lp_in(ol + j, E1)) {
                x.dst.e_row[ol + j] = pl; x.dst.e_col[ol + j] = c; x.dst.e_coef[ol + j] = (float)(-xv);
                if (stage) {
                    const int s = vb + x.ent_rank[2 * (size_t)rel];
                    if (lp_in(s, x.dE)) { x.tmp_row[s] = pl; x.tmp_coef[s] = (float)(-xv); }
                }
            }
            if (lp_in(pr, C1) && lp_in(orr + j, E1)) {
                x.dst.e_row[orr + j] = pr; x.dst.e_col[orr + j] = c; x.dst.e_coef[orr + j] = (float)xv;
                if (stage) {
                    const int s = vb + nl + x.ent_rank[2 * (size_t)rel + 1];
                    if (lp_in(s, x.dE)) { x.tmp_row[s] = pr; x.tmp_coef[s] = (float)xv; }
                }
            }
        }
    }
}

__device__ __forceinline__ void lpa_move_body(const LpArgs& a, const LpaArgs& x, int b) {
    const int t = threadIdx.x;
    const int C1 = x.C0 + x.dC, E1 = x.E0 + x.dE;
    if (b < x.nb_new) { lpa_emit_body(a, x, b); return; }
    b -= x.nb_new;
    if (b < x.nb_rows) {                                       // ---- old state rows: features and by-left offsets
        const int i = b * LP_NT + t;
        if (i >= x.C0) return;
        const bool left = i < x.L0;
        const int to = left ? i : i + x.dL;
        if (!lp_in(to, C1)) return;
        ((float4*)x.dst.cons_feats)[to] = ((const float4*)x.src.cons_feats)[i];
        x.dst.l_ptr[to] = lpa_clamp(x.src.l_ptr[i] + (left ? 0 : x.dEL), E1);
        return;
    }
    b -= x.nb_rows;
    if (b < x.nb_edges) {                                      // ---- old edges, in both orders
        const int i = b * LP_NT + t;
        if (i >= x.E0) return;
        {
            const bool left = i < x.EL0;
            const int to = left ? i : i + x.dEL;
            if (lp_in(to, E1)) {
                x.dst.e_row[to] = x.src.e_row[i] + (left ? 0 : x.dL); x.dst.e_col[to] = x.src.e_col[i]; x.dst.e_coef[to] = x.src.e_coef[i];
            }
        }
        int lo = 1, hi = x.V;                                  // the entry's variable: the first j with v_ptr[j] > i, less one
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (x.src.v_ptr[mid] > i) hi = mid; else lo = mid + 1;
        }
        const int v = lo - 1;
        if (!lp_in(v, x.V)) return;
        const int k = i - lpa_clamp(x.src.v_ptr[v], x.E0);
        const bool left = k < x.vsplit[v];
        const int to = x.dst.v_ptr[v] + k + (left ? 0 : x.cnt[2 * (size_t)v]);
        if (k >= 0 && lp_in(to, E1)) { x.dst.v_oth[to] = x.src.v_oth[i] + (left ? 0 : x.dL); x.dst.v_coef[to] = x.src.v_coef[i]; }
        return;
    }
    b -= x.nb_edges;
    if (b < x.nb_lprows) {                                     // ---- old LP rows: places and scales
        const int r = b * LP_NT + t;
        if (r >= x.R0) return;
        const int p1 = x.src.row_place[2 * (size_t)r + 1];
        x.dst.row_place[2 * (size_t)r] = x.src.row_place[2 * (size_t)r];
        x.dst.row_place[2 * (size_t)r + 1] = p1 < 0 ? p1 : p1 + x.dL;
        x.dst.row_scale[r] = x.src.row_scale[r];
        return;
    }
    __shared__ int si[8];                                      // ---- the block's totals against the host's, and the flag words
    int pre[4], tot[4];
    lp_chunk_prefix(a.row_part, a.nrc, 0, pre, tot, si);
    int f = 0;
    for (int i = t; i < a.n_stat_blocks; i += LP_NT) f |= a.blk_flags[i];
    if (t == 0) si[0] = 0;
    __syncthreads();
    if (f) atomicOr(&si[0], f);
    __syncthreads();
    if (t < 4) {
        int w = si[0] >> t & 1;
        if (t == LP_F_SIZES && (tot[0] != x.dL || tot[1] != x.dEL || tot[0] + tot[2] != x.dC || tot[1] + tot[3] != x.dE)) w = 1;
        x.flags_out[t] = w;
    }
    if (t == 0) x.dst.l_ptr[C1] = E1;
}
__global__ __launch_bounds__(LP_NT) void k_lpa_move(LpArgs a, LpaArgs x) { lpa_move_body(a, x, blockIdx.x); }

__device__ __forceinline__ void lpa_order_body(const LpaArgs& x, const int blk) {
    const int t = threadIdx.x;
    const int v = blk * (LP_NT / LP_SUB) + t / LP_SUB, l = t % LP_SUB;
    if (v >= x.V) return;
    const int nl = x.cnt[2 * (size_t)v], nr = x.cnt[2 * (size_t)v + 1];
    if (nl + nr == 0) return;
    const int E1 = x.E0 + x.dE;
    const int ob = lpa_clamp(x.src.v_ptr[v], x.E0), oe = max(lpa_clamp(x.src.v_ptr[v + 1], x.E0), ob);
    const int nb = x.dst.v_ptr[v];
    for (int side = 0; side < 2; ++side) {
        const int n = side ? nr : nl;
        const int tb = nb - ob + (side ? nl : 0);              // in the staging list
        const int fb = nb + (side ? oe - ob + nl : x.vsplit[v]);   // in the new by-variable list
        if (tb < 0 || n < 0 || tb > x.dE - n) continue;
        for (int i = l; i < n; i += LP_SUB) {
            const int row = x.tmp_row[tb + i];
            int rank = 0;
            for (int k = 0; k < n; ++k) { const int o = x.tmp_row[tb + k]; rank += o < row || (o == row && k < i); }
            if (lp_in(fb + rank, E1)) { x.dst.v_oth[fb + rank] = row; x.dst.v_coef[fb + rank] = x.tmp_coef[tb + i]; }
        }
    }
}
__global__ __launch_bounds__(LP_NT) void k_lpa_order(LpaArgs x) { lpa_order_body(x, blockIdx.x); }
