// gcnn_lprounds.hpp -- host side of gcnn_lp_rounds (include/gcnn_hip.h): the rounds of 1..GCNN_LP_ROUNDS_MAX resident LPs, each with
// or without an append, in one call.  Included at the end of gcnn_capi.hip behind gcnn_lpappend.hpp and gcnn_group.hpp: a member's
// work is the unchanged solo code (lpa_enqueue, lpr_run with forward_impl and the tail inside) run with a recorder installed
// (k_group.hpp), and the launch tables and launches are gcnn_group.hpp's (group_tables, group_launches).  What this file adds is the
// call's own layout, the checks across members, the two phases (appends in front, so that the rounds share their stages whether or
// not a member appends) and the twins of the LP launches (k_lprounds.hpp).  Kept apart so that its launch names form their own
// inventory (tests/test_lprounds_build.py).
#include "k_lprounds.hpp"

static_assert(GCNN_LP_ROUNDS_MAX == GCNN_GROUP_MAX, "include/gcnn_hip.h");
static_assert(sizeof(GPair<LpArgs, LpaArgs>) <= GROUP_REC_BYTES && sizeof(GPair<LpArgs, LprArgs>) <= GROUP_REC_BYTES &&
              sizeof(GPair<LpArgs, LpEmitMore>) <= GROUP_REC_BYTES && sizeof(SelArgs) <= GROUP_REC_BYTES, "k_group.hpp: GROUP_REC_BYTES");

#define LPRS_APPEND_STAGES 4      // launches of one member's append
#define LPRS_STAGES (GCNN_GROUP_MAX_STAGES + LPRS_APPEND_STAGES)

// the LP launches a member's call records, and their twins; every other kernel is the forward pass's (g_group_kernels)
static GroupKernel g_lprounds_kernels[] = {
    {(const void*)k_lpa_stats, (const void*)k_lprs_append_stats, "k_lprs_append_stats", {}},
    {(const void*)k_lpa_scan, (const void*)k_lprs_append_scan, "k_lprs_append_scan", {}},
    {(const void*)k_lpa_move, (const void*)k_lprs_append_move, "k_lprs_append_move", {}},
    {(const void*)k_lpa_order, (const void*)k_lprs_append_order, "k_lprs_append_order", {}},
    {(const void*)k_lpr_stats, (const void*)k_lprs_round_stats, "k_lprs_round_stats", {}},
    {(const void*)k_lpr_emit, (const void*)k_lprs_round_emit, "k_lprs_round_emit", {}},
    {(const void*)k_rank_scores, (const void*)k_lprs_rank_scores, "k_lprs_rank_scores", {}},
    {(const void*)k_sel_pairs, (const void*)k_lprs_sel_pairs, "k_lprs_sel_pairs", {}},
    {(const void*)k_sel_filter, (const void*)k_lprs_sel_filter, "k_lprs_sel_filter", {}},
};
static GroupKernel* lprounds_kernel(const void* solo) {
    for (GroupKernel& g : g_lprounds_kernels) if (g.solo == solo) return &g;
    return group_kernel(solo);
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline size_t lprounds_table_bytes(int n) {
    return (size_t)n * LPRS_STAGES * (sizeof(GroupHead) + ((al16(GROUP_REC_BYTES) + 63) & ~(size_t)63));
}

// one member as the call sees it: the dims its round runs on, its solo layouts, and where its pieces lie in the call's arena
struct LprsMember {
    bool app, degenerate;
    gcnn_lp_dims after;
    gcnn_lp_append_layout AL;      // app
    gcnn_lp_round_layout RL;       // relative to the member's round upload, its download block and its round arena
    size_t in_bytes, out_bytes, arena_bytes, counts_bytes;
};

static int lprounds_member(const gcnn_lp_rounds_member& m, int mode, LprsMember* M) {
    const bool select = mode == GCNN_IBATCH_SELECT;
    if (m.has_append < 0 || m.has_append > 1 || (select ? m.n_forced < 0 : m.n_forced != -1)) return GCNN_E_BADARG;
    memset(M, 0, sizeof(*M));
    M->app = m.has_append != 0;
    int rc;
    if (M->app) {
        if ((rc = lpa_layout(&m.dims, &m.block, m.present, m.n_forced, m.n_forced_entries, &M->AL))) return rc;
        if (!lpa_dims_after(&m.dims, &m.block, &M->after)) return GCNN_E_BADARG;
        M->RL = M->AL.round;
        M->in_bytes = M->AL.in_bytes; M->out_bytes = M->AL.out_bytes; M->arena_bytes = M->AL.arena_bytes;
        M->counts_bytes = al16(lpa_scratch(&m.dims, &m.block).clear_bytes);
    } else {
        if ((rc = lpr_round_layout(&m.dims, m.present, m.n_forced, m.n_forced_entries, &M->RL))) return rc;
        M->after = m.dims;
        M->in_bytes = M->RL.in_bytes; M->out_bytes = M->RL.out_bytes; M->arena_bytes = M->RL.arena_bytes;
    }
    if (mode != GCNN_IBATCH_SCORES && M->after.n_cuts > 4096) return GCNN_E_UNSUPPORTED;
    M->degenerate = group_degenerate(lp_state_dims(&M->after));
    return 0;
}

static int lprounds_layout(int n, const gcnn_lp_rounds_member* mem, int mode, gcnn_lp_rounds_layout* L, LprsMember* M) {
    if (n < 1 || n > GCNN_LP_ROUNDS_MAX || !mem || !L || mode < GCNN_IBATCH_SCORES || mode > GCNN_IBATCH_SELECT) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    L->n = n; L->mode = mode;
    int rc;
    for (int i = 0; i < n; ++i) if ((rc = lprounds_member(mem[i], mode, &M[i]))) return rc;
    Carver c{0};
    for (int i = 0; i < n; ++i) { L->in_size[i] = al256(M[i].in_bytes); L->in_off[i] = c.take(L->in_size[i], 256); }
    L->in_bytes = c.off;
    for (int i = 0; i < n; ++i) {
        L->arena_off[i] = c.take(M[i].arena_bytes, 256);
        L->member_round_off[i] = L->arena_off[i] + (M[i].app ? M[i].AL.round_off : 0);
        L->scratch_off[i] = M[i].app ? L->arena_off[i] + M[i].AL.scratch_off : 0;
    }
    L->counts_base = c.off;
    for (int i = 0; i < n; ++i) L->counts_off[i] = M[i].app ? c.take(M[i].counts_bytes, 16) : 0;
    L->counts_bytes = c.off - L->counts_base;
    c.off = al256(c.off);
    L->out_base = c.off;
    for (int i = 0; i < n; ++i) { L->out_size[i] = al16(M[i].out_bytes); L->out_off[i] = c.take(L->out_size[i], 16) - L->out_base; }
    L->out_bytes = c.off - L->out_base;
    c.off = al256(c.off);
    L->table_bytes = lprounds_table_bytes(n);
    L->table_off = c.take(L->table_bytes, 256);
    L->arena_bytes = c.off;
    return 0;
}

extern "C" int gcnn_lp_rounds_layout_for(int32_t n, const gcnn_lp_rounds_member* members, int32_t mode, gcnn_lp_rounds_layout* layout) {
    LprsMember M[GCNN_LP_ROUNDS_MAX];
    return lprounds_layout(n, members, mode, layout, M);
}

// group_check's rule on resident LPs: what a member's launches write must not overlap anything another member's launches touch
struct LprsSpan { const void* p; size_t bytes; };
static void lprounds_spans(const gcnn_lp_rounds_member& m, const LprsMember& M, std::vector<LprsSpan>& wr, std::vector<LprsSpan>& rd) {
    const gcnn_lp_dims &a = M.after, &b = m.dims;
    const size_t R = a.n_rows, V = a.n_cols, C = a.n_state_rows, E = a.n_state_edges, N = a.row_nnz;
    const gcnn_lp_resident& r = *m.resident;
    const gcnn_graph& g = r.cons_graph;
    wr = {{r.cons_feats, 16 * C}, {r.col_lb, 8 * V}, {r.col_ub, 8 * V}, {r.col_primal, 8 * V}, {r.col_primal_avg, 8 * V}};
    rd = {{m.params, (size_t)g_ptotal * sizeof(float)}, {r.row_place, 8 * R}, {r.row_scale, 8 * R}, {r.col_type, V}, {r.col_obj, 8 * V},
          {g.l_ptr, 4 * (C + 1)}, {g.l_oth, 4 * E}, {g.l_coef, 4 * E}, {g.v_ptr, 4 * (V + 1)}, {g.v_oth, 4 * E}, {g.v_coef, 4 * E}};
    if (!M.app) return;
    const gcnn_lp_rows_set& d = *m.dst;
    wr.insert(wr.end(), {{d.cons_feats, 16 * C}, {d.edge_row, 4 * E}, {d.edge_col, 4 * E}, {d.edge_coef, 4 * E}, {d.l_ptr, 4 * (C + 1)},
                         {d.v_ptr, 4 * (V + 1)}, {d.v_oth, 4 * E}, {d.v_coef, 4 * E}, {d.row_place, 8 * R}, {d.row_scale, 8 * R},
                         {m.row_ptr, 4 * (R + 1)}, {m.row_col, 4 * N}, {m.row_val, 8 * N}, {m.row_lhs, 8 * R}, {m.row_rhs, 8 * R}});
    const gcnn_lp_rows_set& s = *m.src;
    const size_t R0 = b.n_rows, C0 = b.n_state_rows, E0 = b.n_state_edges;
    rd.insert(rd.end(), {{s.cons_feats, 16 * C0}, {s.edge_row, 4 * E0}, {s.edge_col, 4 * E0}, {s.edge_coef, 4 * E0}, {s.l_ptr, 4 * (C0 + 1)},
                         {s.v_ptr, 4 * (V + 1)}, {s.v_oth, 4 * E0}, {s.v_coef, 4 * E0}, {s.row_place, 8 * R0}, {s.row_scale, 8 * R0}});
}
static bool lprounds_overlap(int n, const gcnn_lp_rounds_member* mem, const LprsMember* M) {
    std::vector<LprsSpan> wr[GCNN_LP_ROUNDS_MAX], rd[GCNN_LP_ROUNDS_MAX];
    for (int i = 0; i < n; ++i) lprounds_spans(mem[i], M[i], wr[i], rd[i]);
    auto hit = [](const LprsSpan& a, const LprsSpan& b) {
        if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
        const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
        return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
    };
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (i == j) continue;
            for (const LprsSpan& a : wr[i]) {
                for (const LprsSpan& b : wr[j]) if (hit(a, b)) return true;
                for (const LprsSpan& b : rd[j]) if (hit(a, b)) return true;
            }
        }
    return false;
}

struct LprsPlan { GroupLaunch launches[GCNN_LP_ROUNDS_MAX * LPRS_STAGES]; int nl; size_t bytes; };

extern "C" int gcnn_lp_rounds(int32_t n, const gcnn_lp_rounds_member* mem, int32_t mode, const void* host_in, void* host_out, void* arena,
                              size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream) {
    gcnn_lp_rounds_layout L;
    static thread_local LprsMember M[GCNN_LP_ROUNDS_MAX];
    int rc = lprounds_layout(n, mem, mode, &L, M);
    if (rc) return rc;
    const bool select = mode == GCNN_IBATCH_SELECT;
    const int want = mode != GCNN_IBATCH_SCORES;
    if (!host_in || !host_out || !host_staging || ((uintptr_t)host_staging & 15) || !arena || ((uintptr_t)arena & 255) ||
        arena_bytes < L.arena_bytes)
        return GCNN_E_BADARG;
    if (select && !finite_thresholds(p_max, p_max_ub)) return GCNN_E_BADARG;
    layout_init();
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    // 1. everything the solo calls check, member by member, then the members against each other
    for (int i = 0; i < n; ++i) {
        const gcnn_lp_rounds_member& m = mem[i];
        if (!m.resident) return GCNN_E_BADARG;
        gcnn_lp_dims after;
        if (M[i].app && (rc = lpa_check(&m.dims, &m.block, &after, m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs, m.resident->col_obj,
                                        m.src, m.dst)))
            return rc;
        gcnn_lp_round_layout RL;
        if ((rc = lpr_check(&M[i].after, m.present, m.n_forced, m.n_forced_entries, m.resident, m.params, host_in, host_out,
                            A + L.member_round_off[i], M[i].RL.arena_bytes, want, p_max, p_max_ub, M[i].app ? 16 : 0, &RL)))
            return rc;
    }
    if (lprounds_overlap(n, mem, M)) return GCNN_E_BADARG;
    // 2. record: the appends, then the rounds of the regular members (nothing is enqueued)
    static thread_local std::vector<GroupRecord> recs;
    recs.resize((size_t)GCNN_LP_ROUNDS_MAX * LPRS_STAGES);
    GroupRecorder ra[GCNN_LP_ROUNDS_MAX], rr[GCNN_LP_ROUNDS_MAX];
    int napp = 0, nreg = 0;
    auto at_of = [&](int i) { return LprAt{A + L.in_off[i] + (M[i].app ? M[i].AL.block_bytes : 0), A + L.out_base + L.out_off[i]}; };
    auto round_of = [&](int i, const LprAt& at) {
        const gcnn_lp_rounds_member& m = mem[i];
        return lpr_run(&M[i].after, M[i].RL, m.present, m.n_forced, m.resident, m.params, nullptr, nullptr, A + L.member_round_off[i], want, p_max,
                       p_max_ub, stream, &at);
    };
    for (int i = 0; i < n; ++i) {
        const gcnn_lp_rounds_member& m = mem[i];
        GroupRecord* slot = recs.data() + (size_t)i * LPRS_STAGES;
        const LprAt at = at_of(i);
        if (M[i].app) {
            GroupRecorder& q = ra[napp++];
            q = GroupRecorder{slot, 0, LPRS_APPEND_STAGES, false};
            const gcnn_lp_append_layout& AL = M[i].AL;
            const char* blk = A + L.in_off[i];
            int32_t* const raw[2] = {m.row_ptr, m.row_col};
            double* const rawd[3] = {m.row_val, m.row_lhs, m.row_rhs};
            GroupRecScope scope(&q);
            if ((rc = lpa_enqueue(&m.dims, &m.block, (const int*)(blk + AL.block_off[0]), (const int*)(blk + AL.block_off[1]),
                                  (const double*)(blk + AL.block_off[2]), (const double*)(blk + AL.block_off[3]),
                                  (const double*)(blk + AL.block_off[4]), m.block.row_nnz, 0, raw, rawd, m.resident->col_obj, m.src, m.dst,
                                  A + L.scratch_off[i], (int32_t*)(at.out + AL.flags_off), st, A + L.counts_off[i])))
                return rc;
        }
        if (M[i].degenerate) continue;
        GroupRecorder& q = rr[nreg++];
        q = GroupRecorder{slot + LPRS_APPEND_STAGES, 0, GCNN_GROUP_MAX_STAGES, false};
        GroupRecScope scope(&q);
        if ((rc = round_of(i, at))) return rc;
    }
    // 3. the launch tables of both phases in the staging buffer
    static thread_local LprsPlan plan;
    plan.nl = 0; plan.bytes = 0;
    const int cap = GCNN_LP_ROUNDS_MAX * LPRS_STAGES;
    if ((rc = group_tables(napp, ra, host_staging, lprounds_kernel, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if ((rc = group_tables(nreg, rr, host_staging, lprounds_kernel, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if (plan.bytes > L.table_bytes) return GCNN_E_WORKSPACE;
    // 4. ONE upload of all rounds and blocks, one of the tables, at most ONE fill, the launches, ONE download
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));
    if (plan.bytes) HIPCHK(hipMemcpyAsync(A + L.table_off, host_staging, plan.bytes, hipMemcpyHostToDevice, st));
    if (L.counts_bytes) HIPCHK(hipMemsetAsync(A + L.counts_base, 0, L.counts_bytes, st));
    if ((rc = group_launches(plan.launches, plan.nl, A + L.table_off, st))) return rc;
    for (int i = 0; i < n; ++i)
        if (M[i].degenerate && (rc = round_of(i, at_of(i)))) return rc;      // its solo launches, on the call's addresses
    HIPCHK(hipMemcpyAsync(host_out, A + L.out_base, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
