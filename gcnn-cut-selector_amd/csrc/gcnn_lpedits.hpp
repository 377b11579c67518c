// gcnn_lpedits.hpp -- host side of gcnn_lp_rounds_edit (include/gcnn_hip.h): gcnn_lp_rounds with an optional removal per member.
// Included at the end of gcnn_capi.hip behind gcnn_lpremove.hpp and gcnn_lprounds.hpp: a member's work is the unchanged solo code
// (lpd_enqueue, lpa_enqueue, lpr_run with forward_impl and the tail inside) run with a recorder installed (k_group.hpp), the launch
// tables and launches are gcnn_group.hpp's (group_tables, group_launches), and the twins of the appends' and rounds' launches are
// gcnn_lprounds.hpp's (lprounds_kernel).  What this file adds is the call's own layout, the checks across members, the removals'
// phase in front of the other two and the twins of the removal's launches (k_lpedits.hpp).  Kept apart so that its launch names
// form their own inventory (tests/test_lpedits_build.py).
#include "k_lpedits.hpp"

static_assert(sizeof(LpdArgs) <= GROUP_REC_BYTES, "k_group.hpp: GROUP_REC_BYTES");

#define LPES_REMOVE_STAGES 3      // launches of one member's removal
#define LPES_STAGES (LPES_REMOVE_STAGES + LPRS_STAGES)

// the removal's launches and their twins; every other kernel is gcnn_lprounds.hpp's or the forward pass's
static GroupKernel g_lpedits_kernels[] = {
    {(const void*)k_lpd_mark, (const void*)k_lpes_mark, "k_lpes_mark", {}},
    {(const void*)k_lpd_rows, (const void*)k_lpes_rows, "k_lpes_rows", {}},
    {(const void*)k_lpd_vars, (const void*)k_lpes_vars, "k_lpes_vars", {}},
};
static GroupKernel* lpedits_kernel(const void* solo) {
    for (GroupKernel& g : g_lpedits_kernels) if (g.solo == solo) return &g;
    return lprounds_kernel(solo);
}

static inline size_t lpedits_table_bytes(int n) {
    return (size_t)n * LPES_STAGES * (sizeof(GroupHead) + ((al16(GROUP_REC_BYTES) + 63) & ~(size_t)63));
}

// one member as the call sees it: the dims between and after its edits, its solo layout, and where the solo layout keeps its
// pieces relative to the member's upload and the member's part of the arena
struct LpesMember {
    bool app, rem, degenerate;
    gcnn_lp_dims mid, after;       // after the removal (the dims as given without one), after the append behind it
    gcnn_lp_append_layout AL;      // app without rem
    gcnn_lp_remove_layout DL;      // rem
    gcnn_lp_round_layout RL;       // relative to the member's round upload, its download block and its round arena
    size_t in_bytes, out_bytes, arena_bytes, extra_out;
    size_t up_rel, block_off[5];   // upload: where the round starts, where the block's arrays lie
    size_t round_rel, app_scratch_rel, rem_scratch_rel;
    size_t flags_off, append_flags_off;
    size_t app_counts_bytes, rem_counts_bytes;
};

static int lpedits_member(const gcnn_lp_rounds_edit_member& m, int mode, LpesMember* M) {
    const bool select = mode == GCNN_IBATCH_SELECT;
    if (m.has_append < 0 || m.has_append > 1 || m.has_remove < 0 || m.has_remove > 1 || (select ? m.n_forced < 0 : m.n_forced != -1))
        return GCNN_E_BADARG;
    memset(M, 0, sizeof(*M));
    M->app = m.has_append != 0; M->rem = m.has_remove != 0;
    const gcnn_lp_append_dims* b = M->app ? &m.block : nullptr;
    int rc;
    if (M->rem) {
        if ((rc = lpd_layout(&m.dims, &m.removed, b, m.present, m.n_forced, m.n_forced_entries, &M->DL))) return rc;
        if (!lpd_dims_after(&m.dims, &m.removed, b, &M->mid)) return GCNN_E_BADARG;
        M->after = M->mid;
        if (b && !lpa_dims_after(&M->mid, b, &M->after)) return GCNN_E_BADARG;
        const gcnn_lp_remove_layout& D = M->DL;
        M->RL = D.round;
        M->in_bytes = D.in_bytes; M->out_bytes = D.out_bytes; M->arena_bytes = D.arena_bytes; M->extra_out = b ? 32 : 16;
        M->up_rel = D.list_bytes + D.block_bytes;
        for (int i = 0; i < 5; ++i) M->block_off[i] = D.block_off[i];
        M->round_rel = D.round_off; M->app_scratch_rel = D.append_scratch_off; M->rem_scratch_rel = D.scratch_off;
        M->flags_off = D.flags_off; M->append_flags_off = D.append_flags_off;
        M->rem_counts_bytes = al16(lpd_scratch(&m.dims).clear_bytes);
        if (b) M->app_counts_bytes = al16(lpa_scratch(&M->mid, b).clear_bytes);
    } else if (M->app) {
        if ((rc = lpa_layout(&m.dims, b, m.present, m.n_forced, m.n_forced_entries, &M->AL))) return rc;
        M->mid = m.dims;
        if (!lpa_dims_after(&m.dims, b, &M->after)) return GCNN_E_BADARG;
        const gcnn_lp_append_layout& Q = M->AL;
        M->RL = Q.round;
        M->in_bytes = Q.in_bytes; M->out_bytes = Q.out_bytes; M->arena_bytes = Q.arena_bytes; M->extra_out = 16;
        M->up_rel = Q.block_bytes;
        for (int i = 0; i < 5; ++i) M->block_off[i] = Q.block_off[i];
        M->round_rel = Q.round_off; M->app_scratch_rel = Q.scratch_off;
        M->append_flags_off = Q.flags_off;
        M->app_counts_bytes = al16(lpa_scratch(&m.dims, b).clear_bytes);
    } else {
        if ((rc = lpr_round_layout(&m.dims, m.present, m.n_forced, m.n_forced_entries, &M->RL))) return rc;
        M->mid = M->after = m.dims;
        M->in_bytes = M->RL.in_bytes; M->out_bytes = M->RL.out_bytes; M->arena_bytes = M->RL.arena_bytes;
    }
    if (mode != GCNN_IBATCH_SCORES && M->after.n_cuts > 4096) return GCNN_E_UNSUPPORTED;
    M->degenerate = group_degenerate(lp_state_dims(&M->after));
    return 0;
}

static int lpedits_layout(int n, const gcnn_lp_rounds_edit_member* mem, int mode, gcnn_lp_rounds_edit_layout* L, LpesMember* M) {
    if (n < 1 || n > GCNN_LP_ROUNDS_MAX || !mem || !L || mode < GCNN_IBATCH_SCORES || mode > GCNN_IBATCH_SELECT) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    L->n = n; L->mode = mode;
    int rc;
    for (int i = 0; i < n; ++i) if ((rc = lpedits_member(mem[i], mode, &M[i]))) return rc;
    Carver c{0};
    for (int i = 0; i < n; ++i) { L->in_size[i] = al256(M[i].in_bytes); L->in_off[i] = c.take(L->in_size[i], 256); }
    L->in_bytes = c.off;
    for (int i = 0; i < n; ++i) {
        L->arena_off[i] = c.take(M[i].arena_bytes, 256);
        L->member_round_off[i] = L->arena_off[i] + M[i].round_rel;
        L->scratch_off[i] = M[i].app ? L->arena_off[i] + M[i].app_scratch_rel : 0;
        L->remove_scratch_off[i] = M[i].rem ? L->arena_off[i] + M[i].rem_scratch_rel : 0;
    }
    // the one fill: every removal's counters and every append's count tables, side by side
    L->counts_base = c.off;
    for (int i = 0; i < n; ++i) {
        L->remove_counts_off[i] = M[i].rem ? c.take(M[i].rem_counts_bytes, 16) : 0;
        L->counts_off[i] = M[i].app ? c.take(M[i].app_counts_bytes, 16) : 0;
    }
    L->counts_bytes = c.off - L->counts_base;
    c.off = al256(c.off);
    L->out_base = c.off;
    for (int i = 0; i < n; ++i) { L->out_size[i] = al16(M[i].out_bytes); L->out_off[i] = c.take(L->out_size[i], 16) - L->out_base; }
    L->out_bytes = c.off - L->out_base;
    c.off = al256(c.off);
    L->table_bytes = lpedits_table_bytes(n);
    L->table_off = c.take(L->table_bytes, 256);
    L->arena_bytes = c.off;
    return 0;
}

extern "C" int gcnn_lp_rounds_edit_layout_for(int32_t n, const gcnn_lp_rounds_edit_member* members, int32_t mode,
                                              gcnn_lp_rounds_edit_layout* layout) {
    LpesMember M[GCNN_LP_ROUNDS_MAX];
    return lpedits_layout(n, members, mode, layout, M);
}

// gcnn_lprounds.hpp's rule, extended by what a removing member writes (out_*, the transit set, dst) and reads (src, the raw source)
static void lpedits_set(std::vector<LprsSpan>& to, const gcnn_lp_rows_set& s, const gcnn_lp_dims& d) {
    const size_t R = d.n_rows, V = d.n_cols, C = d.n_state_rows, E = d.n_state_edges;
    to.insert(to.end(), {{s.cons_feats, 16 * C}, {s.edge_row, 4 * E}, {s.edge_col, 4 * E}, {s.edge_coef, 4 * E}, {s.l_ptr, 4 * (C + 1)},
                         {s.v_ptr, 4 * (V + 1)}, {s.v_oth, 4 * E}, {s.v_coef, 4 * E}, {s.row_place, 8 * R}, {s.row_scale, 8 * R}});
}
static void lpedits_raw(std::vector<LprsSpan>& to, const void* const raw[5], const gcnn_lp_dims& d) {
    const size_t R = d.n_rows, N = d.row_nnz;
    to.insert(to.end(), {{raw[0], 4 * (R + 1)}, {raw[1], 4 * N}, {raw[2], 8 * N}, {raw[3], 8 * R}, {raw[4], 8 * R}});
}
static void lpedits_spans(const gcnn_lp_rounds_edit_member& m, const LpesMember& M, std::vector<LprsSpan>& wr, std::vector<LprsSpan>& rd) {
    const gcnn_lp_dims& a = M.after;
    const size_t R = a.n_rows, V = a.n_cols, C = a.n_state_rows, E = a.n_state_edges;
    const gcnn_lp_resident& r = *m.resident;
    const gcnn_graph& g = r.cons_graph;
    wr = {{r.cons_feats, 16 * C}, {r.col_lb, 8 * V}, {r.col_ub, 8 * V}, {r.col_primal, 8 * V}, {r.col_primal_avg, 8 * V}};
    rd = {{m.params, (size_t)g_ptotal * sizeof(float)}, {r.row_place, 8 * R}, {r.row_scale, 8 * R}, {r.col_type, V}, {r.col_obj, 8 * V},
          {g.l_ptr, 4 * (C + 1)}, {g.l_oth, 4 * E}, {g.l_coef, 4 * E}, {g.v_ptr, 4 * (V + 1)}, {g.v_oth, 4 * E}, {g.v_coef, 4 * E}};
    if (!M.app && !M.rem) return;
    const void* const raw[5] = {m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs};
    const void* const out[5] = {m.out_ptr, m.out_col, m.out_val, m.out_lhs, m.out_rhs};
    lpedits_set(wr, *m.dst, a);
    lpedits_set(rd, *m.src, m.dims);
    if (M.rem) {
        lpedits_raw(rd, raw, m.dims);
        lpedits_raw(wr, out, a);
        if (M.app) lpedits_set(wr, *m.transit, M.mid);
    } else {
        lpedits_raw(wr, raw, a);
    }
}
static bool lpedits_overlap(int n, const gcnn_lp_rounds_edit_member* mem, const LpesMember* M) {
    std::vector<LprsSpan> wr[GCNN_LP_ROUNDS_MAX], rd[GCNN_LP_ROUNDS_MAX];
    for (int i = 0; i < n; ++i) lpedits_spans(mem[i], M[i], wr[i], rd[i]);
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

// what the solo call of member m decides before anything is enqueued (gcnn_lp_round_remove / _append / gcnn_lp_round)
static int lpedits_check(const gcnn_lp_rounds_edit_member& m, const LpesMember& M, const void* host_in, void* host_out, char* round_arena,
                         int want, double p_max, double p_max_ub) {
    if (!m.resident) return GCNN_E_BADARG;
    int rc;
    gcnn_lp_dims mid, after;
    const gcnn_lp_append_dims* b = M.app ? &m.block : nullptr;
    if (M.rem) {
        const void* const raw_src[5] = {m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs};
        const void* const raw_dst[5] = {m.out_ptr, m.out_col, m.out_val, m.out_lhs, m.out_rhs};
        const gcnn_lp_rows_set* first = b ? m.transit : m.dst;      // what the removal writes
        if ((rc = lpd_check(&m.dims, &m.removed, b, &mid, raw_src, raw_dst, b ? &M.after : nullptr, m.src, first))) return rc;
        if (b) {
            if ((rc = lpa_check(&mid, b, &after, m.out_ptr, m.out_col, m.out_val, m.out_lhs, m.out_rhs, m.resident->col_obj, m.transit, m.dst)))
                return rc;
            const std::vector<LpdSpan> last = lpd_set_spans(m.dst, &after);
            if (lpd_meet(lpd_set_spans(m.src, &m.dims), last) || lpd_meet(lpd_set_spans(m.transit, &mid), last)) return GCNN_E_BADARG;
        }
    } else if (b) {
        if ((rc = lpa_check(&m.dims, b, &after, m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs, m.resident->col_obj, m.src, m.dst)))
            return rc;
    }
    gcnn_lp_round_layout RL;
    return lpr_check(&M.after, m.present, m.n_forced, m.n_forced_entries, m.resident, m.params, host_in, host_out, round_arena,
                     M.RL.arena_bytes, want, p_max, p_max_ub, M.extra_out, &RL);
}

struct LpesPlan { GroupLaunch launches[GCNN_LP_ROUNDS_MAX * LPES_STAGES]; int nl; size_t bytes; };

extern "C" int gcnn_lp_rounds_edit(int32_t n, const gcnn_lp_rounds_edit_member* mem, int32_t mode, const void* host_in, void* host_out,
                                   void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream) {
    gcnn_lp_rounds_edit_layout L;
    static thread_local LpesMember M[GCNN_LP_ROUNDS_MAX];
    int rc = lpedits_layout(n, mem, mode, &L, M);
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
    for (int i = 0; i < n; ++i)
        if ((rc = lpedits_check(mem[i], M[i], host_in, host_out, A + L.member_round_off[i], want, p_max, p_max_ub))) return rc;
    if (lpedits_overlap(n, mem, M)) return GCNN_E_BADARG;
    // 2. record: the removals, the appends, then the rounds of the regular members (nothing is enqueued)
    static thread_local std::vector<GroupRecord> recs;
    recs.resize((size_t)GCNN_LP_ROUNDS_MAX * LPES_STAGES);
    GroupRecorder rd[GCNN_LP_ROUNDS_MAX], ra[GCNN_LP_ROUNDS_MAX], rr[GCNN_LP_ROUNDS_MAX];
    int nrem = 0, napp = 0, nreg = 0;
    auto at_of = [&](int i) { return LprAt{A + L.in_off[i] + M[i].up_rel, A + L.out_base + L.out_off[i]}; };
    auto round_of = [&](int i, const LprAt& at) {
        const gcnn_lp_rounds_edit_member& m = mem[i];
        return lpr_run(&M[i].after, M[i].RL, m.present, m.n_forced, m.resident, m.params, nullptr, nullptr, A + L.member_round_off[i], want, p_max,
                       p_max_ub, stream, &at);
    };
    for (int i = 0; i < n; ++i) {
        const gcnn_lp_rounds_edit_member& m = mem[i];
        GroupRecord* slot = recs.data() + (size_t)i * LPES_STAGES;
        const LprAt at = at_of(i);
        const char* up = A + L.in_off[i];
        if (M[i].rem) {
            GroupRecorder& q = rd[nrem++];
            q = GroupRecorder{slot, 0, LPES_REMOVE_STAGES, false};
            const void* const raw_src[5] = {m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs};
            void* const raw_dst[5] = {m.out_ptr, m.out_col, m.out_val, m.out_lhs, m.out_rhs};
            GroupRecScope scope(&q);
            if ((rc = lpd_enqueue(&m.dims, &m.removed, &M[i].mid, (const int32_t*)up, raw_src, raw_dst, m.src, M[i].app ? m.transit : m.dst,
                                  A + L.remove_scratch_off[i], (int32_t*)(at.out + M[i].flags_off), st, A + L.remove_counts_off[i])))
                return rc;
        }
        if (M[i].app) {
            GroupRecorder& q = ra[napp++];
            q = GroupRecorder{slot + LPES_REMOVE_STAGES, 0, LPRS_APPEND_STAGES, false};
            const size_t* bo = M[i].block_off;
            int32_t* const raw[2] = {M[i].rem ? m.out_ptr : m.row_ptr, M[i].rem ? m.out_col : m.row_col};
            double* const rawd[3] = {M[i].rem ? m.out_val : m.row_val, M[i].rem ? m.out_lhs : m.row_lhs, M[i].rem ? m.out_rhs : m.row_rhs};
            GroupRecScope scope(&q);
            if ((rc = lpa_enqueue(&M[i].mid, &m.block, (const int*)(up + bo[0]), (const int*)(up + bo[1]), (const double*)(up + bo[2]),
                                  (const double*)(up + bo[3]), (const double*)(up + bo[4]), m.block.row_nnz, 0, raw, rawd, m.resident->col_obj,
                                  M[i].rem ? m.transit : m.src, m.dst, A + L.scratch_off[i], (int32_t*)(at.out + M[i].append_flags_off), st,
                                  A + L.counts_off[i])))
                return rc;
        }
        if (M[i].degenerate) continue;
        GroupRecorder& q = rr[nreg++];
        q = GroupRecorder{slot + LPES_REMOVE_STAGES + LPRS_APPEND_STAGES, 0, GCNN_GROUP_MAX_STAGES, false};
        GroupRecScope scope(&q);
        if ((rc = round_of(i, at))) return rc;
    }
    // 3. the launch tables of the three phases in the staging buffer
    static thread_local LpesPlan plan;
    plan.nl = 0; plan.bytes = 0;
    const int cap = GCNN_LP_ROUNDS_MAX * LPES_STAGES;
    if ((rc = group_tables(nrem, rd, host_staging, lpedits_kernel, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if ((rc = group_tables(napp, ra, host_staging, lpedits_kernel, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if ((rc = group_tables(nreg, rr, host_staging, lpedits_kernel, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if (plan.bytes > L.table_bytes) return GCNN_E_WORKSPACE;
    // 4. ONE upload of all lists, blocks and rounds, one of the tables, at most ONE fill, the launches, ONE download
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));
    if (plan.bytes) HIPCHK(hipMemcpyAsync(A + L.table_off, host_staging, plan.bytes, hipMemcpyHostToDevice, st));
    if (L.counts_bytes) HIPCHK(hipMemsetAsync(A + L.counts_base, 0, L.counts_bytes, st));
    if ((rc = group_launches(plan.launches, plan.nl, A + L.table_off, st))) return rc;
    for (int i = 0; i < n; ++i)
        if (M[i].degenerate && (rc = round_of(i, at_of(i)))) return rc;      // its solo launches, on the call's addresses
    HIPCHK(hipMemcpyAsync(host_out, A + L.out_base, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
