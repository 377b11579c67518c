// gcnn_lpedits.hpp -- host side of the rounds of 1..GCNN_LP_ROUNDS_MAX resident LPs in one call (include/gcnn_hip.h): gcnn_lp_rounds,
// each member with or without an append, and gcnn_lp_rounds_edit, each also with or without a removal.  Both are one body on the
// round with edits of gcnn_lpremove.hpp: a member becomes an LpEdit, and its work is the unchanged solo code (lpe_check,
// lpe_enqueue_edits, lpr_run with forward_impl and the tail inside) run with a recorder installed (k_group.hpp); the launch tables
// and launches are gcnn_group.hpp's (group_tables, group_launches).  What this file adds is the call's own layout, the overlap rule
// across members, the three phases (removals, appends, rounds: so the rounds share their stages whatever edits a member carries)
// and the twins of the removal's launches (k_lpedits.hpp); the twins of the appends' and rounds' launches are gcnn_lprounds.hpp's
// (lprounds_kernel).  The two calls differ in the member struct they read, in the stages their tables are sized for and in the
// twin lookup.  Included at the end of gcnn_capi.hip behind gcnn_lpremove.hpp and gcnn_lprounds.hpp, kept apart so that its launch
// names form their own inventory (tests/test_lpedits_build.py).
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

// one member of either call as an LpEdit and its plan; a gcnn_lp_rounds_member is the front of a gcnn_lp_rounds_edit_member
template <class Member>
static int lpes_member(const Member& m, int mode, LpEdit* e, LpePlan* P) {
    int has_remove = 0;
    if constexpr (std::is_same_v<Member, gcnn_lp_rounds_edit_member>) has_remove = m.has_remove;
    const bool select = mode == GCNN_IBATCH_SELECT;
    if (m.has_append < 0 || m.has_append > 1 || has_remove < 0 || has_remove > 1 || (select ? m.n_forced < 0 : m.n_forced != -1))
        return GCNN_E_BADARG;
    *e = LpEdit{&m.dims, nullptr, m.has_append ? &m.block : nullptr, m.present, m.n_forced, m.n_forced_entries, {},
                {m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs}, m.src, nullptr, m.dst, m.resident, m.params};
    if constexpr (std::is_same_v<Member, gcnn_lp_rounds_edit_member>) {
        if (has_remove) {                                       // row_* are the raw source, out_* the raw rows the edit leaves
            void* const out[5] = {m.out_ptr, m.out_col, m.out_val, m.out_lhs, m.out_rhs};
            for (int i = 0; i < 5; ++i) { e->raw_in[i] = e->raw[i]; e->raw[i] = out[i]; }
            e->rem = &m.removed; e->transit = m.transit;
        }
    }
    const int rc = lpe_plan(*e, P);
    if (rc) return rc;
    return mode != GCNN_IBATCH_SCORES && P->after.n_cuts > 4096 ? GCNN_E_UNSUPPORTED : 0;
}

// The layout of either call, into either layout struct (gcnn_lp_rounds_layout is gcnn_lp_rounds_edit_layout without the removals'
// offsets); stages: what the tables are sized for.
template <class Member, class Layout>
static int lpes_layout(int n, const Member* mem, int mode, int stages, Layout* L, LpEdit* E, LpePlan* P) {
    constexpr bool removes = std::is_same_v<Layout, gcnn_lp_rounds_edit_layout>;
    if (n < 1 || n > GCNN_LP_ROUNDS_MAX || !mem || !L || mode < GCNN_IBATCH_SCORES || mode > GCNN_IBATCH_SELECT) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    L->n = n; L->mode = mode;
    int rc;
    for (int i = 0; i < n; ++i) if ((rc = lpes_member(mem[i], mode, &E[i], &P[i]))) return rc;
    Carver c{0};
    for (int i = 0; i < n; ++i) { L->in_size[i] = al256(P[i].in_bytes); L->in_off[i] = c.take(L->in_size[i], 256); }
    L->in_bytes = c.off;
    for (int i = 0; i < n; ++i) {
        L->arena_off[i] = c.take(P[i].arena_bytes, 256);
        L->member_round_off[i] = L->arena_off[i] + P[i].round_rel;
        L->scratch_off[i] = E[i].app ? L->arena_off[i] + P[i].app_scratch_rel : 0;
        if constexpr (removes) L->remove_scratch_off[i] = E[i].rem ? L->arena_off[i] + P[i].rem_scratch_rel : 0;
    }
    // the one fill: every removal's counters and every append's count tables, side by side
    L->counts_base = c.off;
    for (int i = 0; i < n; ++i) {
        const size_t rem_counts = E[i].rem ? c.take(P[i].rem_counts_bytes, 16) : 0;
        if constexpr (removes) L->remove_counts_off[i] = rem_counts;
        L->counts_off[i] = E[i].app ? c.take(P[i].app_counts_bytes, 16) : 0;
    }
    L->counts_bytes = c.off - L->counts_base;
    c.off = al256(c.off);
    L->out_base = c.off;
    for (int i = 0; i < n; ++i) { L->out_size[i] = al16(P[i].out_bytes); L->out_off[i] = c.take(L->out_size[i], 16) - L->out_base; }
    L->out_bytes = c.off - L->out_base;
    c.off = al256(c.off);
    L->table_bytes = group_table_bytes(n, stages);
    L->table_off = c.take(L->table_bytes, 256);
    L->arena_bytes = c.off;
    return 0;
}

extern "C" int gcnn_lp_rounds_layout_for(int32_t n, const gcnn_lp_rounds_member* members, int32_t mode, gcnn_lp_rounds_layout* layout) {
    LpEdit E[GCNN_LP_ROUNDS_MAX]; LpePlan P[GCNN_LP_ROUNDS_MAX];
    return layout_out(layout, [&](gcnn_lp_rounds_layout* l) { return lpes_layout(n, members, mode, LPRS_STAGES, l, E, P); });
}
extern "C" int gcnn_lp_rounds_edit_layout_for(int32_t n, const gcnn_lp_rounds_edit_member* members, int32_t mode,
                                              gcnn_lp_rounds_edit_layout* layout) {
    LpEdit E[GCNN_LP_ROUNDS_MAX]; LpePlan P[GCNN_LP_ROUNDS_MAX];
    return layout_out(layout, [&](gcnn_lp_rounds_edit_layout* l) { return lpes_layout(n, members, mode, LPES_STAGES, l, E, P); });
}

// group_check's rule on resident LPs: what a member's launches write must not overlap anything another member's launches touch.
// What a checked member writes (the resident columns and features; with an edit dst, the raw rows it leaves and the transit set)
// and what it reads (the parameters, the resident LP; with an edit src, and a removal's raw source):
static void lpes_spans(const LpEdit& e, const LpePlan& P, LpSpans& wr, LpSpans& rd) {
    const gcnn_lp_dims& a = P.after;
    const size_t R = a.n_rows, V = a.n_cols, C = a.n_state_rows, E = a.n_state_edges;
    const gcnn_lp_resident& r = *e.resident;
    const gcnn_graph& g = r.cons_graph;
    wr.add(r.cons_feats, 16 * C).add(r.col_lb, 8 * V).add(r.col_ub, 8 * V).add(r.col_primal, 8 * V).add(r.col_primal_avg, 8 * V);
    rd.add(e.params, (size_t)g_ptotal * sizeof(float)).add(r.row_place, 8 * R).add(r.row_scale, 8 * R).add(r.col_type, V).add(r.col_obj, 8 * V)
        .add(g.l_ptr, 4 * (C + 1)).add(g.l_oth, 4 * E).add(g.l_coef, 4 * E).add(g.v_ptr, 4 * (V + 1)).add(g.v_oth, 4 * E).add(g.v_coef, 4 * E);
    if (!e.rem && !e.app) return;
    wr.set(e.dst, &a).raw(e.raw, &a);
    rd.set(e.src, e.dims);
    if (e.rem) rd.raw(e.raw_in, e.dims);
    if (e.rem && e.app) wr.set(e.transit, &P.mid);
}
static bool lpes_overlap(int n, const LpEdit* E, const LpePlan* P) {
    LpSpans wr[GCNN_LP_ROUNDS_MAX], rd[GCNN_LP_ROUNDS_MAX];
    for (int i = 0; i < n; ++i) lpes_spans(E[i], P[i], wr[i], rd[i]);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (i != j && (wr[i].meets(wr[j]) || wr[i].meets(rd[j]))) return true;
    return false;
}

struct LpesLaunches { GroupLaunch launches[GCNN_LP_ROUNDS_MAX * LPES_STAGES]; int nl; size_t bytes; };
// a call's members, planned: on this thread, so that a call allocates nothing
struct LpesCall { LpEdit E[GCNN_LP_ROUNDS_MAX]; LpePlan P[GCNN_LP_ROUNDS_MAX]; gcnn_lp_rounds_edit_layout L; };
static thread_local LpesCall g_lpes_call;

// The call proper, on planned members.  rem_stages: the stages a member's removal may take (none in gcnn_lp_rounds); find: the twins.
static int lpes_run(int n, const LpesCall& call, int mode, int rem_stages, GroupLookup find, const void* host_in, void* host_out, void* arena,
                    size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream) {
    const LpEdit* E = call.E;
    const LpePlan* P = call.P;
    const gcnn_lp_rounds_edit_layout& L = call.L;
    const bool select = mode == GCNN_IBATCH_SELECT;
    const int want = mode != GCNN_IBATCH_SCORES;
    const int stages = rem_stages + LPRS_STAGES;
    if (!host_in || !host_out || !host_staging || ((uintptr_t)host_staging & 15) || !arena || ((uintptr_t)arena & 255) ||
        arena_bytes < L.arena_bytes)
        return GCNN_E_BADARG;
    if (select && !finite_thresholds(p_max, p_max_ub)) return GCNN_E_BADARG;
    layout_init();
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    int rc;
    // 1. everything the solo calls check, member by member, then the members against each other
    for (int i = 0; i < n; ++i) {
        if (!E[i].resident) return GCNN_E_BADARG;
        if ((rc = lpe_check(E[i], P[i], host_in, host_out, A + L.arena_off[i], P[i].arena_bytes, want, p_max, p_max_ub))) return rc;
    }
    if (lpes_overlap(n, E, P)) return GCNN_E_BADARG;
    // 2. record: the removals, the appends, then the rounds of the regular members (nothing is enqueued)
    static thread_local std::vector<GroupRecord> recs;
    recs.resize((size_t)GCNN_LP_ROUNDS_MAX * LPES_STAGES);
    GroupRecorder rd[GCNN_LP_ROUNDS_MAX], ra[GCNN_LP_ROUNDS_MAX], rr[GCNN_LP_ROUNDS_MAX];
    int nrem = 0, napp = 0, nreg = 0;
    auto at_of = [&](int i) { return LprAt{A + L.in_off[i] + P[i].round_rel, A + L.out_base + L.out_off[i]}; };
    auto round_of = [&](int i, const LprAt& at) {
        return lpr_run(&P[i].after, P[i].RL, E[i].present, E[i].n_forced, E[i].resident, E[i].params, nullptr, nullptr, A + L.member_round_off[i],
                       want, p_max, p_max_ub, stream, &at);
    };
    for (int i = 0; i < n; ++i) {
        GroupRecord* slot = recs.data() + (size_t)i * stages;
        const LprAt at = at_of(i);
        LpeAt edits = {A + L.in_off[i], at.out, A + L.remove_scratch_off[i], A + L.scratch_off[i], A + L.remove_counts_off[i],
                       A + L.counts_off[i], nullptr, nullptr};
        if (E[i].rem) { edits.rem_rec = &rd[nrem++]; *edits.rem_rec = GroupRecorder{slot, 0, rem_stages, false}; }
        if (E[i].app) { edits.app_rec = &ra[napp++]; *edits.app_rec = GroupRecorder{slot + rem_stages, 0, LPRS_APPEND_STAGES, false}; }
        if ((rc = lpe_enqueue_edits(E[i], P[i], edits, st))) return rc;
        if (P[i].degenerate) continue;
        GroupRecorder& q = rr[nreg++];
        q = GroupRecorder{slot + rem_stages + LPRS_APPEND_STAGES, 0, GCNN_GROUP_MAX_STAGES, false};
        GroupRecScope scope(&q);
        if ((rc = round_of(i, at))) return rc;
    }
    // 3. the launch tables of the three phases in the staging buffer
    static thread_local LpesLaunches plan;
    plan.nl = 0; plan.bytes = 0;
    const int cap = GCNN_LP_ROUNDS_MAX * stages;
    if ((rc = group_tables(nrem, rd, host_staging, find, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if ((rc = group_tables(napp, ra, host_staging, find, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if ((rc = group_tables(nreg, rr, host_staging, find, plan.launches, cap, &plan.nl, &plan.bytes))) return rc;
    if (plan.bytes > L.table_bytes) return GCNN_E_WORKSPACE;
    // 4. ONE upload of all lists, blocks and rounds, one of the tables, at most ONE fill, the launches, ONE download
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));
    if (plan.bytes) HIPCHK(hipMemcpyAsync(A + L.table_off, host_staging, plan.bytes, hipMemcpyHostToDevice, st));
    if (L.counts_bytes) HIPCHK(hipMemsetAsync(A + L.counts_base, 0, L.counts_bytes, st));
    if ((rc = group_launches(plan.launches, plan.nl, A + L.table_off, st))) return rc;
    for (int i = 0; i < n; ++i)
        if (P[i].degenerate && (rc = round_of(i, at_of(i)))) return rc;      // its solo launches, on the call's addresses
    HIPCHK(hipMemcpyAsync(host_out, A + L.out_base, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}

extern "C" int gcnn_lp_rounds(int32_t n, const gcnn_lp_rounds_member* mem, int32_t mode, const void* host_in, void* host_out, void* arena,
                              size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream) {
    LpesCall& c = g_lpes_call;
    const int rc = lpes_layout(n, mem, mode, LPRS_STAGES, &c.L, c.E, c.P);
    return rc ? rc : lpes_run(n, c, mode, 0, lprounds_kernel, host_in, host_out, arena, arena_bytes, host_staging, p_max, p_max_ub, stream);
}

extern "C" int gcnn_lp_rounds_edit(int32_t n, const gcnn_lp_rounds_edit_member* mem, int32_t mode, const void* host_in, void* host_out,
                                   void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream) {
    LpesCall& c = g_lpes_call;
    const int rc = lpes_layout(n, mem, mode, LPES_STAGES, &c.L, c.E, c.P);
    return rc ? rc : lpes_run(n, c, mode, LPES_REMOVE_STAGES, lpedits_kernel, host_in, host_out, arena, arena_bytes, host_staging, p_max,
                              p_max_ub, stream);
}
