// gcnn_group.hpp -- groups of independent models stepped together (include/gcnn_hip.h: gcnn_group_train_step,
// gcnn_group_forward).  Included at the end of gcnn_capi.hip; the kernels and the recorder are in k_group.hpp.
//
// A group call records each member's solo step (the launchers' GCNN_LAUNCH), builds every launch table of the step in the
// caller's pinned staging buffer, uploads them with ONE copy, and then issues stage by stage one launch per distinct kernel.
// A member with an empty node set takes the solo entry points instead (their degenerate paths clear and launch differently).

#include <vector>

// the solo kernels a member's step can record, and the group kernel that runs each of them
struct GroupKernel { const void* solo; const void* group; const char* name; PerDeviceOnce attr; };
#define GK(SOLO, GROUP, NAME) GroupKernel{(const void*)SOLO, (const void*)GROUP, NAME, {}}
static GroupKernel g_group_kernels[] = {
    GK(k_embed_fwd<8>, k_group_embed_fwd<8>, "k_group_embed_fwd"),
    GK(k_embed_fwd<4>, k_group_embed_fwd<4>, "k_group_embed_fwd"),
    GK(k_embed_fwd_split, k_group_embed_fwd_split, "k_group_embed_fwd_split"),
    GK((k_edge_fwd<4, true, false>), (k_group_edge_fwd<4, true, false>), "k_group_edge_fwd<count>"),
    GK((k_edge_fwd<2, true, false>), (k_group_edge_fwd<2, true, false>), "k_group_edge_fwd<count>"),
    GK((k_edge_fwd<1, true, false>), (k_group_edge_fwd<1, true, false>), "k_group_edge_fwd<count>"),
    GK((k_edge_fwd<2, true, true>), (k_group_edge_fwd<2, true, true>), "k_group_edge_fwd<count> + long segments"),
    GK((k_edge_fwd<1, true, true>), (k_group_edge_fwd<1, true, true>), "k_group_edge_fwd<count> + long segments"),
    GK((k_edge_fwd<4, false, false>), (k_group_edge_fwd<4, false, false>), "k_group_edge_fwd"),
    GK((k_edge_fwd<2, false, false>), (k_group_edge_fwd<2, false, false>), "k_group_edge_fwd"),
    GK((k_edge_fwd<1, false, false>), (k_group_edge_fwd<1, false, false>), "k_group_edge_fwd"),
    GK((k_edge_fwd<2, false, true>), (k_group_edge_fwd<2, false, true>), "k_group_edge_fwd + long segments"),
    GK((k_edge_fwd<1, false, true>), (k_group_edge_fwd<1, false, true>), "k_group_edge_fwd + long segments"),
    GK(k_edge_fwd_block<true>, k_group_edge_fwd_block<true>, "k_group_edge_fwd_block<count>"),
    GK(k_edge_fwd_block<false>, k_group_edge_fwd_block<false>, "k_group_edge_fwd_block"),
    GK((k_conv_fwd<8, CF_PROJ>), (k_group_conv_fwd<8, CF_PROJ>), "k_group_conv_fwd<proj>"),
    GK((k_conv_fwd<4, CF_PROJ>), (k_group_conv_fwd<4, CF_PROJ>), "k_group_conv_fwd<proj>"),
    GK((k_conv_fwd<8, CF_READOUT>), (k_group_conv_fwd<8, CF_READOUT>), "k_group_conv_fwd<readout>"),
    GK((k_conv_fwd<4, CF_READOUT>), (k_group_conv_fwd<4, CF_READOUT>), "k_group_conv_fwd<readout>"),
    GK(k_conv_fwd_split<CF_PROJ>, k_group_conv_fwd_split<CF_PROJ>, "k_group_conv_fwd_split<proj>"),
    GK(k_conv_fwd_split<CF_READOUT>, k_group_conv_fwd_split<CF_READOUT>, "k_group_conv_fwd_split<readout>"),
    GK(k_conv_turn<8>, k_group_conv_turn<8>, "k_group_conv_turn"),
    GK(k_conv_turn<4>, k_group_conv_turn<4>, "k_group_conv_turn"),
    GK(k_conv_turn_split, k_group_conv_turn_split, "k_group_conv_turn_split"),
    GK(k_conv_bwd<8>, k_group_conv_bwd<8>, "k_group_conv_bwd"),
    GK(k_conv_bwd<4>, k_group_conv_bwd<4>, "k_group_conv_bwd"),
    GK(k_tail_bwd<8>, k_group_tail_bwd<8>, "k_group_tail_bwd"),
    GK(k_tail_bwd<4>, k_group_tail_bwd<4>, "k_group_tail_bwd"),
    GK((k_edge_bwd_send<4, false>), (k_group_edge_bwd_send<4, false>), "k_group_edge_bwd_send"),
    GK((k_edge_bwd_send<2, false>), (k_group_edge_bwd_send<2, false>), "k_group_edge_bwd_send"),
    GK((k_edge_bwd_send<1, false>), (k_group_edge_bwd_send<1, false>), "k_group_edge_bwd_send"),
    GK((k_edge_bwd_send<2, true>), (k_group_edge_bwd_send<2, true>), "k_group_edge_bwd_send + long segments"),
    GK((k_edge_bwd_send<1, true>), (k_group_edge_bwd_send<1, true>), "k_group_edge_bwd_send + long segments"),
    GK(k_wgrad, k_group_wgrad, "k_group_wgrad"),
    GK(k_reduce, k_group_reduce, "k_group_reduce"),
    // PreNorm fitting (gcnn_prenorm.hpp): the forward's keep-A row programs, then the statistics and the merge (k_prenorm.hpp)
    GK((k_conv_fwd<8, CF_PROJ, true>), (k_pgroup_conv_fwd<8, CF_PROJ>), "k_group_conv_fwd<proj, keep A>"),
    GK((k_conv_fwd<4, CF_PROJ, true>), (k_pgroup_conv_fwd<4, CF_PROJ>), "k_group_conv_fwd<proj, keep A>"),
    GK((k_conv_fwd<8, CF_READOUT, true>), (k_pgroup_conv_fwd<8, CF_READOUT>), "k_group_conv_fwd<readout, keep A>"),
    GK((k_conv_fwd<4, CF_READOUT, true>), (k_pgroup_conv_fwd<4, CF_READOUT>), "k_group_conv_fwd<readout, keep A>"),
    GK((k_conv_fwd_split<CF_PROJ, true>), k_pgroup_conv_fwd_split<CF_PROJ>, "k_group_conv_fwd_split<proj, keep A>"),
    GK((k_conv_fwd_split<CF_READOUT, true>), k_pgroup_conv_fwd_split<CF_READOUT>, "k_group_conv_fwd_split<readout, keep A>"),
    GK(k_expand_ptr, k_pgroup_expand_ptr, "k_group_expand_ptr"),
    GK(k_stats, k_pgroup_stats, "k_group_stats"),
    GK(k_stats_fold, k_pgroup_stats_fold, "k_group_stats_fold"),
};
#undef GK
static GroupKernel* group_kernel(const void* solo) {
    for (GroupKernel& g : g_group_kernels) if (g.solo == solo) return &g;
    return nullptr;
}

// every launch of the step: a head and at least one record (each padded to 64 B at most); GCNN_GROUP_MAX_STAGES launches per
// member at most (stages: of a call that records more phases, gcnn_lpedits.hpp).  (What a step uploads is what it uses: records at
// their own size, about 40 KB per setcov member.)
static inline size_t group_table_bytes(int n, int stages = GCNN_GROUP_MAX_STAGES) {
    return (size_t)n * stages * (sizeof(GroupHead) + ((al16(GROUP_REC_BYTES) + 63) & ~(size_t)63));
}

extern "C" int gcnn_group_table_bytes(int32_t n_members, size_t* bytes) {
    if (n_members < 1 || n_members > GCNN_GROUP_MAX || !bytes) return GCNN_E_BADARG;
    *bytes = group_table_bytes(n_members);
    return 0;
}

static bool group_degenerate(const gcnn_dims& d) { return d.n_cons <= 0 || d.n_vars <= 0 || d.n_cuts <= 0; }

// Everything a group call checks before it enqueues anything.  A member's writable buffers must not overlap any buffer of
// another member, written or read: their launches run side by side.  Read-only inputs may be shared.  `states` (PreNorm
// fitting, gcnn_group_prenorm_merge): one merge state per member, writable; the forward's scores then stay in the workspace.
static int group_check(int n, const gcnn_group_member* mem, const void* host, const void* dev, size_t table_bytes, bool train,
                       void* const* states = nullptr) {
    if (n < 1 || n > GCNN_GROUP_MAX || !mem || !host || !dev) return GCNN_E_BADARG;
    if (((uintptr_t)dev & 63) || ((uintptr_t)host & 15)) return GCNN_E_BADARG;
    if (table_bytes < group_table_bytes(n)) return GCNN_E_WORKSPACE;
    layout_init();
    const size_t P = (size_t)g_ptotal * sizeof(float);
    struct Span { const void* p; size_t bytes; };
    std::vector<Span> spans[GCNN_GROUP_MAX], reads[GCNN_GROUP_MAX];
    for (int i = 0; i < n; ++i) {
        const gcnn_group_member& m = mem[i];
        int rc = check_common(&m.dims, m.params, &m.cons_graph, &m.cut_graph, m.workspace, m.workspace_floats);
        if (rc) return rc;
        if (states) {
            if (!states[i] || ((uintptr_t)states[i] & 7)) return GCNN_E_BADARG;
            spans[i] = {{m.workspace, m.workspace_floats * sizeof(float)}, {states[i], (size_t)GCNN_PRENORM_STATE_BYTES}};
        } else {
            if (m.dims.n_cuts > 0 && !m.scores) return GCNN_E_BADARG;
            spans[i] = {{m.workspace, m.workspace_floats * sizeof(float)}, {m.scores, (size_t)m.dims.n_cuts * sizeof(float)}};
        }
        const size_t C = m.dims.n_cons, V = m.dims.n_vars, K = m.dims.n_cuts, E1 = m.dims.n_cons_edges, E2 = m.dims.n_cut_edges;
        const gcnn_graph &cg = m.cons_graph, &kg = m.cut_graph;
        reads[i] = {{m.params, P}, {m.cons_feats, 16 * C}, {m.var_feats, 56 * V}, {m.cut_feats, 24 * K},
                    {cg.l_ptr, 4 * (C + 1)}, {cg.l_oth, 4 * E1}, {cg.l_coef, 4 * E1}, {cg.v_ptr, 4 * (V + 1)}, {cg.v_oth, 4 * E1},
                    {cg.v_coef, 4 * E1}, {kg.l_ptr, 4 * (K + 1)}, {kg.l_oth, 4 * E2}, {kg.l_coef, 4 * E2}, {kg.v_ptr, 4 * (V + 1)},
                    {kg.v_oth, 4 * E2}, {kg.v_coef, 4 * E2}};
        if (!train) continue;
        reads[i].push_back({m.targets, 4 * K});
        if (!m.grads || (m.dims.n_cuts > 0 && !m.targets)) return GCNN_E_BADARG;
        if (m.adam && (!m.adam->params || !m.adam->m || !m.adam->v)) return GCNN_E_BADARG;
        spans[i].push_back({m.grads, P});
        spans[i].push_back({m.loss_out, sizeof(float)});
        if (m.adam) for (const void* q : {(const void*)m.adam->params, (const void*)m.adam->m, (const void*)m.adam->v}) spans[i].push_back({q, P});
    }
    auto overlap = [](const Span& a, const Span& b) {
        if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
        const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
        return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
    };
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (i == j) continue;
            for (const Span& a : spans[i]) {
                for (const Span& b : spans[j]) if (overlap(a, b)) return GCNN_E_BADARG;
                for (const Span& b : reads[j]) if (overlap(a, b)) return GCNN_E_BADARG;
            }
        }
    return 0;
}

// One member's step as the solo entry points enqueue it: launched (rec == nullptr) or recorded
static int group_member_step(const gcnn_group_member& m, bool train, hipStream_t st) {
    const gcnn_dims* d = &m.dims;
    if (!train)
        return forward_impl(d, m.params, m.cons_feats, m.var_feats, m.cut_feats, &m.cons_graph, &m.cut_graph, m.workspace,
                            m.workspace_floats, m.scores, 0, nullptr, 0.f, st);
    int rc = gcnn_forward_loss(d, m.params, m.cons_feats, m.var_feats, m.cut_feats, &m.cons_graph, &m.cut_graph, m.workspace,
                               m.workspace_floats, m.scores, m.targets, m.loss_scale, st);
    if (rc) return rc;
    return gcnn_backward(d, m.params, m.cons_feats, m.var_feats, m.cut_feats, &m.cons_graph, &m.cut_graph, m.workspace,
                         m.workspace_floats, nullptr, m.grads, nullptr, m.loss_out, m.adam, st);
}

struct GroupRecScope {   // installs a recorder on this thread for one member's step
    explicit GroupRecScope(GroupRecorder* r) { g_group_rec = r; }
    ~GroupRecScope() { g_group_rec = nullptr; }
};

// The group call proper, after group_check, in two halves.  group_plan records every regular member's step and builds the launch
// tables in the caller's staging buffer: host work only, so whatever it refuses is refused before anything is enqueued.
// group_issue uploads the tables and launches.  member_step(i) enqueues member i's solo work (or records it).
struct GroupLaunch { GroupKernel* k; size_t off; int grid, block; size_t smem; };
struct GroupPlan { GroupLaunch launches[GCNN_GROUP_MAX * GCNN_GROUP_MAX_STAGES]; int nl; size_t bytes; };

// The launch tables of recorded steps, stage by stage, appended at *off of the staging buffer: the members whose s-th launch runs
// the same kernel share one launch.  r[0..nreg): the members' recordings; find: the group kernel of a solo kernel.
typedef GroupKernel* (*GroupLookup)(const void*);
static int group_tables(int nreg, const GroupRecorder* r, void* host, GroupLookup find, GroupLaunch* launches, int cap, int* nl_io,
                        size_t* off_io) {
    int nl = *nl_io, nstage = 0;
    size_t off = *off_io;
    char* h = (char*)host;
    for (int i = 0; i < nreg; ++i) {
        if (r[i].bad) return GCNN_E_UNSUPPORTED;
        for (int s = 0; s < r[i].n; ++s) if (!find(r[i].rec[s].kern)) return GCNN_E_UNSUPPORTED;
        nstage = std::max(nstage, r[i].n);
    }
    for (int s = 0; s < nstage; ++s) {
        bool done[GCNN_GROUP_MAX] = {};
        for (int i = 0; i < nreg; ++i) {
            if (done[i] || s >= r[i].n) continue;
            const GroupRecord& first = r[i].rec[s];
            GroupHead* head = (GroupHead*)(h + off);
            char* body = h + off + sizeof(GroupHead);
            memset(head, 0, sizeof(*head));
            const size_t stride = al16((size_t)first.bytes);   // one kernel per launch: every record has its size
            head->stride = (int)stride;
            for (int j = i; j < nreg; ++j) {
                if (done[j] || s >= r[j].n || r[j].rec[s].kern != first.kern) continue;
                const GroupRecord& q = r[j].rec[s];
                if (q.block != first.block || q.smem != first.smem) return GCNN_E_UNSUPPORTED;
                memcpy(body + (size_t)head->n * stride, q.args, (size_t)q.bytes);
                head->blk0[head->n + 1] = head->blk0[head->n] + q.grid;
                ++head->n;
                done[j] = true;
            }
            if (nl >= cap) return GCNN_E_UNSUPPORTED;
            launches[nl++] = GroupLaunch{find(first.kern), off, head->blk0[head->n], first.block, first.smem};
            off = (off + sizeof(GroupHead) + (size_t)head->n * stride + 63) & ~(size_t)63;
        }
    }
    *nl_io = nl; *off_io = off;
    return 0;
}
// the launches of such tables, once they lie at `dev`
static int group_launches(const GroupLaunch* launches, int nl, void* dev, hipStream_t st) {
    for (int k = 0; k < nl; ++k) {
        const GroupLaunch& L = launches[k];
        if (L.grid <= 0) continue;
        if (L.smem > 0 && L.k->attr.first())
            HIPCHK(hipFuncSetAttribute(L.k->group, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.smem));
        const GroupHead* tab = (const GroupHead*)((char*)dev + L.off);
        void* args[] = {&tab};
        ProfScope prof(L.k->name, st);
        HIPCHK(hipLaunchKernel(L.k->group, dim3(L.grid), dim3(L.block), args, L.smem, st));
    }
    return 0;
}

template <class Step>
static int group_plan(int n, const gcnn_group_member* mem, void* host, Step member_step, GroupPlan* P) {
    int rc;
    // 1. record every regular member's step (nothing is enqueued)
    static thread_local std::vector<GroupRecord> recs;
    recs.resize((size_t)GCNN_GROUP_MAX * GCNN_GROUP_MAX_STAGES);
    GroupRecorder r[GCNN_GROUP_MAX];
    int nreg = 0;
    for (int i = 0; i < n; ++i) {
        if (group_degenerate(mem[i].dims)) continue;
        GroupRecorder& q = r[nreg];
        q = GroupRecorder{recs.data() + (size_t)nreg * GCNN_GROUP_MAX_STAGES, 0, GCNN_GROUP_MAX_STAGES, false};
        {
            GroupRecScope scope(&q);
            rc = member_step(i);
        }
        if (rc) return rc;
        ++nreg;
    }
    // 2. the launch tables
    int nl = 0;
    size_t off = 0;
    if ((rc = group_tables(nreg, r, host, group_kernel, P->launches, GCNN_GROUP_MAX * GCNN_GROUP_MAX_STAGES, &nl, &off))) return rc;
    P->nl = nl; P->bytes = off;
    return 0;
}

// 3. one upload, then the launches; the members with an empty node set run their solo steps behind them
template <class Step>
static int group_issue(int n, const gcnn_group_member* mem, void* host, void* dev, const GroupPlan& P, Step member_step, hipStream_t st) {
    int rc;
    if (P.bytes) HIPCHK(hipMemcpyAsync(dev, host, P.bytes, hipMemcpyHostToDevice, st));
    if ((rc = group_launches(P.launches, P.nl, dev, st))) return rc;
    for (int i = 0; i < n; ++i)
        if (group_degenerate(mem[i].dims) && (rc = member_step(i))) return rc;
    return 0;
}

template <class Step>
static int group_run(int n, const gcnn_group_member* mem, void* host, void* dev, Step member_step, hipStream_t st) {
    static thread_local GroupPlan plan;
    const int rc = group_plan(n, mem, host, member_step, &plan);
    return rc ? rc : group_issue(n, mem, host, dev, plan, member_step, st);
}

static int group_step(int n, const gcnn_group_member* mem, void* host, void* dev, size_t table_bytes, bool train, hipStream_t st) {
    const int rc = group_check(n, mem, host, dev, table_bytes, train);
    if (rc) return rc;
    return group_run(n, mem, host, dev, [&](int i) { return group_member_step(mem[i], train, st); }, st);
}

extern "C" int gcnn_group_train_step(int32_t n_members, const gcnn_group_member* members, void* host_staging, void* device_table,
                                     size_t table_bytes, void* stream) {
    return group_step(n_members, members, host_staging, device_table, table_bytes, true, (hipStream_t)stream);
}
extern "C" int gcnn_group_forward(int32_t n_members, const gcnn_group_member* members, void* host_staging, void* device_table,
                                  size_t table_bytes, void* stream) {
    return group_step(n_members, members, host_staging, device_table, table_bytes, false, (hipStream_t)stream);
}
