// gcnn_prenorm.hpp -- PreNorm fitting with the streaming merge on the device (include/gcnn_hip.h: gcnn_prenorm_merge,
// gcnn_group_prenorm_merge).  Included at the end of gcnn_capi.hip, after gcnn_group.hpp; the group twins are in k_prenorm.hpp.
//
// One call is what GCNN.pretrain does with a batch, without its host read: the save_for_backward = 2 forward (layers >= 5), the
// two statistics passes of gcnn_prenorm_stats (the same plan, so the same fp64 sums) and, in the second pass's final, the
// Chan merge into the caller's state (k_stats_fold).  At most 7 + 1 + 4 launches, all through GCNN_LAUNCH: a group call records
// each member's call and sends the members' stages out together (gcnn_group.hpp).

// GCNN.pretrain's sample_count: the elements the layer absorbs from a batch of these dims
static double prenorm_count(const gcnn_dims* d, int layer) {
    if (layer <= 4) {
        const int n[5] = {d->n_cons, d->n_cons_edges, d->n_vars, d->n_cuts, d->n_cut_edges};
        return (double)n[layer];
    }
    const int conv = (layer - 5) >> 1;
    const int n_recv[3] = {d->n_cons, d->n_vars, d->n_cuts}, n_edge[3] = {d->n_cons_edges, d->n_cons_edges, d->n_cut_edges};
    return (double)(((layer - 5) & 1) ? n_recv[conv] : n_edge[conv]) * EMB;
}

static int prenorm_merge_enqueue(const gcnn_dims* d, const float* p, const float* cons_feats, const float* var_feats,
                                 const float* cut_feats, const gcnn_graph* cg, const gcnn_graph* kg, float* workspace,
                                 size_t workspace_floats, int32_t layer, void* state, hipStream_t st) {
    if (layer < 0 || layer > 10 || !state || ((uintptr_t)state & 7)) return GCNN_E_BADARG;
    layout_init();
    int rc = check_common(d, p, cg, kg, workspace, workspace_floats);
    if (rc) return rc;
    if (prenorm_count(d, layer) <= 0.0) return 0;   // nothing to absorb: the state stays as it is
    if (layer >= 5) {   // the two-layer form, which also stores A; its scores go to the (unused) gradient rows of O1
        Work w; carve(d, workspace, &w);
        if ((rc = forward_impl(d, p, cons_feats, var_feats, cut_feats, cg, kg, workspace, workspace_floats, w.g.O1, 2, nullptr, 0.f, st)))
            return rc;
    }
    StatPlan s;
    if ((rc = prenorm_plan(d, p, cons_feats, var_feats, cut_feats, cg, kg, workspace, workspace_floats, layer, &s))) return rc;
    PrenormState* S = (PrenormState*)state;
    if (s.x.n_seg > 0) {
        ProfScope prof("k_prenorm_expand_ptr", st);
        GCNN_LAUNCH(k_expand_ptr, dim3(expand_grid(s.x)), dim3(256), 0, st, s.x);
        LAUNCHCHK();
    }
    StatArgs a = s.a;
    StatFoldArgs f = {a.partial, s.grid, s.units, s.count, S->mean64, nullptr};   // pass 1: the batch mean (fp64) into the state
    for (int pass = 0; pass < 2; ++pass) {
        {
            ProfScope prof("k_prenorm_stats", st);
            GCNN_LAUNCH(k_stats, dim3(s.grid), dim3(256), 0, st, a);
            LAUNCHCHK();
        }
        {
            ProfScope prof(pass ? "k_prenorm_stats_fold<merge>" : "k_prenorm_stats_fold", st);
            GCNN_LAUNCH(k_stats_fold, dim3(1), dim3(64), 0, st, f);
            LAUNCHCHK();
        }
        a.mean = S->mean64;   // pass 2: the centred second moment around it, then the merge
        f.out = nullptr;
        f.state = S;
    }
    return 0;
}

extern "C" int gcnn_prenorm_merge(const gcnn_dims* d, const float* p, const float* cons_feats, const float* var_feats,
                                  const float* cut_feats, const gcnn_graph* cg, const gcnn_graph* kg, float* workspace,
                                  size_t workspace_floats, int32_t layer, void* state, void* stream) {
    return prenorm_merge_enqueue(d, p, cons_feats, var_feats, cut_feats, cg, kg, workspace, workspace_floats, layer, state,
                                 (hipStream_t)stream);
}

extern "C" int gcnn_group_prenorm_merge(int32_t n_members, const gcnn_group_member* members, const int32_t* layers,
                                        void* const* states, void* host_staging, void* device_table, size_t table_bytes,
                                        void* stream) {
    if (!layers || !states) return GCNN_E_BADARG;
    int rc = group_check(n_members, members, host_staging, device_table, table_bytes, false, states);
    if (rc) return rc;
    for (int i = 0; i < n_members; ++i)
        if (layers[i] < 0 || layers[i] > 10) return GCNN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    return group_run(n_members, members, host_staging, device_table, [&](int i) {
        const gcnn_group_member& m = members[i];
        return prenorm_merge_enqueue(&m.dims, m.params, m.cons_feats, m.var_feats, m.cut_feats, &m.cons_graph, &m.cut_graph,
                                     m.workspace, m.workspace_floats, layers[i], states[i], st);
    }, st);
}
