// hostsan_refusals.inc -- included by hostsan_main.hip, inside its namespace.  Entry points that launch, with argument sets they
// refuse before their first HIP call: the practice of the *_build tests' test_limits_and_bad_arguments_without_a_device, in C++.
// A record is (entry, variant, the code the header promises); the call's own code has to equal it, or the run stops there.
// Every pointer is the fake one -- never dereferenced by a call that refuses in time -- or null; layouts come from the library's
// own *_layout_for on a small valid base case.
// Fake buffers that a call compares for overlap (the group calls, the round ensemble) lie far apart, so that the base case passes
// every check and a refusal is the variant's own.

enum Variant {
    V_SHORT_ARENA = 0, V_MISALIGNED_ARENA, V_PMAX_NAN, V_PMAX_INF, V_NULL_IN, V_NULL_OUT, V_NULL_PARAMS, V_NULL_ARENA, V_N_ZERO,
    V_N_OVER, V_NEGATIVE_DIM, V_NULL_DIMS, V_NULL_STAGING, V_BAD_MODE, V_MODELS_ZERO, V_MODELS_OVER, V_SHORT_WORKSPACE, V_NULL_MISC
};

struct Refuse {
    int v;
    void* fake(int k = 0) const { return (void*)(FAKE + 4096 * (uintptr_t)k); }
    double p_max() const { return v == V_PMAX_NAN ? (double)NAN : v == V_PMAX_INF ? (double)INFINITY : 0.1; }
    void* in() const { return v == V_NULL_IN ? nullptr : fake(1); }
    void* out() const { return v == V_NULL_OUT ? nullptr : fake(2); }
    float* params() const { return v == V_NULL_PARAMS ? nullptr : (float*)fake(3); }
    void* staging() const { return v == V_NULL_STAGING ? nullptr : fake(5); }
    void* arena() const { return v == V_NULL_ARENA ? nullptr : v == V_MISALIGNED_ARENA ? (void*)((char*)fake(8) + 16) : fake(8); }
    size_t size(size_t need) const { return v == V_SHORT_ARENA ? need - 1 : need; }
    int count(int n, int max) const { return v == V_N_ZERO ? 0 : v == V_N_OVER ? max + 1 : n; }
    int mode(int m) const { return v == V_BAD_MODE ? 3 : m; }
    int models(int m) const { return v == V_MODELS_ZERO ? 0 : v == V_MODELS_OVER ? GCNN_GROUP_MAX + 1 : m; }
};

static const gcnn_dims R_DIMS = {5, 6, 3, 7, 4};
static gcnn_lp_dims r_lp_dims() {
    gcnn_lp_dims d; memset(&d, 0, sizeof(d));
    d.n_rows = 4; d.n_cols = 6; d.n_cuts = 3; d.row_nnz = 9; d.cut_nnz = 5; d.n_model_vars = 6; d.n_state_rows = 5; d.n_state_edges = 11;
    d.infinity = 1e20; d.sum_epsilon = 1e-6; d.obj_norm = 1.0;
    return d;
}

static void refusal_case(Reader& r) {
    const int entry = r.i(), variant = r.i(), want = r.i();
    const Refuse R{variant};
    const bool neg = variant == V_NEGATIVE_DIM, nod = variant == V_NULL_DIMS;
    gcnn_dims d1 = R_DIMS, d2[GCNN_IBATCH_MAX + 1];
    for (gcnn_dims& d : d2) d = R_DIMS;
    gcnn_lp_dims l1 = r_lp_dims(), l2[GCNN_IBATCH_MAX + 1];
    for (gcnn_lp_dims& d : l2) d = l1;
    gcnn_hybrid_dims h2[GCNN_IBATCH_MAX + 1];
    for (gcnn_hybrid_dims& h : h2) { memset(&h, 0, sizeof(h)); h.n_cols = 6; h.n_cuts = 3; h.cut_nnz = 5; h.infinity = 1e20; }
    if (neg) { d1.n_cuts = -1; d2[1].n_cuts = -1; l1.n_cuts = -1; l2[1].n_cuts = -1; h2[1].n_cuts = -1; }
    const int32_t model_of[2] = {0, 1};
    const float* pp[GCNN_GROUP_MAX + 1];
    for (const float*& p : pp) p = (const float*)R.fake(3);
    const float* const* params2 = variant == V_NULL_PARAMS ? nullptr : pp;
    const gcnn_dims* D1 = nod ? nullptr : &d1; const gcnn_dims* D2 = nod ? nullptr : d2;
    const gcnn_lp_dims* L1 = nod ? nullptr : &l1; const gcnn_lp_dims* L2 = nod ? nullptr : l2;
    const gcnn_hybrid_dims* H2 = nod ? nullptr : h2;
    const gcnn_dims good = R_DIMS; const gcnn_lp_dims lgood = r_lp_dims();
    const gcnn_dims good2[2] = {R_DIMS, R_DIMS}; const gcnn_lp_dims lgood2[2] = {lgood, lgood};
    gcnn_hybrid_dims hgood2[2];
    for (gcnn_hybrid_dims& h : hgood2) { memset(&h, 0, sizeof(h)); h.n_cols = 6; h.n_cuts = 3; h.cut_nnz = 5; h.infinity = 1e20; }
    // the resident-LP calls: a resident LP, two sets of derived arrays and an append / a removal that fit the base LP
    gcnn_lp_resident res; memset(&res, 0, sizeof(res));
    { void** q = (void**)&res; for (int i = 0; i < 9; ++i) q[i] = R.fake(20 + i); }
    res.cons_graph.l_ptr = (const int32_t*)R.fake(30); res.cons_graph.l_oth = (const int32_t*)R.fake(31); res.cons_graph.l_coef = (const float*)R.fake(32);
    res.cons_graph.v_ptr = (const int32_t*)R.fake(33); res.cons_graph.v_oth = (const int32_t*)R.fake(34); res.cons_graph.v_coef = (const float*)R.fake(35);
    gcnn_lp_rows_set set_a, set_b;
    { void** q = (void**)&set_a; for (int i = 0; i < 10; ++i) q[i] = R.fake(40 + i); }
    { void** q = (void**)&set_b; for (int i = 0; i < 10; ++i) q[i] = R.fake(60 + i); }
    const gcnn_lp_append_dims blk = {2, 4, 3, 6, 1, 2, 2, 5};
    const gcnn_lp_remove_dims gone = {1, 2, 1, 2, 0, 0, 2, 5};
    const int present = variant == V_BAD_MODE ? 16 : 3;
    int32_t* I = (int32_t*)R.fake(80); double* Dp = (double*)R.fake(81);
    int rc = INT32_MIN;
    switch (entry) {
    case 0: { gcnn_infer_layout L; gcnn_infer_layout_for(&good, &L);
        rc = gcnn_infer(D1, R.params(), R.in(), R.out(), R.arena(), R.size(L.arena_bytes), 1, nullptr); break; }
    case 1: { gcnn_select_layout L; gcnn_infer_select_layout_for(&good, 1, 2, &L);
        rc = gcnn_infer_select(D1, 1, 2, R.params(), R.in(), R.out(), R.arena(), R.size(L.infer.arena_bytes), R.p_max(), 0.5, nullptr); break; }
    case 2: { gcnn_ibatch_layout L; gcnn_infer_batch_layout_for(2, good2, nullptr, nullptr, 2, &L);
        rc = gcnn_infer_batch(R.count(2, GCNN_IBATCH_MAX), D2, nullptr, nullptr, R.mode(2), R.params(), R.in(), R.out(), R.arena(),
                              R.size(L.arena_bytes), R.p_max(), 0.5, nullptr); break; }
    case 3: { gcnn_lp_layout L; gcnn_lp_layout_for(&lgood, -1, 0, &L);
        rc = gcnn_lp_infer(L1, R.params(), R.in(), R.out(), R.arena(), R.size(L.arena_bytes), 1, nullptr); break; }
    case 4: { gcnn_lp_layout L; gcnn_lp_layout_for(&lgood, 1, 2, &L);
        rc = gcnn_lp_infer_select(L1, 1, 2, R.params(), R.in(), R.out(), R.arena(), R.size(L.arena_bytes), R.p_max(), 0.5, nullptr); break; }
    case 5: { gcnn_lp_batch_layout* L = fresh<gcnn_lp_batch_layout>(); gcnn_lp_batch_layout_for(2, lgood2, nullptr, nullptr, 2, L);
        rc = gcnn_lp_batch(R.count(2, GCNN_IBATCH_MAX), L2, nullptr, nullptr, R.mode(2), R.params(), R.in(), R.out(), R.arena(),
                           R.size(L->arena_bytes), R.p_max(), 0.5, nullptr); free(L); break; }
    case 6: { gcnn_hybrid_layout* L = fresh<gcnn_hybrid_layout>(); gcnn_hybrid_layout_for(2, hgood2, nullptr, nullptr, 2, L);
        const size_t need = L->arena_bytes; free(L);
        rc = gcnn_hybrid_select(R.count(2, GCNN_IBATCH_MAX), H2, nullptr, nullptr, R.mode(2), R.in(), R.out(), R.arena(), R.size(need),
                                R.p_max(), 0.5, nullptr); break; }
    case 7: { gcnn_lp_collect_layout L; gcnn_lp_collect_layout_for(&lgood, 1, 2, &L);
        rc = gcnn_lp_collect(L1, 1, 2, R.in(), R.out(), R.arena(), R.size(L.arena_bytes), R.p_max(), 0.5, nullptr); break; }
    case 8: { gcnn_mbatch_layout* L = fresh<gcnn_mbatch_layout>(); gcnn_infer_models_layout_for(2, good2, nullptr, nullptr, 2, 2, model_of, L);
        rc = gcnn_infer_models(R.count(2, GCNN_IBATCH_MAX), D2, nullptr, nullptr, R.mode(2), R.models(2), model_of, params2, R.in(), R.out(),
                               R.arena(), R.size(L->u.arena_bytes), R.staging(), R.p_max(), 0.5, nullptr); free(L); break; }
    case 9: { gcnn_lp_models_layout* L = fresh<gcnn_lp_models_layout>(); gcnn_lp_models_layout_for(2, lgood2, nullptr, nullptr, 2, 2, model_of, L);
        rc = gcnn_lp_models(R.count(2, GCNN_IBATCH_MAX), L2, nullptr, nullptr, R.mode(2), R.models(2), model_of, params2, R.in(), R.out(),
                            R.arena(), R.size(L->lp.arena_bytes), R.staging(), R.p_max(), 0.5, nullptr); free(L); break; }
    case 10: { gcnn_ensemble_layout* L = fresh<gcnn_ensemble_layout>(); gcnn_infer_ensemble_layout_for(&good, 1, 2, 2, 2, L);
        rc = gcnn_infer_ensemble(D1, 1, 2, R.mode(2), R.models(2), params2, R.in(), R.out(), R.arena(), R.size(L->u.arena_bytes), R.staging(),
                                 R.p_max(), 0.5, nullptr); free(L); break; }
    case 11: { gcnn_lp_ensemble_layout* L = fresh<gcnn_lp_ensemble_layout>(); gcnn_lp_ensemble_layout_for(&lgood, 1, 2, 2, 2, L);
        rc = gcnn_lp_ensemble(L1, 1, 2, R.mode(2), R.models(2), params2, R.in(), R.out(), R.arena(), R.size(L->lp.arena_bytes), R.staging(),
                              R.p_max(), 0.5, nullptr); free(L); break; }
    case 12: { gcnn_ensemble_layout* L = fresh<gcnn_ensemble_layout>(); gcnn_infer_ensemble_batch_layout_for(2, good2, nullptr, nullptr, 2, 2, L);
        rc = gcnn_infer_ensemble_batch(R.count(2, GCNN_IBATCH_MAX), D2, nullptr, nullptr, R.mode(2), R.models(2), params2, R.in(), R.out(),
                                       R.arena(), R.size(L->u.arena_bytes), R.staging(), R.p_max(), 0.5, nullptr); free(L); break; }
    case 13: { gcnn_lp_ensemble_layout* L = fresh<gcnn_lp_ensemble_layout>(); gcnn_lp_ensemble_batch_layout_for(2, lgood2, nullptr, nullptr, 2, 2, L);
        rc = gcnn_lp_ensemble_batch(R.count(2, GCNN_IBATCH_MAX), L2, nullptr, nullptr, R.mode(2), R.models(2), params2, R.in(), R.out(),
                                    R.arena(), R.size(L->lp.arena_bytes), R.staging(), R.p_max(), 0.5, nullptr); free(L); break; }
    case 14: {   // gcnn_select_cuts: counts, thresholds, the 4,096-cut limit, missing buffers, a short workspace
        const size_t ws = gcnn_select_workspace_bytes(3, 0, 3);
        rc = gcnn_select_cuts((const float*)R.in(), (const int32_t*)R.fake(1), (const int32_t*)R.fake(1), (const float*)R.fake(1), nullptr,
                              R.count(1, 0) /* V_N_OVER: 1 */, neg ? -1 : 3, variant == V_BAD_MODE ? 4097 : 3, 6, nullptr, nullptr, nullptr, nullptr, 0,
                              R.p_max(), 0.5, (int32_t*)R.out(), variant == V_NULL_MISC ? nullptr : (int32_t*)R.fake(4), R.arena(),
                              variant == V_SHORT_WORKSPACE ? ws - 1 : ws, nullptr);
        break; }
    case 15:     // gcnn_rank_deviations
        rc = gcnn_rank_deviations((const int32_t*)R.in(), R.count(2, 0), (const float*)R.fake(1), variant == V_NULL_MISC ? nullptr : (const double*)R.fake(1),
                                  (const float*)R.params(), R.models(1), nullptr, (const int32_t*)R.fake(2), variant == V_NULL_MISC ? 1 : 0,
                                  (int32_t*)R.out(), nullptr);
        break;
    case 16: {   // gcnn_collate
        gcnn_collate_job job = {R.fake(1), R.fake(2), neg ? -1 : 0, variant == V_BAD_MODE ? 0 : 1, -1, 0};
        rc = gcnn_collate(variant == V_NULL_MISC ? nullptr : &job, variant == V_N_OVER ? 25 : 1, (const int64_t*)R.in(), (const int64_t*)R.out(),
                          variant == V_N_ZERO ? -1 : 2, 8, nullptr);
        break; }
    case 17: case 18: case 19: {   // gcnn_forward / gcnn_forward_loss / gcnn_backward
        gcnn_graph g; memset(&g, 0, sizeof(g));
        const gcnn_graph* G = variant == V_NULL_MISC ? nullptr : &g;
        const size_t ws = gcnn_workspace_floats(&good);
        float* W = (float*)R.arena();   // V_MISALIGNED_ARENA: 16 bytes off a 256-byte boundary is still 16-byte aligned, so not a refusal here
        const size_t wf = (variant == V_SHORT_WORKSPACE || variant == V_SHORT_ARENA) ? ws - 1 : ws;
        if (entry == 17) rc = gcnn_forward(D1, R.params(), (const float*)R.fake(1), (const float*)R.fake(1), (const float*)R.fake(1), G, G, W, wf, (float*)R.out(), 0, nullptr);
        if (entry == 18) rc = gcnn_forward_loss(D1, R.params(), (const float*)R.fake(1), (const float*)R.fake(1), (const float*)R.fake(1), G, G, W, wf, (float*)R.out(),
                                                (const float*)R.in(), 1.0f, nullptr);
        if (entry == 19) rc = gcnn_backward(D1, R.params(), (const float*)R.fake(1), (const float*)R.fake(1), (const float*)R.fake(1), G, G, W, wf, (const float*)R.in(),
                                            (float*)R.out(), nullptr, nullptr, nullptr, nullptr);
        break; }
    case 20: case 21: {   // gcnn_group_forward / gcnn_group_train_step
        gcnn_group_member mem[GCNN_GROUP_MAX + 1];
        const size_t ws = gcnn_workspace_floats(&good);
        for (int i = 0; i <= GCNN_GROUP_MAX; ++i) {
            gcnn_group_member& m = mem[i]; memset(&m, 0, sizeof(m));
            m.dims = (neg && i == 1) ? d1 : good; m.params = R.params();
            m.workspace = (float*)((char*)R.fake(16) + ((size_t)(i + 1) << 32));   /* 4 GiB apart: no member's workspace meets another's */ m.workspace_floats = variant == V_SHORT_WORKSPACE ? ws - 1 : ws;
            m.scores = variant == V_NULL_OUT ? nullptr : (float*)((char*)R.fake(16) + ((size_t)1 << 30) + 4096 * i);   /* clear of the parameters, which every member reads */
            m.targets = (const float*)R.fake(1); m.loss_scale = 1.0f;   /* training: its own gradients, far from everything else */
            m.grads = (float*)((char*)R.fake(16) + ((size_t)(i + 1) << 32) + ((size_t)1 << 31));
        }
        size_t tb = 0; gcnn_group_table_bytes(2, &tb);
        auto fn = entry == 20 ? gcnn_group_forward : gcnn_group_train_step;
        rc = fn(R.count(2, GCNN_GROUP_MAX), nod ? nullptr : mem, R.staging(), R.arena(), R.size(tb), nullptr);
        break; }
    // ---- the single ops, the optimiser, the metrics, the graph plan: null pointers with a positive count, negative counts
    case 22: rc = gcnn_seg_sum_f32((const float*)R.fake(1), variant == V_NULL_IN ? nullptr : I, nullptr, neg ? -1 : 4, (float*)R.out(), nullptr); break;
    case 23: rc = gcnn_seg_bcast_f32((const float*)R.in(), variant == V_NULL_MISC ? nullptr : I, nullptr, neg ? -1 : 4, (float*)R.fake(2), nullptr); break;
    case 24: rc = gcnn_linear_fwd((const float*)R.in(), nullptr, R.params(), variant == V_NULL_MISC ? (const float*)R.fake(4) : nullptr, nullptr, nullptr,
                                  variant == V_NULL_STAGING ? (const float*)R.fake(5) : nullptr, nullptr, 1, (float*)R.out(), neg ? -1 : 4, nullptr); break;
    case 25: rc = gcnn_linear_bwd((float*)R.in(), nullptr, R.params(), nullptr, (float*)R.out(), 0, nullptr, variant == V_NULL_MISC ? (float*)R.fake(4) : nullptr,
                                  0, neg ? -1 : 4, nullptr); break;
    case 26: rc = gcnn_conv_edge_fwd(variant == V_NULL_MISC ? nullptr : I, variant == V_NULL_IN ? nullptr : I, (const float*)R.fake(1), neg ? -1 : 4,
                                     variant == V_N_ZERO ? -1 : 6, R.params(), (const float*)R.fake(2), (const float*)R.fake(3), (const float*)R.fake(4),
                                     (const float*)R.fake(5), (const float*)R.fake(6), (float*)R.out(), nullptr, 0, nullptr); break;
    case 27: rc = gcnn_conv_edge_bwd_recv((const float*)R.in(), (const float*)R.fake(1), R.params(), neg ? -1 : 4, (float*)R.out(), nullptr); break;
    case 28: { int32_t parts = 0;
        rc = gcnn_conv_edge_bwd_send(I, variant == V_NULL_IN ? nullptr : I, (const float*)R.fake(1), neg ? -1 : 4, variant == V_N_ZERO ? -1 : 6, R.params(),
                                     (const float*)R.fake(2), (const float*)R.fake(3), (const float*)R.fake(4), (const float*)R.fake(5), (const float*)R.fake(6),
                                     (const float*)R.fake(7), (float*)R.out(), (float*)R.fake(9), variant == V_NULL_MISC ? nullptr : &parts, 0, nullptr);
        break; }
    case 29: rc = gcnn_adam_step(R.params(), (const float*)R.in(), (float*)R.out(), (float*)R.arena(), neg ? -1 : 8, 1e-3f, 0.9f, 0.999f, 1e-7f, nullptr, 0, nullptr); break;
    case 30: rc = gcnn_adam_step_dev(R.params(), (const float*)R.in(), (float*)R.out(), (float*)R.arena(), neg ? -1 : 8,
                                     variant == V_NULL_MISC ? nullptr : (float*)R.fake(4), nullptr, 0, nullptr); break;
    case 31: rc = gcnn_mse_loss((const float*)R.in(), (const float*)R.params(), neg ? -1 : 8, 1.0f, (float*)R.out(), nullptr, nullptr); break;
    case 32: rc = gcnn_ranking_metric((const float*)R.in(), (const float*)R.params(), variant == V_NULL_MISC ? nullptr : I, neg ? -1 : 2,
                                      variant == V_BAD_MODE ? 4097 : 8, variant == V_NULL_OUT ? nullptr : (const float*)R.fake(2), variant == V_N_ZERO ? -1 : 3,
                                      (float*)R.fake(3), nullptr, nullptr, 1.0f, variant == V_NULL_STAGING ? (float*)R.fake(5) : nullptr, nullptr); break;
    case 33: rc = gcnn_ensemble_mean(params2, R.models(2), neg ? -1 : 8, (float*)R.out(), nullptr); break;
    case 34: rc = gcnn_graph_check(variant == V_NULL_IN ? nullptr : I, neg ? -1 : 6, 4, 5, (int32_t*)R.out(), nullptr); break;
    case 35: { const size_t tb = gcnn_graph_temp_bytes(6);
        rc = gcnn_graph_build(variant == V_NULL_IN ? nullptr : I, (const float*)R.fake(1), neg ? -1 : 6, variant == V_N_ZERO ? -1 : 4, 5, 0,
                              variant == V_NULL_OUT ? nullptr : I, I, (float*)R.fake(2), variant == V_NULL_MISC ? nullptr : I, I, (float*)R.fake(3), nullptr,
                              R.arena(), variant == V_SHORT_WORKSPACE ? tb - 1 : tb, nullptr);
        break; }
    case 36: case 37: {   // gcnn_prenorm_stats / gcnn_prenorm_merge
        gcnn_graph g; memset(&g, 0, sizeof(g));
        const gcnn_graph* G = variant == V_NULL_MISC ? nullptr : &g;
        const size_t ws = gcnn_workspace_floats(&good);
        float* W = (float*)R.arena();
        const size_t wf = variant == V_SHORT_WORKSPACE ? ws - 1 : ws;
        const int layer = variant == V_BAD_MODE ? 11 : 0;
        if (entry == 36) rc = gcnn_prenorm_stats(D1, R.params(), (const float*)R.fake(1), (const float*)R.fake(1), (const float*)R.fake(1), G, G, W, wf, layer,
                                                 (double*)R.out(), nullptr);
        else rc = gcnn_prenorm_merge(D1, R.params(), (const float*)R.fake(1), (const float*)R.fake(1), (const float*)R.fake(1), G, G, W, wf, layer, R.out(), nullptr);
        break; }
    case 38: {   // gcnn_group_prenorm_merge
        gcnn_group_member mem[GCNN_GROUP_MAX + 1];
        const size_t ws = gcnn_workspace_floats(&good);
        int32_t layers[GCNN_GROUP_MAX + 1]; void* states[GCNN_GROUP_MAX + 1];
        for (int i = 0; i <= GCNN_GROUP_MAX; ++i) {
            gcnn_group_member& m = mem[i]; memset(&m, 0, sizeof(m));
            m.dims = (neg && i == 1) ? d1 : good; m.params = R.params();
            m.workspace = (float*)((char*)R.fake(16) + ((size_t)(i + 1) << 32)); m.workspace_floats = variant == V_SHORT_WORKSPACE ? ws - 1 : ws;
            layers[i] = (variant == V_BAD_MODE && i == 1) ? 11 : 0;
            states[i] = (variant == V_NULL_OUT && i == 1) ? nullptr : (char*)R.fake(16) + ((size_t)1 << 30) + 4096 * i + (variant == V_NULL_MISC ? 4 : 0);
        }
        size_t tb = 0; gcnn_group_table_bytes(2, &tb);
        rc = gcnn_group_prenorm_merge(R.count(2, GCNN_GROUP_MAX), nod ? nullptr : mem, variant == V_NULL_IN ? nullptr : layers,
                                      variant == V_NULL_PARAMS ? nullptr : states, R.staging(), R.arena(), R.size(tb), nullptr);
        break; }
    // ---- the state from a snapshot, and the calls on a resident LP
    case 39: { gcnn_lp_layout L; gcnn_lp_layout_for(&lgood, -1, 0, &L);
        rc = gcnn_lp_state(L1, R.in(), R.arena(), variant == V_SHORT_WORKSPACE ? L.scratch_bytes - 1 : L.scratch_bytes, (float*)R.fake(1), I, (float*)R.fake(2),
                           (float*)R.fake(3), (float*)R.fake(4), I, (float*)R.fake(5), variant == V_NULL_MISC ? nullptr : I, (int32_t*)R.out(), nullptr);
        break; }
    case 40: { gcnn_lp_rows_layout L; gcnn_lp_rows_layout_for(&lgood, &L);
        rc = gcnn_lp_rows_build(L1, variant == V_NULL_IN ? nullptr : I, I, Dp, Dp, Dp, Dp, R.arena(), variant == V_SHORT_WORKSPACE ? L.bytes - 1 : L.bytes, nullptr);
        break; }
    case 41: { gcnn_lp_round_layout L; gcnn_lp_round_layout_for(&lgood, 3, -1, 0, &L);
        rc = gcnn_lp_round(L1, present, variant == V_NULL_MISC ? nullptr : &res, R.params(), R.in(), R.out(), R.arena(), R.size(L.arena_bytes), 1, nullptr);
        break; }
    case 42: { gcnn_lp_round_layout L; gcnn_lp_round_layout_for(&lgood, 3, 1, 2, &L);
        rc = gcnn_lp_round_select(L1, present, 1, 2, variant == V_NULL_MISC ? nullptr : &res, R.params(), R.in(), R.out(), R.arena(), R.size(L.arena_bytes),
                                  R.p_max(), 0.5, nullptr);
        break; }
    case 43: { gcnn_lp_append_layout* L = fresh<gcnn_lp_append_layout>(); gcnn_lp_append_layout_for(&lgood, &blk, 3, -1, 0, L);
        rc = gcnn_lp_rows_append(L1, variant == V_NULL_MISC ? nullptr : &blk, I, I, Dp, Dp, Dp, Dp, variant == V_NULL_IN ? nullptr : &set_a,
                                 variant == V_NULL_OUT ? nullptr : &set_b, R.arena(), variant == V_SHORT_WORKSPACE ? L->scratch_bytes - 1 : L->scratch_bytes,
                                 I, nullptr);
        free(L); break; }
    case 44: { gcnn_lp_append_layout* L = fresh<gcnn_lp_append_layout>(); gcnn_lp_append_layout_for(&lgood, &blk, 3, 1, 2, L);
        rc = gcnn_lp_round_append(L1, variant == V_NULL_MISC ? nullptr : &blk, present, 1, 2, I, I, Dp, Dp, Dp, &set_a, &set_b, &res, R.params(), R.in(), R.out(),
                                  R.arena(), R.size(L->arena_bytes), 1, R.p_max(), 0.5, nullptr);
        free(L); break; }
    case 45: { gcnn_lp_remove_layout* L = fresh<gcnn_lp_remove_layout>(); gcnn_lp_remove_layout_for(&lgood, &gone, nullptr, 3, -1, 0, L);
        rc = gcnn_lp_rows_remove(L1, variant == V_NULL_MISC ? nullptr : &gone, I, I, I, Dp, Dp, Dp, (int32_t*)R.fake(90), (int32_t*)R.fake(91), (double*)R.fake(92),
                                 (double*)R.fake(93), (double*)R.fake(94), variant == V_NULL_IN ? nullptr : &set_a, variant == V_NULL_OUT ? nullptr : &set_b,
                                 R.arena(), variant == V_SHORT_WORKSPACE ? L->scratch_bytes - 1 : L->scratch_bytes, I, nullptr);
        free(L); break; }
    case 46: { gcnn_lp_remove_layout* L = fresh<gcnn_lp_remove_layout>(); gcnn_lp_remove_layout_for(&lgood, &gone, nullptr, 3, 1, 2, L);
        rc = gcnn_lp_round_remove(L1, variant == V_NULL_MISC ? nullptr : &gone, nullptr, present, 1, 2, I, I, Dp, Dp, Dp, (int32_t*)R.fake(90), (int32_t*)R.fake(91),
                                  (double*)R.fake(92), (double*)R.fake(93), (double*)R.fake(94), &set_a, nullptr, &set_b, &res, R.params(), R.in(), R.out(),
                                  R.arena(), R.size(L->arena_bytes), 1, R.p_max(), 0.5, nullptr);
        free(L); break; }
    case 47: case 48: {   // gcnn_lp_rounds / gcnn_lp_rounds_edit: counts, modes, thresholds, buffers, a member's dims
        gcnn_lp_rounds_member mem[GCNN_LP_ROUNDS_MAX + 1]; gcnn_lp_rounds_edit_member edit[GCNN_LP_ROUNDS_MAX + 1];
        gcnn_lp_resident many_res[GCNN_LP_ROUNDS_MAX + 1];
        for (int i = 0; i <= GCNN_LP_ROUNDS_MAX; ++i) {
            many_res[i] = res;
            { void** q = (void**)&many_res[i]; for (int k = 0; k < 9; ++k) q[k] = (char*)R.fake(100) + ((size_t)(9 * i + k) << 28); }
            memset(&mem[i], 0, sizeof(mem[i])); memset(&edit[i], 0, sizeof(edit[i]));
            mem[i].dims = edit[i].dims = (neg && i == 1) ? l1 : lgood;
            mem[i].present = edit[i].present = 3; mem[i].n_forced = edit[i].n_forced = 1; mem[i].n_forced_entries = edit[i].n_forced_entries = 2;
            mem[i].resident = edit[i].resident = &many_res[i]; mem[i].params = edit[i].params = R.params();
        }
        const int n = R.count(2, GCNN_LP_ROUNDS_MAX);
        if (entry == 47) { gcnn_lp_rounds_layout* L = fresh<gcnn_lp_rounds_layout>(); gcnn_lp_rounds_layout_for(2, mem, 2, L);
            const gcnn_lp_rounds_member* M = nod ? nullptr : mem;
            rc = gcnn_lp_rounds(n, M, R.mode(2), R.in(), R.out(), R.arena(), R.size(L->arena_bytes), R.staging(), R.p_max(), 0.5, nullptr); free(L); }
        else { gcnn_lp_rounds_edit_layout* L = fresh<gcnn_lp_rounds_edit_layout>(); gcnn_lp_rounds_edit_layout_for(2, edit, 2, L);
            const gcnn_lp_rounds_edit_member* M = nod ? nullptr : edit;
            rc = gcnn_lp_rounds_edit(n, M, R.mode(2), R.in(), R.out(), R.arena(), R.size(L->arena_bytes), R.staging(), R.p_max(), 0.5, nullptr); free(L); }
        break; }
    case 49: {   // gcnn_lp_round_ensemble
        // (everything the members read lies 1 GiB apart and far from the arena: the group's overlap rule must not be what refuses)
        auto far = [](int k) { return (void*)(0x100000000000ull + ((uintptr_t)k << 30)); };
        gcnn_lp_resident far_res = res;
        { void** q = (void**)&far_res; for (int i = 0; i < 9; ++i) q[i] = far(i); }
        far_res.cons_graph.l_ptr = (const int32_t*)far(10); far_res.cons_graph.l_oth = (const int32_t*)far(11); far_res.cons_graph.l_coef = (const float*)far(12);
        far_res.cons_graph.v_ptr = (const int32_t*)far(13); far_res.cons_graph.v_oth = (const int32_t*)far(14); far_res.cons_graph.v_coef = (const float*)far(15);
        for (int i = 0; i <= GCNN_GROUP_MAX; ++i) pp[i] = (variant == V_NULL_MISC && i == 1) ? nullptr : (const float*)far(20 + i);
        gcnn_lp_rounds_edit_member round; memset(&round, 0, sizeof(round));
        round.dims = neg ? l1 : lgood; round.present = 3; round.n_forced = 1; round.n_forced_entries = 2; round.resident = &far_res;
        gcnn_lp_rounds_edit_member ok = round; ok.dims = lgood;
        gcnn_lp_round_ensemble_layout* L = fresh<gcnn_lp_round_ensemble_layout>(); gcnn_lp_round_ensemble_layout_for(&ok, 2, 2, L);
        rc = gcnn_lp_round_ensemble(nod ? nullptr : &round, R.mode(2), R.models(2), params2, R.in(), R.out(), R.arena(), R.size(L->arena_bytes), R.staging(),
                                    R.p_max(), 0.5, nullptr);
        free(L); break; }
    default: fprintf(stderr, "hostsan: unknown refusal entry %d\n", entry); exit(3);
    }
    if (rc != want) { fprintf(stderr, "hostsan: refusal entry %d variant %d returned %d, expected %d\n", entry, variant, rc, want); exit(4); }
    emit(rc, nullptr, 0);
}
