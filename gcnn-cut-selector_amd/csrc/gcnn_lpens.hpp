// gcnn_lpens.hpp -- host side of the round of ONE resident LP scored by an ensemble (include/gcnn_hip.h:
// gcnn_lp_round_ensemble_layout_for, gcnn_lp_round_ensemble): 1..GCNN_GROUP_MAX models (the reference trains five seeds per problem,
// model_trainer.py:38-49) score the state of one round, with its optional removal and append, and the plugin's ranking or
// parallelism filter (model_evaluator.py:82-154) runs once over the fp32 mean of their scores.  Nothing in a resident LP belongs
// to a model, so this is pure composition, and it launches no kernel of its own: the round with edits of gcnn_lpremove.hpp
// (lpes_member's LpEdit, lpe_plan, lpe_check, lpe_enqueue_edits), the round's two state launches and its tail (gcnn_lpres.hpp:
// lpr_run, whose one forward pass is replaced through LprForward), the members' forward passes as ONE group (gcnn_group.hpp:
// group_check, group_plan, group_issue over group_member_step -- every member reads the SAME feature arrays, the resident
// constraint graph and the round's cut graph, and has its own parameters, workspace and score row) and gcnn_ensemble.hpp's
// launch_ens_mean.  Included at the end of gcnn_capi.hip behind gcnn_group.hpp, gcnn_ensemble.hpp, gcnn_lpremove.hpp and
// gcnn_lpedits.hpp.  It spells no launch name: every launch goes out under the name its own file gives it.
//
// The arena: the solo call's arena of this round and these edits, unchanged (the upload in front; its download block and forward
// workspace stay unused), then the call's own download block -- the solo block with the mean where the scores were -- and, 256-byte
// aligned behind it so that ONE copy brings both home, the members' rows [M][member_stride]; then the M forward workspaces and the
// launch tables of the group.

struct LpensCall {
    LpEdit e;
    LpePlan P;
    gcnn_lp_round_ensemble_layout L;
    gcnn_group_member mem[GCNN_GROUP_MAX];
    const float* rows[GCNN_GROUP_MAX];
    GroupPlan plan;
    char* arena;
    void* staging;
};

static int lpens_layout(const gcnn_lp_rounds_edit_member* m, int mode, int n_models, LpEdit* e, LpePlan* P,
                        gcnn_lp_round_ensemble_layout* L) {
    if (!m || !L || n_models < 1 || n_models > GCNN_GROUP_MAX || mode < GCNN_IBATCH_SCORES || mode > GCNN_IBATCH_SELECT) return GCNN_E_BADARG;
    const int rc = lpes_member(*m, mode, e, P);       // the member's flags, n_forced against the mode, the solo limits
    if (rc) return rc;
    memset(L, 0, sizeof(*L));
    const gcnn_dims sd = lp_state_dims(&P->after);
    const size_t M = n_models, row = al16(4 * (size_t)sd.n_cuts);
    const size_t ws = sizeof(float) * gcnn_workspace_floats(&sd);
    L->round = P->RL;
    L->n_models = n_models;
    L->in_bytes = P->in_bytes; L->round_off = P->round_rel;
    L->solo_out_bytes = P->out_bytes; L->flags_off = P->flags_off; L->append_flags_off = P->append_flags_off;
    Carver c{al256(P->arena_bytes)};
    L->solo_arena_bytes = c.off;
    L->out_base = c.take(P->out_bytes, 256);
    L->member_off = c.take(M * row, 256) - L->out_base;
    L->member_stride = row;
    L->out_bytes = L->member_off + M * row;           // the download reaches over the members' rows
    for (size_t i = 0; i < M; ++i) L->ws_off[i] = c.take(ws, 256);
    L->table_bytes = group_table_bytes(n_models);
    L->table_off = c.take(L->table_bytes, 256);
    L->arena_bytes = c.off;
    return 0;
}

extern "C" int gcnn_lp_round_ensemble_layout_for(const gcnn_lp_rounds_edit_member* round, int32_t mode, int32_t n_models,
                                                 gcnn_lp_round_ensemble_layout* layout) {
    LpEdit e; LpePlan P;
    return layout_out(layout, [&](gcnn_lp_round_ensemble_layout* l) { return lpens_layout(round, mode, n_models, &e, &P, l); });
}

// The host half behind the checks: the members over the state this round will build (the places lpr_run gives the round's feature
// arrays and cut graph in the round's arena), group_check's rules, and the recording of every member's forward pass into the
// staging buffer.  Nothing is enqueued.
static int lpens_prepare(LpensCall* c, const float* const* params, hipStream_t st) {
    const gcnn_lp_round_ensemble_layout& L = c->L;
    const gcnn_lp_round_layout& RL = c->P.RL;
    char* A = c->arena;
    char* round = A + L.round_off;
    char* out = A + L.out_base;
    const gcnn_dims sd = lp_state_dims(&c->P.after);
    const gcnn_lp_resident* res = c->e.resident;
    gcnn_graph kg; memset(&kg, 0, sizeof(kg));
    kg.l_ptr = (int*)(round + RL.dev_off[5]); kg.l_oth = (int*)(round + RL.dev_off[3]) + sd.n_cut_edges;
    kg.l_coef = (float*)(round + RL.dev_off[4]); kg.v_ptr = res->cons_graph.v_ptr;      // (v_*: never read, as in lpr_run)
    memset(c->mem, 0, sizeof(c->mem));
    for (int m = 0; m < L.n_models; ++m) {
        gcnn_group_member& g = c->mem[m];
        g.dims = sd; g.params = params[m];
        g.cons_feats = res->cons_feats; g.var_feats = (const float*)(round + RL.dev_off[1]); g.cut_feats = (const float*)(round + RL.dev_off[2]);
        g.cons_graph = res->cons_graph; g.cut_graph = kg;
        g.workspace = (float*)(A + L.ws_off[m]); g.workspace_floats = gcnn_workspace_floats(&sd);
        g.scores = (float*)(out + L.member_off + (size_t)m * L.member_stride);
        c->rows[m] = g.scores;
    }
    const int rc = group_check(L.n_models, c->mem, c->staging, A + L.table_off, L.table_bytes, false);
    if (rc) return rc;
    return group_plan(L.n_models, c->mem, c->staging, [&](int i) { return group_member_step(c->mem[i], false, st); }, &c->plan);
}

// What lpr_run enqueues in place of its forward pass: the launch tables (the second upload), every stage of the M forward passes as
// one launch per distinct kernel -- a state without constraint rows or columns: the members' solo launches -- and the mean into
// the download's score slot.
static int lpens_forward(void* self, hipStream_t st) {
    LpensCall& c = *(LpensCall*)self;
    const gcnn_lp_round_ensemble_layout& L = c.L;
    char* A = c.arena;
    const int rc = group_issue(L.n_models, c.mem, c.staging, A + L.table_off, c.plan,
                               [&](int i) { return group_member_step(c.mem[i], false, st); }, st);
    if (rc) return rc;
    return launch_ens_mean(c.rows, L.n_models, c.mem[0].dims.n_cuts, (float*)(A + L.out_base + c.P.RL.out_off[0]), st);
}

extern "C" int gcnn_lp_round_ensemble(const gcnn_lp_rounds_edit_member* round, int32_t mode, int32_t n_models, const float* const* params,
                                      const void* host_in, void* host_out, void* arena, size_t arena_bytes, void* host_staging,
                                      double p_max, double p_max_ub, void* stream) {
    static thread_local LpensCall call;
    LpensCall& c = call;
    int rc = lpens_layout(round, mode, n_models, &c.e, &c.P, &c.L);
    if (rc) return rc;
    const gcnn_lp_round_ensemble_layout& L = c.L;
    if (!params || !host_staging || ((uintptr_t)host_staging & 15)) return GCNN_E_BADARG;
    for (int m = 0; m < n_models; ++m) {
        if (!params[m]) return GCNN_E_BADARG;
        for (int q = 0; q < m; ++q) if (params[q] == params[m]) return GCNN_E_BADARG;
    }
    if (!arena || ((uintptr_t)arena & 255) || arena_bytes < L.arena_bytes) return GCNN_E_BADARG;
    c.e.params = params[0];                           // (the member's own field is not read)
    const int want = mode != GCNN_IBATCH_SCORES;
    // everything the solo call of this round refuses, unchanged
    if ((rc = lpe_check(c.e, c.P, host_in, host_out, arena, L.solo_arena_bytes, want, p_max, p_max_ub))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    c.arena = A; c.staging = host_staging;
    const bool scores = c.P.after.n_cuts > 0;         // a round without cuts scores nothing: it only refreshes the resident columns
    if (scores && (rc = lpens_prepare(&c, params, st))) return rc;                      // host work only
    char* round_arena = A + L.round_off;
    char* out = A + L.out_base;
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));          // upload 1: the list | the block | the round | forced rows
    const LpeAt edits = {A, out, A + c.P.rem_scratch_rel, A + c.P.app_scratch_rel, nullptr, nullptr, nullptr, nullptr};
    if ((rc = lpe_enqueue_edits(c.e, c.P, edits, st))) return rc;
    const LprAt at = {round_arena + c.P.RL.dev_off[0], out};
    const LprForward fwd = {lpens_forward, &c};
    if ((rc = lpr_run(&c.P.after, c.P.RL, c.e.present, c.e.n_forced, c.e.resident, nullptr, nullptr, nullptr, round_arena, want, p_max,
                      p_max_ub, stream, &at, &fwd)))
        return rc;
    // ONE download: mean | order | flags | n_kept | LP flags | cut_index | the edits' flag words | members
    HIPCHK(hipMemcpyAsync(host_out, out, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
