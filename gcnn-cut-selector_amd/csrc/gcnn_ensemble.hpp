// gcnn_ensemble.hpp -- host side of the ensemble calls (include/gcnn_hip.h): gcnn_ensemble_mean, gcnn_infer_ensemble and
// gcnn_lp_ensemble -- ONE state scored by 1..GCNN_GROUP_MAX models (the reference trains five seeds per problem,
// model_trainer.py:38-49), their scores averaged in the caller's order (k_ensemble.hpp) and the plugin's ranking or parallelism
// filter (model_evaluator.py:82-154) run once over the mean.  Pure composition around that one kernel: gcnn_infer_batch's union of
// ONE state (gcnn_ibatch.hpp: ibatch_sums, union_layout, union_at, union_args, union_grid, union_tail; k_ib_unpack and the
// by-variable stage, recorded here as k_ens_unpack / k_ens_by_variable), the members' forward passes as ONE group (gcnn_group.hpp:
// group_check, group_plan, group_issue -- every member reads the SAME feature arrays and the same two graphs and has its own
// parameters, workspace and score row), k_ens_mean, then k_ib_rank (recorded as k_ens_rank) or launch_select over the mean, one
// download.  The LP form puts gcnn_lp_batch's two builder launches (gcnn_lpbatch.hpp: lpset_layout, lpset_fill, lpset_launch,
// lpset_at; recorded as k_ens_lp_stats / k_ens_lp_emit) in front of the same work.  Included from gcnn_capi.hip's list of host
// files, after gcnn_group.hpp, gcnn_ibatch.hpp and gcnn_lpbatch.hpp.  Kept apart so that its launch names form their own inventory
// (tests/test_ensemble_build.py).  Layout, host half, device half and the two whole calls (ens_layout, ens_prepare, ens_run, ens_call,
// lpens_call) take the number of states: the entry points here pass one, gcnn_ensbatch.hpp, included after this file, passes 1..64
// and its own tail for RANK mode; with one state every launch and every offset is what it was.
//
// The download: the union's output block (mean | order | n_kept | flags), then at member_off the members' rows [M][member_stride
// bytes], then in the LP form the LP flags and cut_index.  In the host form the rows lie at the start of the arena block behind the
// output block (dev_off[12], which also holds the M forward workspaces), so one copy brings both home.
#include "k_ensemble.hpp"

static_assert(ENS_MAX == GCNN_GROUP_MAX, "one score row per member of a group");

static int launch_ens_mean(const float* const* rows, int n_models, int n, float* mean, hipStream_t st) {
    if (n <= 0) return 0;
    EnsArgs a; memset(&a, 0, sizeof(a));
    for (int m = 0; m < n_models; ++m) a.row[m] = rows[m];
    a.mean = mean; a.n_models = n_models; a.n = n;
    ProfScope prof("k_ens_mean", st);
    hipLaunchKernelGGL(k_ens_mean, dim3(std::min(cdiv(n, 256), 1024)), dim3(256), 0, st, a);
    LAUNCHCHK();
    return 0;
}

extern "C" int gcnn_ensemble_mean(const float* const* member_scores, int32_t n_models, int32_t n, float* mean, void* stream) {
    if (n_models < 1 || n_models > GCNN_GROUP_MAX || n < 0) return GCNN_E_BADARG;
    if (n == 0) return 0;
    if (!member_scores || !mean) return GCNN_E_BADARG;
    for (int m = 0; m < n_models; ++m) if (!member_scores[m]) return GCNN_E_BADARG;
    return launch_ens_mean(member_scores, n_models, n, mean, (hipStream_t)stream);
}

// The layout: gcnn_infer_batch's for the call's states, whose forward-workspace block holds the members' score rows over the whole
// union and then M forward workspaces; the launch tables of the group behind the selection workspace.  `solo`: the single-state
// calls, whose limits hold so that what they decline is what gcnn_infer declines -- 32,768 variables, and 4,096 cuts in the two
// ordering modes; the many-state calls (gcnn_ensbatch.hpp) know the second limit alone, for every state of theirs.
static int ens_layout(int n_states, const gcnn_dims* d, const int32_t* n_forced, const int32_t* n_forced_entries, int mode, int n_models,
                      bool solo, gcnn_ensemble_layout* EL) {
    if (!EL || !d || n_models < 1 || n_models > GCNN_GROUP_MAX) return GCNN_E_BADARG;
    IbSums t;
    const int rc = ibatch_sums(n_states, d, n_forced, n_forced_entries, mode, &t, nullptr);
    if (rc) return rc;
    if (solo && d->n_vars > IPLAN_MAX_VARS) return GCNN_E_UNSUPPORTED;
    for (int s = 0; s < n_states; ++s)
        if (mode != GCNN_IBATCH_SCORES && d[s].n_cuts > SEL_MAX_CUTS) return GCNN_E_UNSUPPORTED;
    memset(EL, 0, sizeof(*EL));
    gcnn_ibatch_layout* L = &EL->u;
    const gcnn_dims total = t.dims();
    const size_t M = n_models;
    const size_t row = al16(4 * (size_t)total.n_cuts), rows = (M * row + 255) & ~(size_t)255;
    const size_t ws = (sizeof(float) * gcnn_workspace_floats(&total) + 255) & ~(size_t)255;
    EL->n_models = n_models;
    EL->table_bytes = group_table_bytes(n_models);
    size_t extra[1];
    union_layout(t, n_states, mode, 1, 4 * (size_t)IB_COLS * IB_TS, false, rows + M * ws, {EL->table_bytes}, extra, L);
    EL->table_off = extra[0];
    EL->member_off = L->dev_off[12] - L->dev_off[11];
    EL->member_stride = row;
    for (size_t m = 0; m < M; ++m) EL->ws_off[m] = L->dev_off[12] + rows + m * ws;
    L->out_bytes = EL->member_off + M * row;   // the download reaches over the members' rows
    return 0;
}

extern "C" int gcnn_infer_ensemble_layout_for(const gcnn_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode,
                                              int32_t n_models, gcnn_ensemble_layout* layout) {
    return layout_out(layout, [&](gcnn_ensemble_layout* l) { return ens_layout(1, dims, &n_forced, &n_forced_entries, mode, n_models, true, l); });
}

// What a call holds between its host half and its device half: the index pass's arguments, the members and their recorded launches.
struct EnsCall {
    IbArgs ia;
    int n_models;
    gcnn_group_member mem[GCNN_GROUP_MAX];
    const float* rows[GCNN_GROUP_MAX];
    GroupPlan plan;
};

// What a many-state call runs in RANK mode in place of the mean and the ranking (gcnn_ensbatch.hpp); the single-state calls pass none.
typedef int (*EnsRankTail)(const EnsCall& c, const gcnn_ibatch_layout& L, const IbAt& at, hipStream_t st);

// ens_prepare: the host half -- the members over the union that lies at `at`, group_check's rules, and the recording of every
// member's forward pass into `host_staging`.  Nothing is enqueued.
static int ens_prepare(const gcnn_ensemble_layout& EL, const float* const* params, char* A, const IbAt& at, void* host_staging,
                       hipStream_t st, EnsCall* c) {
    const gcnn_ibatch_layout& L = EL.u;
    memset(c->mem, 0, sizeof(c->mem));
    c->n_models = EL.n_models;
    c->ia = union_args(at, L, A, 1);
    const IbArgs& ia = c->ia;
    gcnn_graph cg, kg; memset(&cg, 0, sizeof(cg)); memset(&kg, 0, sizeof(kg));
    cg.l_ptr = ia.l_ptr[0]; cg.l_oth = ia.var[0]; cg.l_coef = (const float*)at.arr[2];
    cg.v_ptr = (int*)(A + L.dev_off[6]); cg.v_oth = (int*)(A + L.dev_off[7]); cg.v_coef = (float*)(A + L.dev_off[8]);
    kg.l_ptr = ia.l_ptr[1]; kg.l_oth = ia.var[1]; kg.l_coef = (const float*)at.arr[6];
    kg.v_ptr = cg.v_ptr;   // never read: conv v->k gathers by cut only and nothing is differentiated
    for (int m = 0; m < EL.n_models; ++m) {
        gcnn_group_member& g = c->mem[m];
        if (!params[m]) return GCNN_E_BADARG;
        g.dims = L.total; g.params = params[m];
        g.cons_feats = (const float*)at.arr[0]; g.var_feats = (const float*)at.arr[3]; g.cut_feats = (const float*)at.arr[4];
        g.cons_graph = cg; g.cut_graph = kg;
        g.workspace = (float*)(A + EL.ws_off[m]); g.workspace_floats = gcnn_workspace_floats(&L.total);
        g.scores = (float*)(at.out + EL.member_off + (size_t)m * EL.member_stride);
        c->rows[m] = g.scores;
    }
    int rc = group_check(EL.n_models, c->mem, host_staging, A + EL.table_off, EL.table_bytes, false);
    if (rc) return rc;
    return group_plan(EL.n_models, c->mem, host_staging, [&](int i) { return group_member_step(c->mem[i], false, st); }, &c->plan);
}

// ens_run: the device half, on a union that lies at `at`: the index pass, the by-variable stage, the launch tables and the forward
// passes as a group, the mean, ranking or selection over the mean per state, the flags into the output block.
static int ens_run(int mode, const gcnn_ensemble_layout& EL, char* A, const IbAt& at, void* host_staging, EnsCall& c, double p_max,
                   double p_max_ub, EnsRankTail rank_tail, hipStream_t st) {
    int rc;
    const gcnn_ibatch_layout& L = EL.u;
    const gcnn_dims& T = L.total;
    const int E1 = T.n_cons_edges, V = T.n_vars;
    const IbArgs& ia = c.ia;
    const gcnn_graph& cg = c.mem[0].cons_graph;
    {
        ProfScope prof("k_ens_unpack", st);
        hipLaunchKernelGGL(k_ib_unpack, union_grid(L), dim3(256), 0, st, ia);
        LAUNCHCHK();
    }
    if (E1 > 0) {          // gcnn_graph_build's by-variable stage on the state's list
        ProfScope prof("k_ens_by_variable", st);
        if ((rc = by_key_stage(A + L.dev_off[10], sort_temp_bytes(E1), ia.var[0], ia.iota, (int*)(A + L.dev_off[4]), (int*)(A + L.dev_off[5]),
                               V, E1, ia.left, cg.l_coef, (int*)cg.v_ptr, (int*)cg.v_oth, (float*)cg.v_coef, st))) return rc;
    } else {
        HIPCHK(hipMemsetAsync((void*)cg.v_ptr, 0, ((size_t)V + 1) * sizeof(int), st));
    }
    // the second upload: the launch tables; then every stage of the M forward passes as one launch per distinct kernel
    if ((rc = group_issue(EL.n_models, c.mem, host_staging, A + EL.table_off, c.plan,
                          [&](int i) { return group_member_step(c.mem[i], false, st); }, st))) return rc;
    float* mean = (float*)(at.out + L.out_off[0]);
    if (mode == GCNN_IBATCH_RANK && rank_tail) {
        if (T.n_cuts > 0 && (rc = rank_tail(c, L, at, st))) return rc;
    } else {
        if ((rc = launch_ens_mean(c.rows, EL.n_models, T.n_cuts, mean, st))) return rc;
        if (mode == GCNN_IBATCH_RANK && T.n_cuts > 0) {
            ProfScope prof("k_ens_rank", st);
            hipLaunchKernelGGL(k_ib_rank, dim3(L.n_states), dim3(256), 0, st, (const float*)mean, at.table, (int*)(at.out + L.out_off[1]));
            LAUNCHCHK();
        }
    }
    return union_tail(mode, L, A, at, ia, ia.l_ptr[1], p_max, p_max_ub, st);
}

static int ens_call_check(int n_models, const float* const* params, const void* host_in, const void* host_out, const void* arena,
                          size_t arena_bytes, size_t need_bytes, const void* host_staging, int mode, double p_max, double p_max_ub) {
    if (!params || !host_staging) return GCNN_E_BADARG;
    for (int m = 0; m < n_models; ++m) if (!params[m]) return GCNN_E_BADARG;
    return call_check(params[0], host_in, host_out, arena, arena_bytes, need_bytes, mode == GCNN_IBATCH_SELECT, p_max, p_max_ub);
}

// ens_call: the whole call on host states -- gcnn_infer_ensemble with one state and the single-state limits, gcnn_infer_ensemble_batch
// (gcnn_ensbatch.hpp) with 1..64 and its own tail in RANK mode.
static int ens_call(int n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode, int n_models,
                    bool solo, const float* const* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes,
                    void* host_staging, double p_max, double p_max_ub, EnsRankTail rank_tail, void* stream) {
    gcnn_ensemble_layout EL;
    int rc = ens_layout(n_states, dims, n_forced, n_forced_entries, mode, n_models, solo, &EL);
    if (rc) return rc;
    const gcnn_ibatch_layout& L = EL.u;
    if ((rc = ens_call_check(n_models, params, host_in, host_out, arena, arena_bytes, L.arena_bytes, host_staging, mode, p_max, p_max_ub)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    const IbAt at = union_at(A, L);
    static thread_local EnsCall call;
    if ((rc = ens_prepare(EL, params, A, at, host_staging, st, &call))) return rc;       // host work only
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));          // upload 1: the states (+ forced rows), ONCE
    if ((rc = ens_run(mode, EL, A, at, host_staging, call, p_max, p_max_ub, rank_tail, st))) return rc;
    HIPCHK(hipMemcpyAsync(host_out, at.out, L.out_bytes, hipMemcpyDeviceToHost, st));   // ONE download: mean | order | n_kept | flags | members
    return 0;
}

extern "C" int gcnn_infer_ensemble(const gcnn_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode, int32_t n_models,
                                   const float* const* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes,
                                   void* host_staging, double p_max, double p_max_ub, void* stream) {
    return ens_call(1, dims, &n_forced, &n_forced_entries, mode, n_models, true, params, host_in, host_out, arena, arena_bytes,
                    host_staging, p_max, p_max_ub, nullptr, stream);
}

// ---- the LP form: gcnn_lp_batch's builder launches for the call's snapshots in front of the same work ----------------------------------
static int lpens_layout(int n, const gcnn_lp_dims* d, const int32_t* n_forced, const int32_t* n_forced_entries, int mode, int n_models,
                        bool solo, gcnn_lp_ensemble_layout* L, gcnn_lp_layout* each) {
    if (!L) return GCNN_E_BADARG;
    return lpset_layout(n, d, LPSET_IB_TABLE, [&](const gcnn_dims* sd, gcnn_ibatch_layout* S) {
        const int rc = ens_layout(n, sd, n_forced, n_forced_entries, mode, n_models, solo, &L->ens);
        if (!rc) *S = L->ens.u;
        return rc; }, &L->lp, each);
}

extern "C" int gcnn_lp_ensemble_layout_for(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode,
                                           int32_t n_models, gcnn_lp_ensemble_layout* layout) {
    return layout_out(layout, [&](gcnn_lp_ensemble_layout* l) { return lpens_layout(1, dims, &n_forced, &n_forced_entries, mode, n_models, true, l, nullptr); });
}

// lpens_call: the whole call on LP snapshots -- gcnn_lp_ensemble with one, gcnn_lp_ensemble_batch (gcnn_ensbatch.hpp) with 1..64.
static int lpens_call(int n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode, int n_models,
                      bool solo, const float* const* params, void* host_in, void* host_out, void* arena, size_t arena_bytes,
                      void* host_staging, double p_max, double p_max_ub, EnsRankTail rank_tail, void* stream) {
    gcnn_lp_ensemble_layout L;
    gcnn_lp_layout each[GCNN_IBATCH_MAX];
    int rc =lpens_layout(n, dims, n_forced, n_forced_entries, mode, n_models, solo, &L, each);
    if (rc) return rc;
    if ((rc = ens_call_check(n_models, params, host_in, host_out, arena, arena_bytes, L.lp.arena_bytes, host_staging, mode, p_max, p_max_ub)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    // the tables in front of the packed snapshots: the union's table, then the snapshots' descriptors (host work)
    gcnn_dims sd[GCNN_IBATCH_MAX];
    for (int s = 0; s < n; ++s) sd[s] = lp_state_dims(&dims[s]);
    memset(host_in, 0, L.lp.table_bytes);
    if ((rc = ibatch_sums(n, sd, n_forced, n_forced_entries, mode, nullptr, (int32_t*)host_in))) return rc;
    lpset_fill(n, dims, L.lp, each, LPSET_IB_TABLE, host_in);
    const IbAt at = lpset_at(A, L.lp);
    static thread_local EnsCall call;
    if ((rc = ens_prepare(L.ens, params, A, at, host_staging, st, &call))) return rc;   // host work only
    HIPCHK(hipMemcpyAsync(A + L.lp.up_off, host_in, L.lp.in_bytes, hipMemcpyHostToDevice, st));   // upload 1: tables | snapshots | forced rows
    int n_stats, n_emit;
    const LpSetArgs g = lpset_launch(n, dims, L.lp, LPSET_IB_TABLE, A, &n_stats, &n_emit);
    {
        ProfScope prof("k_ens_lp_stats", st);
        hipLaunchKernelGGL(k_lpset_stats, dim3(n_stats), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_ens_lp_emit", st);
        hipLaunchKernelGGL(k_lpset_emit, dim3(n_emit), dim3(LP_NT), 0, st, g);
        LAUNCHCHK();
    }
    // A flagged snapshot leaves parts of its state unwritten: the index pass confines whatever ids lie there to the state's own
    // ranges, as in gcnn_lp_batch, and the caller discards the results once an LP flag is set.
    if ((rc = ens_run(mode, L.ens, A, at, host_staging, call, p_max, p_max_ub, rank_tail, st))) return rc;
    // ONE download: mean | order | n_kept | flags | members | LP flags | cut_index
    HIPCHK(hipMemcpyAsync(host_out, at.out, L.lp.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}

extern "C" int gcnn_lp_ensemble(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode, int32_t n_models,
                                const float* const* params, void* host_in, void* host_out, void* arena, size_t arena_bytes,
                                void* host_staging, double p_max, double p_max_ub, void* stream) {
    return lpens_call(1, dims, &n_forced, &n_forced_entries, mode, n_models, true, params, host_in, host_out, arena, arena_bytes,
                      host_staging, p_max, p_max_ub, nullptr, stream);
}
