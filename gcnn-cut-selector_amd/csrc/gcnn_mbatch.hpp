// gcnn_mbatch.hpp -- host side of gcnn_infer_models (include/gcnn_hip.h): gcnn_infer_batch's contract for 1..64 host states that
// belong to 1..GCNN_GROUP_MAX models -- what a scoring server holds when the evaluators' task farm runs with `seed` as its innermost
// loop (model_evaluator.py:211-219).  One upload of the states, one index pass over all of them and one by-variable stage for the
// whole union (k_mbatch.hpp), the models' forward passes as ONE group (gcnn_group.hpp: one launch per distinct kernel and stage,
// each member's solo bits), one ranking or selection over all states, one download.  Included from gcnn_capi.hip's list of host
// files, after gcnn_group.hpp and gcnn_ibatch.hpp: the layout, the index pass's arguments and the end of a run are that file's
// (union_layout, union_at, union_args, union_tail).  Kept apart so that its launch names form their own inventory
// (tests/test_mbatch_build.py).
//
// The upload and the download are gcnn_infer_batch's (gcnn_ibatch_layout), with two differences: the table carries the model words
// behind its seven columns (MB_TABLE_WORDS), and the zero block holds one closing by-left entry per MODEL (C + n_models and
// K + n_models entries) and, in selection mode, the cut rows' offsets over the whole union.  Arrays stay at the union's positions.
// The selection is ONE launch pair over all states: pairs are only formed inside a state, a state's cut rows and forced rows carry
// the same model-relative column ids, and k_sel_pairs reads the union-wide offsets that k_mb_unpack writes beside the per-model ones.
// A model without a state is refused (GCNN_E_BADARG): the caller numbers the models it sends.
#include "k_mbatch.hpp"

static_assert(MB_TABLE_WORDS == GCNN_MBATCH_TABLE_WORDS, "table shape");

struct MbModels { int first[GCNN_GROUP_MAX + 1]; gcnn_dims dims[GCNN_GROUP_MAX]; };

// model_of_state: non-decreasing, from 0, without gaps, up to n_models - 1
static int mbatch_models(int n_states, const gcnn_dims* dims, int n_models, const int32_t* model_of_state, MbModels* M) {
    if (n_models < 1 || n_models > GCNN_GROUP_MAX || !model_of_state) return GCNN_E_BADARG;
    memset(M, 0, sizeof(*M));
    int prev = -1;
    for (int s = 0; s < n_states; ++s) {
        const int m = model_of_state[s];
        if (m < 0 || m >= n_models || m < prev || m > prev + 1) return GCNN_E_BADARG;
        if (m != prev) M->first[m] = s;
        prev = m;
        gcnn_dims& t = M->dims[m];
        const gcnn_dims& d = dims[s];
        t.n_cons += d.n_cons; t.n_vars += d.n_vars; t.n_cuts += d.n_cuts; t.n_cons_edges += d.n_cons_edges; t.n_cut_edges += d.n_cut_edges;
    }
    if (prev != n_models - 1) return GCNN_E_BADARG;
    M->first[n_models] = n_states;
    return 0;
}

static int mbatch_layout(int n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode,
                         int n_models, const int32_t* model_of_state, gcnn_mbatch_layout* ML) {
    if (!ML) return GCNN_E_BADARG;
    IbSums t;
    int rc = ibatch_sums(n_states, dims, n_forced, n_forced_entries, mode, &t, nullptr);
    if (rc) return rc;
    MbModels mm;
    if ((rc = mbatch_models(n_states, dims, n_models, model_of_state, &mm))) return rc;
    memset(ML, 0, sizeof(*ML));
    gcnn_ibatch_layout* L = &ML->u;
    ML->n_models = n_models;
    for (int m = 0; m <= n_models; ++m) ML->first_state[m] = mm.first[m];
    size_t ws = 0;
    for (int m = 0; m < n_models; ++m) {
        ML->model[m] = mm.dims[m];
        ML->ws_off[m] = ws;
        ws += (sizeof(float) * gcnn_workspace_floats(&mm.dims[m]) + 255) & ~(size_t)255;
    }
    ML->table_bytes = group_table_bytes(n_models);
    // gcnn_infer_batch's layout with the model words behind the table, one closing entry per model ([6]: one v_ptr per model) and
    // the models' forward workspaces at [12]; behind it the sort keys [14] | the union's v_ptr [15] | the group's launch tables
    size_t extra[3];
    union_layout(t, n_states, mode, n_models, al16(4 * (size_t)MB_TABLE_WORDS), mode == GCNN_IBATCH_SELECT, ws,
                 {4 * (size_t)t.e1, 4 * ((size_t)t.v + 1), ML->table_bytes}, extra, L);
    L->dev_off[14] = extra[0]; L->dev_off[15] = extra[1]; ML->table_off = extra[2];
    for (int m = 0; m < n_models; ++m) ML->ws_off[m] += L->dev_off[12];
    return 0;
}

extern "C" int gcnn_infer_models_layout_for(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced,
                                            const int32_t* n_forced_entries, int32_t mode, int32_t n_models,
                                            const int32_t* model_of_state, gcnn_mbatch_layout* layout) {
    return layout_out(layout, [&](gcnn_mbatch_layout* l) { return mbatch_layout(n_states, dims, n_forced, n_forced_entries, mode, n_models, model_of_state, l); });
}

extern "C" int gcnn_infer_models_fill_table(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced,
                                            const int32_t* n_forced_entries, int32_t n_models, const int32_t* model_of_state,
                                            int32_t* table) {
    if (!table) return GCNN_E_BADARG;
    // (checked in full before the first word is written: a refused call leaves the table as it was)
    int rc = ibatch_sums(n_states, dims, n_forced, n_forced_entries, GCNN_IBATCH_SELECT, nullptr, nullptr);
    if (rc) return rc;
    MbModels mm;
    if ((rc = mbatch_models(n_states, dims, n_models, model_of_state, &mm))) return rc;
    if ((rc = ibatch_sums(n_states, dims, n_forced, n_forced_entries, GCNN_IBATCH_SELECT, nullptr, table))) return rc;
    int32_t* mod = table + IB_COLS * IB_TS;
    memset(mod, 0, sizeof(int32_t) * (MB_HEAD + IB_MAX_STATES));
    mod[0] = n_models;
    for (int m = 0; m <= n_models; ++m) mod[1 + m] = mm.first[m];
    for (int s = 0; s < n_states; ++s) mod[MB_HEAD + s] = model_of_state[s];
    return 0;
}

// What a call holds between its host half and its device half: the index pass's arguments, the members (each model's sub-union,
// every array a slice of the union's at the model's first state) and the recorded launch tables of their forward passes.
struct MbCall {
    MbArgs ma;
    gcnn_group_member mem[GCNN_GROUP_MAX];
    int *v_ptr, *v_oth, *g_ptr;
    float* v_coef;
    GroupPlan plan;
};

// mbatch_prepare: the host half -- where everything lies for a union at `at` (IbAt, gcnn_ibatch.hpp), group_check's rules, and the
// recording of every member's forward pass into `host_staging`.  Nothing is enqueued: what it refuses is refused before any
// device work (GCNN_E_UNSUPPORTED for a forward pass the group recorder cannot take).
static int mbatch_prepare(int n_states, int mode, const gcnn_mbatch_layout& ML, const float* const* params, char* A, const IbAt& at,
                          void* host_staging, hipStream_t st, MbCall* c) {
    const gcnn_ibatch_layout& L = ML.u;
    const gcnn_dims& T = L.total;
    const size_t M = ML.n_models;
    memset(c->mem, 0, sizeof(c->mem));
    c->ma.ib = union_args(at, L, A, M);
    IbArgs& ia = c->ma.ib;
    c->ma.key = (int*)(A + L.dev_off[14]);
    c->ma.sel_ptr = mode == GCNN_IBATCH_SELECT ? ia.l_ptr[1] + al16(4 * ((size_t)T.n_cuts + M)) / 4 : nullptr;
    c->v_ptr = (int*)(A + L.dev_off[6]); c->v_oth = (int*)(A + L.dev_off[7]); c->v_coef = (float*)(A + L.dev_off[8]);
    c->g_ptr = (int*)(A + L.dev_off[15]);
    float* scores = (float*)(at.out + L.out_off[0]);
    size_t cc = 0, v = 0, k = 0, e1 = 0, e2 = 0;
    for (int m = 0; m < ML.n_models; ++m) {
        gcnn_group_member& g = c->mem[m];
        const gcnn_dims& d = ML.model[m];
        if (!params[m]) return GCNN_E_BADARG;
        g.dims = d; g.params = params[m];
        g.cons_feats = (const float*)at.arr[0] + 4 * cc; g.var_feats = (const float*)at.arr[3] + 14 * v; g.cut_feats = (const float*)at.arr[4] + 6 * k;
        g.cons_graph.l_ptr = ia.l_ptr[0] + cc + m; g.cons_graph.l_oth = ia.var[0] + e1; g.cons_graph.l_coef = (const float*)at.arr[2] + e1;
        g.cons_graph.v_ptr = c->v_ptr + v + m; g.cons_graph.v_oth = c->v_oth + e1; g.cons_graph.v_coef = c->v_coef + e1;
        g.cut_graph.l_ptr = ia.l_ptr[1] + k + m; g.cut_graph.l_oth = ia.var[1] + e2; g.cut_graph.l_coef = (const float*)at.arr[6] + e2;
        g.cut_graph.v_ptr = g.cons_graph.v_ptr;   // never read: conv v->k gathers by cut only and nothing is differentiated
        g.workspace = (float*)(A + ML.ws_off[m]); g.workspace_floats = gcnn_workspace_floats(&d);
        g.scores = scores + k;
        cc += d.n_cons; v += d.n_vars; k += d.n_cuts; e1 += d.n_cons_edges; e2 += d.n_cut_edges;
    }
    int rc = group_check(ML.n_models, c->mem, host_staging, A + ML.table_off, ML.table_bytes, false);
    if (rc) return rc;
    return group_plan(ML.n_models, c->mem, host_staging, [&](int i) { return group_member_step(c->mem[i], false, st); }, &c->plan);
}

// mbatch_run: the device half, on a union that lies at `at` (ibatch_run's counterpart): the index pass over all states, the
// by-variable stage of the whole union and its split per model, the upload of the launch tables and the forward passes as a
// group, ranking or selection over all states, the flags into the output block.
static int mbatch_run(int n_states, int mode, const gcnn_mbatch_layout& ML, char* A, const IbAt& at, void* host_staging, MbCall& c,
                      double p_max, double p_max_ub, hipStream_t st) {
    int rc;
    const gcnn_ibatch_layout& L = ML.u;
    const gcnn_dims& T = L.total;
    const size_t M = ML.n_models;
    const int E1 = T.n_cons_edges, V = T.n_vars;
    IbArgs& ia = c.ma.ib;
    {
        ProfScope prof("k_mb_unpack", st);
        hipLaunchKernelGGL(k_mb_unpack, union_grid(L), dim3(256), 0, st, c.ma);
        LAUNCHCHK();
    }
    if (E1 > 0) {   // gcnn_graph_build's by-variable stage on the union's list, keyed by the union's variable ids
        {
            ProfScope prof("k_mb_by_variable", st);
            if ((rc = by_key_stage(A + L.dev_off[10], sort_temp_bytes(E1), c.ma.key, ia.iota, (int*)(A + L.dev_off[4]), (int*)(A + L.dev_off[5]),
                                   V, E1, ia.left, (const float*)at.arr[2], c.g_ptr, c.v_oth, c.v_coef, st))) return rc;
        }
        ProfScope prof("k_mb_vptr", st);
        hipLaunchKernelGGL(k_mb_vptr, dim3(std::min(cdiv(V + ML.n_models, 256), 1024)), dim3(256), 0, st, at.table, (const int*)c.g_ptr, c.v_ptr);
        LAUNCHCHK();
    } else {
        HIPCHK(hipMemsetAsync(c.v_ptr, 0, ((size_t)V + M) * sizeof(int), st));
    }
    // the second upload: the launch tables; then every stage of the forward passes as one launch per distinct kernel
    if ((rc = group_issue(ML.n_models, c.mem, host_staging, A + ML.table_off, c.plan,
                          [&](int i) { return group_member_step(c.mem[i], false, st); }, st))) return rc;
    if (mode == GCNN_IBATCH_RANK && T.n_cuts > 0) {
        ProfScope prof("k_mb_rank", st);
        hipLaunchKernelGGL(k_ib_rank, dim3(n_states), dim3(256), 0, st, (const float*)(at.out + L.out_off[0]), at.table,
                           (int*)(at.out + L.out_off[1]));
        LAUNCHCHK();
    }
    return union_tail(mode, L, A, at, ia, c.ma.sel_ptr, p_max, p_max_ub, st);
}

extern "C" int gcnn_infer_models(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                 int32_t mode, int32_t n_models, const int32_t* model_of_state, const float* const* params,
                                 const void* host_in, void* host_out, void* arena, size_t arena_bytes, void* host_staging,
                                 double p_max, double p_max_ub, void* stream) {
    gcnn_mbatch_layout ML;
    int rc = mbatch_layout(n_states, dims, n_forced, n_forced_entries, mode, n_models, model_of_state, &ML);
    if (rc) return rc;
    const gcnn_ibatch_layout& L = ML.u;
    if (!params || !host_staging) return GCNN_E_BADARG;
    if ((rc = call_check(params[0], host_in, host_out, arena, arena_bytes, L.arena_bytes, mode == GCNN_IBATCH_SELECT, p_max, p_max_ub))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    const IbAt at = union_at(A, L);
    static thread_local MbCall call;
    if ((rc = mbatch_prepare(n_states, mode, ML, params, A, at, host_staging, st, &call))) return rc;   // host work only
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));       // upload 1: the states
    if ((rc = mbatch_run(n_states, mode, ML, A, at, host_staging, call, p_max, p_max_ub, st))) return rc;
    HIPCHK(hipMemcpyAsync(host_out, at.out, L.out_bytes, hipMemcpyDeviceToHost, st));   // ONE download: scores | order | n_kept | flags
    return 0;
}
