// gcnn_lpres.hpp -- host side of the resident LP (k_lpres.hpp): gcnn_lp_rows_build, the rebuild behind an open or an append, and
// the per-round calls gcnn_lp_round / gcnn_lp_round_select.  Included at the end of gcnn_capi.hip (it shares that file's statics:
// ProfScope, the carver, forward_impl; gcnn_select.hpp's call_check, infer_tail and forced rows; gcnn_lpstate.hpp's dims check and
// scratch carving), kept apart so that its launch names form their own inventory (tests/test_lpres_build.py).
#include "k_lpres.hpp"

// ---- the rebuild: raw rows -> the constraint half of the state, row_place, row_scale ------------------------------------------------
static gcnn_lp_dims lpr_rows_only(const gcnn_lp_dims* d) { gcnn_lp_dims r = *d; r.n_cuts = 0; r.cut_nnz = 0; return r; }

static int lpr_rows_layout(const gcnn_lp_dims* d, gcnn_lp_rows_layout* L) {
    if (!L || !lp_dims_ok(d)) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    const size_t R = d->n_rows, C = d->n_state_rows, E1 = d->n_state_edges;
    const gcnn_lp_dims r = lpr_rows_only(d);
    Carver c{0};
    const size_t sizes[GCNN_LPR_DERIVED] = {16 * C, 8 * E1, 4 * E1, 8 * R, 8 * R, 16, lp_scratch(&r).bytes};
    for (int i = 0; i < GCNN_LPR_DERIVED; ++i) L->off[i] = c.take(sizes[i], 256);
    L->bytes = c.off;
    return 0;
}
extern "C" int gcnn_lp_rows_layout_for(const gcnn_lp_dims* d, gcnn_lp_rows_layout* L) {
    return layout_out(L, [&](gcnn_lp_rows_layout* l) { return lpr_rows_layout(d, l); });
}

extern "C" int gcnn_lp_rows_build(const gcnn_lp_dims* d, const int32_t* row_ptr, const int32_t* row_col, const double* row_val,
                                  const double* row_lhs, const double* row_rhs, const double* col_obj, void* derived,
                                  size_t derived_bytes, void* stream) {
    gcnn_lp_rows_layout L;
    int rc = lpr_rows_layout(d, &L);
    if (rc) return rc;
    if (!derived || ((uintptr_t)derived & 255) || !row_ptr) return GCNN_E_BADARG;
    if (derived_bytes < L.bytes) return GCNN_E_WORKSPACE;
    if ((d->row_nnz > 0 && (!row_col || !row_val)) || (d->n_rows > 0 && (!row_lhs || !row_rhs)) || (d->n_cols > 0 && !col_obj))
        return GCNN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    char* D = (char*)derived;
    const gcnn_lp_dims r = lpr_rows_only(d);
    const LpScratch s = lp_scratch(&r);
    char* scratch = D + L.off[6];
    LpArgs a; memset(&a, 0, sizeof(a));
    a.row_ptr = row_ptr; a.row_col = row_col; a.row_val = row_val; a.row_lhs = row_lhs; a.row_rhs = row_rhs; a.col_obj = col_obj;
    a.R = d->n_rows; a.V = d->n_cols; a.nnz_r = d->row_nnz; a.n_model_vars = d->n_model_vars; a.C = d->n_state_rows;
    a.E1 = d->n_state_edges; a.infinity = d->infinity; a.eps = d->sum_epsilon; a.obj_norm = d->obj_norm;
    a.row_stat = (double*)(scratch + s.row_stat); a.row_part = (int*)(scratch + s.row_part); a.cut_part = (int*)(scratch + s.cut_part);
    a.blk_flags = (int*)(scratch + s.blk_flags);
    a.nrc = lp_chunks(a.R); a.n_stat_blocks = std::max(1, a.nrc);
    a.cons_feats = (float*)(D + L.off[0]); a.cons_ei = (int*)(D + L.off[1]); a.cons_ef = (float*)(D + L.off[2]);
    a.flags_out = (int*)(D + L.off[5]);
    const LpEmitMore more = {(int*)(D + L.off[3]), (double*)(D + L.off[4]), nullptr};
    {
        ProfScope prof("k_lpr_rows_stats", st);
        hipLaunchKernelGGL(k_lpr_rows_stats, dim3(a.n_stat_blocks), dim3(LP_NT), 0, st, a);
        LAUNCHCHK();
    }
    ProfScope prof("k_lpr_rows_emit", st);
    hipLaunchKernelGGL(k_lpr_rows_emit, dim3(a.nrc + 1), dim3(LP_NT), 0, st, a, more);
    LAUNCHCHK();
    return 0;
}

// ---- a round ----------------------------------------------------------------------------------------------------------------------
// extra_out: a block behind the download's cut_index, for a caller that extends the call (gcnn_lpappend.hpp); it starts at the
// out_bytes of the plain layout.
static int lpr_round_layout(const gcnn_lp_dims* d, int32_t present, int32_t n_forced, int32_t n_forced_entries, gcnn_lp_round_layout* L,
                            size_t extra_out = 0) {
    if (!L || !lp_dims_ok(d) || present < 0 || present > 15 || (n_forced >= 0 && n_forced_entries < 0)) return GCNN_E_BADARG;
    if (!d->has_incumbent && (present & (GCNN_LPR_PRIMAL | GCNN_LPR_PRIMAL_AVG))) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    const size_t R = d->n_rows, V = d->n_cols, K = d->n_cuts, NK = d->cut_nnz;
    auto opt = [&](int bit) { return (present & bit) ? 8 * V : (size_t)0; };
    // header (word 0: the presence mask) | the rows' and columns' solve-dependent arrays | the optional column arrays | the cuts
    const size_t sizes[GCNN_LPR_ARRAYS] = {16, 8 * R, R, V, 8 * V, 8 * V, opt(GCNN_LPR_LB), opt(GCNN_LPR_UB), opt(GCNN_LPR_PRIMAL),
                                           opt(GCNN_LPR_PRIMAL_AVG), 4 * (K + 1), 4 * NK, 8 * NK, 8 * K, 8 * K};
    Carver in{0};
    for (int i = 0; i < GCNN_LPR_ARRAYS; ++i) L->in_off[i] = in.take(sizes[i], 16);
    const bool select = n_forced >= 0;
    forced_block(in, select ? n_forced : 0, select ? n_forced_entries : 0, L->forced_off);
    L->in_bytes = in.off;
    // the download: scores | order | the forward's flag block (always zero here) | n_kept | the 4 LP flags | cut_index
    L->out_off[0] = 0; L->out_off[1] = al16(4 * K); L->out_off[2] = L->out_off[1] + al16(4 * K);
    L->out_off[3] = L->out_off[2] + 16; L->out_off[4] = L->out_off[2] + 32; L->out_off[5] = L->out_off[2] + 48;
    L->out_bytes = L->out_off[5] + al16(4 * K) + extra_out;
    if (d->n_state_rows > (1 << 24) || d->n_cols > (1 << 24) || d->n_cuts > (1 << 24)) return GCNN_E_UNSUPPORTED;   // the edge passes' tables
    if (select && d->n_cuts > SEL_MAX_CUTS) return GCNN_E_UNSUPPORTED;
    const gcnn_dims sd = lp_state_dims(d);
    gcnn_lp_dims cuts_only = *d; cuts_only.n_rows = 0;
    Carver dev{0};
    const size_t blocks[GCNN_LPR_BLOCKS] = {L->in_bytes, 56 * V, 24 * K, 8 * NK, 4 * NK, 4 * (K + 1), L->out_bytes,
                                            sizeof(float) * gcnn_workspace_floats(&sd), 16, lp_scratch(&cuts_only).bytes,
                                            select ? select_ws_bytes(sd.n_cuts, n_forced, sd.n_cuts) : 0};
    for (int i = 0; i < GCNN_LPR_BLOCKS; ++i) L->dev_off[i] = dev.take(blocks[i], 256);
    L->arena_bytes = dev.off;
    return 0;
}
extern "C" int gcnn_lp_round_layout_for(const gcnn_lp_dims* d, int32_t present, int32_t n_forced, int32_t n_forced_entries,
                                        gcnn_lp_round_layout* L) {
    return layout_out(L, [&](gcnn_lp_round_layout* l) { return lpr_round_layout(d, present, n_forced, n_forced_entries, l); });
}

// want_order: 1 ranking, 0 scores only, -1 the state only (no forward pass; the download carries the flags and cut_index)
// lpr_check: everything a round call decides before anything is enqueued, and the layout.  lpr_run: what it enqueues; host_in null:
// the upload already lies at dev_off[0] of the arena (gcnn_lpremove.hpp's round with edits brings it up with the list and the block).
// at (gcnn_lpedits.hpp's calls of several sessions): the upload lies at at->up, the download block is at->out, the forward's flag
// block is cleared where the download finds it, and nothing is copied: the caller brings everything up and down itself.
// fwd (gcnn_lpens.hpp's round of an ensemble): what is enqueued in place of the one forward pass, on the same condition; it leaves
// the scores where the forward pass leaves them, at the head of the download block.
struct LprAt { char* up; char* out; };
struct LprForward { int (*run)(void* self, hipStream_t st); void* self; };
static int lpr_check(const gcnn_lp_dims* d, int32_t present, int32_t n_forced, int32_t n_forced_entries, const gcnn_lp_resident* res,
                     const float* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes, int32_t want_order,
                     double p_max, double p_max_ub, size_t extra_out, gcnn_lp_round_layout* L) {
    int rc = lpr_round_layout(d, present, n_forced, n_forced_entries, L, extra_out);
    if (rc) return rc;
    const bool select = n_forced >= 0;
    if (want_order < -1 || want_order > 1) return GCNN_E_BADARG;
    if (want_order > 0 && d->n_cuts > 4096) return GCNN_E_UNSUPPORTED;
    if ((rc = call_check(params, host_in, host_out, arena, arena_bytes, L->arena_bytes, select, p_max, p_max_ub))) return rc;
    const gcnn_dims sd = lp_state_dims(d);
    if (!res || edges_without_nodes(sd)) return GCNN_E_BADARG;
    const gcnn_graph& cg = res->cons_graph;
    if ((d->n_rows > 0 && (!res->row_place || !res->row_scale)) || (sd.n_cons > 0 && (!res->cons_feats || ((uintptr_t)res->cons_feats & 15))) ||
        (d->n_cols > 0 && (!res->col_type || !res->col_obj || !res->col_lb || !res->col_ub)) ||
        (d->n_cols > 0 && d->has_incumbent && (!res->col_primal || !res->col_primal_avg)) || !cg.l_ptr || !cg.v_ptr ||
        (sd.n_cons_edges > 0 && (!cg.l_oth || !cg.l_coef || !cg.v_oth || !cg.v_coef)))
        return GCNN_E_BADARG;
    return 0;
}

static int lpr_run(const gcnn_lp_dims* d, const gcnn_lp_round_layout& L, int32_t present, int32_t n_forced, const gcnn_lp_resident* res,
                   const float* params, const void* host_in, void* host_out, void* arena, int32_t want_order, double p_max,
                   double p_max_ub, void* stream, const LprAt* at = nullptr, const LprForward* fwd = nullptr) {
    int rc = 0;
    const gcnn_dims sd = lp_state_dims(d);
    const gcnn_graph& cg = res->cons_graph;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    char* up = at ? at->up : A + L.dev_off[0];
    char* out = at ? at->out : A + L.dev_off[6];
    if (host_in && !at) HIPCHK(hipMemcpyAsync(up, host_in, L.in_bytes, hipMemcpyHostToDevice, st));     // ONE upload: the round | forced rows
    double* keep[4] = {res->col_lb, res->col_ub, res->col_primal, res->col_primal_avg};
    LprArgs x; memset(&x, 0, sizeof(x));
    const double* src[4];
    for (int q = 0; q < 4; ++q) {
        const bool here = (present >> q & 1) != 0;
        x.up[q] = here ? (const double*)(up + L.in_off[6 + q]) : nullptr; x.keep[q] = keep[q];
        src[q] = here ? x.up[q] : keep[q];
    }
    gcnn_lp_dims cuts_only = *d; cuts_only.n_rows = 0;
    const LpScratch s = lp_scratch(&cuts_only);
    char* scratch = A + L.dev_off[9];
    LpArgs a; memset(&a, 0, sizeof(a));
    a.col_type = (const signed char*)res->col_type; a.col_obj = res->col_obj; a.col_lb = src[0]; a.col_ub = src[1];
    a.col_primal = src[2]; a.col_avg = src[3];
    a.col_basis = (const signed char*)(up + L.in_off[3]); a.col_lp = (const double*)(up + L.in_off[4]);
    a.col_redcost = (const double*)(up + L.in_off[5]);
    a.cut_ptr = (const int*)(up + L.in_off[10]); a.cut_col = (const int*)(up + L.in_off[11]); a.cut_val = (const double*)(up + L.in_off[12]);
    a.cut_lhs = (const double*)(up + L.in_off[13]); a.cut_rhs = (const double*)(up + L.in_off[14]);
    a.R = 0; a.V = d->n_cols; a.K = d->n_cuts; a.nnz_k = d->cut_nnz; a.has_inc = d->has_incumbent != 0; a.n_model_vars = d->n_model_vars;
    a.C = 0; a.E1 = 0;                       // no rows in these launches: the flag block's size check sees none
    a.infinity = d->infinity; a.eps = d->sum_epsilon; a.obj_norm = d->obj_norm;
    a.cut_stat = (double*)(scratch + s.cut_stat); a.col_part = (double*)(scratch + s.col_part); a.row_part = (int*)(scratch + s.row_part);
    a.cut_part = (int*)(scratch + s.cut_part); a.cut_aux = (int*)(scratch + s.cut_aux); a.blk_flags = (int*)(scratch + s.blk_flags);
    a.nrc = 0; a.ncc = lp_chunks(a.V); a.nkc = lp_chunks(a.K); a.n_stat_blocks = a.ncc + a.nkc;
    a.var_feats = (float*)(A + L.dev_off[1]); a.cut_feats = (float*)(A + L.dev_off[2]); a.cut_ei = (int*)(A + L.dev_off[3]);
    a.cut_ef = (float*)(A + L.dev_off[4]); a.cut_index = (int*)(out + L.out_off[5]); a.flags_out = (int*)(out + L.out_off[4]);
    int* cut_l_ptr = (int*)(A + L.dev_off[5]);
    int* fwd_flags = at ? (int*)(out + L.out_off[2]) : (int*)(A + L.dev_off[8]);
    x.row_dual = (const double*)(up + L.in_off[1]); x.row_basis = (const signed char*)(up + L.in_off[2]);
    x.row_place = res->row_place; x.row_scale = res->row_scale; x.cons_feats = res->cons_feats;
    x.R = d->n_rows; x.C = sd.n_cons; x.nrc = lp_chunks(x.R); x.first_row_block = a.n_stat_blocks;
    x.clear[0] = cut_l_ptr; x.clear_words[0] = a.K + 1; x.clear[1] = a.cut_ei + a.nnz_k; x.clear_words[1] = a.nnz_k;
    x.clear[2] = fwd_flags; x.clear_words[2] = 4;
    const LpEmitMore more = {nullptr, nullptr, cut_l_ptr};
    {
        ProfScope prof("k_lpr_stats", st);
        GCNN_LAUNCH(k_lpr_stats, dim3(std::max(1, a.n_stat_blocks + x.nrc)), dim3(LP_NT), 0, st, a, x);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_lpr_emit", st);
        GCNN_LAUNCH(k_lpr_emit, dim3(a.nkc + 1), dim3(LP_NT), 0, st, a, more);
        LAUNCHCHK();
    }
    // the forward pass as the general path runs it (no graph plan): the resident constraint graph, the round's cut graph
    gcnn_graph kg; memset(&kg, 0, sizeof(kg));
    kg.l_ptr = cut_l_ptr; kg.l_oth = a.cut_ei + a.nnz_k; kg.l_coef = a.cut_ef; kg.v_ptr = cg.v_ptr;    // (v_*: never read, as in infer_run)
    if (want_order >= 0 && sd.n_cuts > 0 &&           // (a round without cuts has nothing to score: it only refreshes the resident columns)
        (rc = fwd ? fwd->run(fwd->self, st)
                  : forward_impl(&sd, params, res->cons_feats, a.var_feats, a.cut_feats, &cg, &kg, (float*)(A + L.dev_off[7]),
                                 gcnn_workspace_floats(&sd), (float*)out, 0, nullptr, 0.f, st, nullptr)))
        return rc;
    gcnn_infer_layout IL; memset(&IL, 0, sizeof(IL));
    IL.dev_off[6] = (size_t)(out - A); IL.out_bytes = L.out_bytes;
    for (int i = 0; i < 3; ++i) IL.out_off[i] = L.out_off[i];
    if (at)
        return infer_order(&sd, IL, A, kg, want_order >= 0 ? n_forced : -1, forced_rows(up, L.forced_off), A + L.dev_off[10], L.out_off[3],
                           want_order > 0, p_max, p_max_ub, st);
    return infer_tail(&sd, IL, A, kg, fwd_flags, want_order >= 0 ? n_forced : -1, forced_rows(up, L.forced_off), A + L.dev_off[10],
                      L.out_off[3], want_order > 0, p_max, p_max_ub, host_out, st);     // ONE download
}

static int lpr_call(const gcnn_lp_dims* d, int32_t present, int32_t n_forced, int32_t n_forced_entries, const gcnn_lp_resident* res,
                    const float* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes, int32_t want_order,
                    double p_max, double p_max_ub, void* stream) {
    gcnn_lp_round_layout L;
    const int rc = lpr_check(d, present, n_forced, n_forced_entries, res, params, host_in, host_out, arena, arena_bytes, want_order,
                             p_max, p_max_ub, 0, &L);
    return rc ? rc : lpr_run(d, L, present, n_forced, res, params, host_in, host_out, arena, want_order, p_max, p_max_ub, stream);
}

extern "C" int gcnn_lp_round(const gcnn_lp_dims* d, int32_t present, const gcnn_lp_resident* res, const float* params,
                             const void* host_in, void* host_out, void* arena, size_t arena_bytes, int32_t want_order, void* stream) {
    return lpr_call(d, present, -1, 0, res, params, host_in, host_out, arena, arena_bytes, want_order, 0.0, 0.0, stream);
}

extern "C" int gcnn_lp_round_select(const gcnn_lp_dims* d, int32_t present, int32_t n_forced, int32_t n_forced_entries,
                                    const gcnn_lp_resident* res, const float* params, const void* host_in, void* host_out, void* arena,
                                    size_t arena_bytes, double p_max, double p_max_ub, void* stream) {
    if (n_forced < 0) return GCNN_E_BADARG;
    return lpr_call(d, present, n_forced, n_forced_entries, res, params, host_in, host_out, arena, arena_bytes, 1, p_max, p_max_ub, stream);
}
