// gcnn_lpstate.hpp -- host side of the state built from a raw LP snapshot (k_lpstate.hpp): gcnn_lp_state and the single calls
// gcnn_lp_infer / gcnn_lp_infer_select.  Included at the end of gcnn_capi.hip (it shares that file's statics: ProfScope, the carver,
// the single-state call's layout and its run-from-the-arena half; and gcnn_select.hpp's call_check and infer_tail), kept apart so
// that its launch names form their own inventory (tests/test_lpstate_build.py).
#include "k_lpstate.hpp"

static bool lp_dims_ok(const gcnn_lp_dims* d) {
    if (!d) return false;
    if (d->n_rows < 0 || d->n_cols < 0 || d->n_cuts < 0 || d->row_nnz < 0 || d->cut_nnz < 0) return false;
    if (d->n_state_rows < 0 || d->n_state_edges < 0 || d->n_model_vars < 1) return false;
    if ((int64_t)d->n_state_rows > 2 * (int64_t)d->n_rows || (int64_t)d->n_state_edges > 2 * (int64_t)d->row_nnz) return false;
    if (!(d->infinity > 0.0) || !(d->sum_epsilon > 0.0) || !(d->obj_norm > 0.0) || d->obj_norm - d->obj_norm != 0.0) return false;
    return true;
}
static inline int lp_chunks(int n) { return (int)(((long long)n + LP_NT - 1) / LP_NT); }   // any n >= 0 a layout query may hold
static gcnn_dims lp_state_dims(const gcnn_lp_dims* d) {
    return gcnn_dims{d->n_state_rows, d->n_cols, d->n_cuts, d->n_state_edges, d->cut_nnz};
}

// scratch carving: row_stat | cut_stat | col_part | row_part | cut_part | cut_aux | blk_flags
struct LpScratch { size_t row_stat, cut_stat, col_part, row_part, cut_part, cut_aux, blk_flags, bytes; };
static LpScratch lp_scratch(const gcnn_lp_dims* d) {
    LpScratch s; Carver c{0};
    s.row_stat = c.take(16 * (size_t)d->n_rows, 16);
    s.cut_stat = c.take(32 * (size_t)d->n_cuts, 16);
    s.col_part = c.take(16 * (size_t)(lp_chunks(d->n_cols) + 1), 16);
    s.row_part = c.take(16 * (size_t)(lp_chunks(d->n_rows) + 1), 16);
    s.cut_part = c.take(16 * (size_t)(lp_chunks(d->n_cuts) + 1), 16);
    s.cut_aux = c.take(8 * (size_t)d->n_cuts, 16);
    s.blk_flags = c.take(4 * (size_t)(lp_chunks(d->n_cols) + lp_chunks(d->n_rows) + lp_chunks(d->n_cuts) + 1), 16);
    s.bytes = c.off;
    return s;
}

static int lp_layout(const gcnn_lp_dims* d, int32_t n_forced, int32_t n_forced_entries, gcnn_lp_layout* L) {
    if (!L || !lp_dims_ok(d) || (n_forced >= 0 && n_forced_entries < 0)) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    const size_t R = d->n_rows, V = d->n_cols, K = d->n_cuts, NR = d->row_nnz, NK = d->cut_nnz, P = d->has_incumbent ? V : 0;
    Carver in{0};
    const size_t sizes[GCNN_LP_ARRAYS] = {16, 4 * (R + 1), 4 * NR, 8 * NR, 8 * R, 8 * R, 8 * R, R,          // header, rows
                                          V, 8 * V, 8 * V, 8 * V, V, 8 * V, 8 * V, 8 * P, 8 * P,           // columns
                                          4 * (K + 1), 4 * NK, 8 * NK, 8 * K, 8 * K};                      // cuts
    for (int i = 0; i < GCNN_LP_ARRAYS; ++i) L->snap_off[i] = in.take(sizes[i], 16);
    L->snap_bytes = in.off;
    L->scratch_bytes = lp_scratch(d).bytes;
    // the single call: the snapshot, then the forced rows, in ONE upload
    const bool select = n_forced >= 0;
    forced_block(in, select ? n_forced : 0, select ? n_forced_entries : 0, L->forced_off);
    L->in_bytes = in.off;
    const gcnn_dims sd = lp_state_dims(d);
    if (sd.n_vars > IPLAN_MAX_VARS || (select && sd.n_cuts > SEL_MAX_CUTS)) return 0;      // call_supported stays 0
    int rc = infer_layout(&sd, 0, 32 + al16(4 * K), &L->state);     // behind the flags: n_kept | lp flags | cut_index
    if (rc) return rc;
    L->out_bytes = L->state.out_bytes;
    for (int i = 0; i < 3; ++i) L->out_off[i] = L->state.out_off[i];
    L->out_off[3] = L->out_off[2] + 16; L->out_off[4] = L->out_off[2] + 32; L->out_off[5] = L->out_off[2] + 48;
    Carver dev{(L->state.arena_bytes + 255) & ~(size_t)255};
    L->ws_off = dev.take(select ? select_ws_bytes(sd.n_cuts, n_forced, sd.n_cuts) : 0, 256);
    L->lp_off = dev.take(L->in_bytes, 256);
    L->scratch_off = dev.take(L->scratch_bytes, 256);
    L->arena_bytes = dev.off;
    L->call_supported = 1;
    return 0;
}

extern "C" int gcnn_lp_layout_for(const gcnn_lp_dims* d, int32_t n_forced, int32_t n_forced_entries, gcnn_lp_layout* L) {
    return layout_out(L, [&](gcnn_lp_layout* l) { return lp_layout(d, n_forced, n_forced_entries, l); });
}

// snap: the packed snapshot in device memory (offsets snap_off); the seven state arrays, cut_index and flags as given
static int lp_launch(const gcnn_lp_dims* d, const size_t* snap_off, const char* snap, char* scratch, float* cons_feats, int* cons_ei,
                     float* cons_ef, float* var_feats, float* cut_feats, int* cut_ei, float* cut_ef, int* cut_index, int* flags,
                     int* zero, int zero_words, hipStream_t st) {
    LpArgs a; memset(&a, 0, sizeof(a));
    auto at = [&](int i) { return snap + snap_off[i]; };
    a.row_ptr = (const int*)at(1); a.row_col = (const int*)at(2); a.row_val = (const double*)at(3);
    a.row_lhs = (const double*)at(4); a.row_rhs = (const double*)at(5); a.row_dual = (const double*)at(6);
    a.row_basis = (const signed char*)at(7);
    a.col_type = (const signed char*)at(8); a.col_obj = (const double*)at(9); a.col_lb = (const double*)at(10);
    a.col_ub = (const double*)at(11); a.col_basis = (const signed char*)at(12); a.col_lp = (const double*)at(13);
    a.col_redcost = (const double*)at(14); a.col_primal = (const double*)at(15); a.col_avg = (const double*)at(16);
    a.cut_ptr = (const int*)at(17); a.cut_col = (const int*)at(18); a.cut_val = (const double*)at(19);
    a.cut_lhs = (const double*)at(20); a.cut_rhs = (const double*)at(21);
    a.R = d->n_rows; a.V = d->n_cols; a.K = d->n_cuts; a.nnz_r = d->row_nnz; a.nnz_k = d->cut_nnz;
    a.has_inc = d->has_incumbent != 0; a.n_model_vars = d->n_model_vars; a.C = d->n_state_rows; a.E1 = d->n_state_edges;
    a.infinity = d->infinity; a.eps = d->sum_epsilon; a.obj_norm = d->obj_norm;
    const LpScratch s = lp_scratch(d);
    a.row_stat = (double*)(scratch + s.row_stat); a.cut_stat = (double*)(scratch + s.cut_stat);
    a.col_part = (double*)(scratch + s.col_part); a.row_part = (int*)(scratch + s.row_part);
    a.cut_part = (int*)(scratch + s.cut_part); a.cut_aux = (int*)(scratch + s.cut_aux); a.blk_flags = (int*)(scratch + s.blk_flags);
    a.nrc = lp_chunks(a.R); a.ncc = lp_chunks(a.V); a.nkc = lp_chunks(a.K); a.n_stat_blocks = std::max(1, a.ncc + a.nrc + a.nkc);
    a.cons_feats = cons_feats; a.cons_ei = cons_ei; a.cons_ef = cons_ef; a.var_feats = var_feats; a.cut_feats = cut_feats;
    a.cut_ei = cut_ei; a.cut_ef = cut_ef; a.cut_index = cut_index; a.flags_out = flags;
    a.zero = zero; a.zero_words = zero_words;
    {
        ProfScope prof("k_lp_stats", st);
        hipLaunchKernelGGL(k_lp_stats, dim3(a.n_stat_blocks), dim3(LP_NT), 0, st, a);
        LAUNCHCHK();
    }
    ProfScope prof("k_lp_emit", st);
    hipLaunchKernelGGL(k_lp_emit, dim3(a.nrc + a.nkc + 1), dim3(LP_NT), 0, st, a);
    LAUNCHCHK();
    return 0;
}

extern "C" int gcnn_lp_state(const gcnn_lp_dims* d, const void* snapshot, void* scratch, size_t scratch_bytes, float* cons_feats,
                             int32_t* cons_edge_inds, float* cons_edge_feats, float* var_feats, float* cut_feats,
                             int32_t* cut_edge_inds, float* cut_edge_feats, int32_t* cut_index, int32_t* flags, void* stream) {
    gcnn_lp_layout L;
    int rc = lp_layout(d, -1, 0, &L);
    if (rc) return rc;
    if (!snapshot || !scratch || !flags || ((uintptr_t)snapshot & 15) || ((uintptr_t)scratch & 15)) return GCNN_E_BADARG;
    if (scratch_bytes < L.scratch_bytes) return GCNN_E_WORKSPACE;
    if ((d->n_state_rows > 0 && (!cons_feats || ((uintptr_t)cons_feats & 15))) || (d->n_cols > 0 && !var_feats) ||
        (d->n_cuts > 0 && (!cut_feats || !cut_index)) || (d->n_state_edges > 0 && (!cons_edge_inds || !cons_edge_feats)) ||
        (d->cut_nnz > 0 && (!cut_edge_inds || !cut_edge_feats)))
        return GCNN_E_BADARG;
    return lp_launch(d, L.snap_off, (const char*)snapshot, (char*)scratch, cons_feats, cons_edge_inds, cons_edge_feats, var_feats,
                     cut_feats, cut_edge_inds, cut_edge_feats, cut_index, flags, nullptr, 0, (hipStream_t)stream);
}

// upload -> state into the arena where gcnn_infer's uploaded arrays live -> plan + forward (+ ranking | selection) -> download
static int lp_call(const gcnn_lp_dims* d, int32_t n_forced, int32_t n_forced_entries, const float* params, const void* host_in,
                   void* host_out, void* arena, size_t arena_bytes, int32_t want_order, double p_max, double p_max_ub, void* stream) {
    gcnn_lp_layout LL;
    int rc = lp_layout(d, n_forced, n_forced_entries, &LL);
    if (rc) return rc;
    if (!LL.call_supported || (want_order && d->n_cuts > 4096)) return GCNN_E_UNSUPPORTED;
    if ((rc = call_check(params, host_in, host_out, arena, arena_bytes, LL.arena_bytes, n_forced >= 0, p_max, p_max_ub))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    const gcnn_infer_layout& L = LL.state;
    const gcnn_dims sd = lp_state_dims(d);
    char* snap = A + LL.lp_off;
    char* out = A + L.dev_off[6];
    HIPCHK(hipMemcpyAsync(snap, host_in, LL.in_bytes, hipMemcpyHostToDevice, st));     // ONE upload: snapshot | forced rows
    rc = lp_launch(d, LL.snap_off, snap, A + LL.scratch_off, (float*)(A + L.in_off[1]), (int*)(A + L.in_off[2]),
                   (float*)(A + L.in_off[3]), (float*)(A + L.in_off[4]), (float*)(A + L.in_off[5]), (int*)(A + L.in_off[6]),
                   (float*)(A + L.in_off[7]), (int*)(out + LL.out_off[5]), (int*)(out + LL.out_off[4]), (int*)(A + L.in_off[0]),
                   (int)((L.in_off[1] - L.in_off[0]) / 4), st);
    if (rc) return rc;
    // A flagged snapshot (bad offsets, say) leaves parts of the state arrays unwritten: they keep what the arena held before.  The
    // plan and the forward pass still run on them; that is safe because the plan validates every index it reads and clamps what
    // it uses (k_infer.hpp), and the caller discards all results once a flag is set.
    gcnn_graph kg;
    const int* flags = nullptr;
    if ((rc = infer_run(&sd, params, A, L, st, &kg, &flags))) return rc;
    return infer_tail(&sd, L, A, kg, flags, n_forced, forced_rows(snap, LL.forced_off), A + LL.ws_off, LL.out_off[3], want_order, p_max,
                      p_max_ub, host_out, st);   // ONE download: LL.out_bytes = L.out_bytes
}

extern "C" int gcnn_lp_infer(const gcnn_lp_dims* d, const float* params, const void* host_in, void* host_out, void* arena,
                             size_t arena_bytes, int32_t want_order, void* stream) {
    return lp_call(d, -1, 0, params, host_in, host_out, arena, arena_bytes, want_order, 0.0, 0.0, stream);
}

extern "C" int gcnn_lp_infer_select(const gcnn_lp_dims* d, int32_t n_forced, int32_t n_forced_entries, const float* params,
                                    const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max,
                                    double p_max_ub, void* stream) {
    if (n_forced < 0) return GCNN_E_BADARG;
    return lp_call(d, n_forced, n_forced_entries, params, host_in, host_out, arena, arena_bytes, 1, p_max, p_max_ub, stream);
}
