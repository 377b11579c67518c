// gcnn_select.hpp -- host side of the cut selection (k_select.hpp): gcnn_select_cuts, and the single-state calls gcnn_infer and
// gcnn_infer_select as one body (state_call).  It also holds what every pinned-upload call shares: the argument check (call_check),
// the one builder of SelArgs (sel_args) and the end of a single-state call (infer_tail) -- gcnn_lpstate.hpp and gcnn_ibatch.hpp,
// included after it, use them.  Included at the end of gcnn_capi.hip (it shares that file's statics: ProfScope, the single-state
// call's layout, its run-from-the-arena half and its ranking), but kept apart so that its launch names form their own inventory
// (tests/test_select_build.py).
#include "k_select.hpp"

static size_t select_ws_bytes(int total_cuts, int total_forced, int max_cuts) {
    const size_t words = ((size_t)std::max(max_cuts, 0) + 63) / 64;
    return std::max<size_t>(((size_t)std::max(total_cuts, 0) + (size_t)std::max(total_forced, 0)) * words * 16, 16);
}

static int launch_select(SelArgs& a, hipStream_t st) {
    const int n_rows = a.total_cuts + a.total_forced;
    if (n_rows > 0 && a.total_cuts > 0) {
        ProfScope prof("k_sel_pairs", st);
        GCNN_LAUNCH(k_sel_pairs, dim3(std::min(n_rows, 65535)), dim3(SEL_NT), 0, st, a);
        LAUNCHCHK();
    }
    ProfScope prof("k_sel_filter", st);
    GCNN_LAUNCH(k_sel_filter, dim3(a.n_samples), dim3(SEL_NT), 0, st, a);
    LAUNCHCHK();
    return 0;
}

static bool finite_thresholds(double p_max, double p_max_ub) {
    return p_max == p_max && p_max - p_max == 0.0 && p_max_ub == p_max_ub && p_max_ub - p_max_ub == 0.0;
}
// Rows in CSR form as the selection reads them (cut rows or forced rows): offsets, columns, values, and `off`, the first row of each
// sample ([n_samples+1]) or null for one sample.
struct SelRows { const int* ptr; const int* col; const float* val; const int* off; };
// every field of SelArgs, in one place.  ws: select_ws_bytes(total_cuts, total_forced, max_cuts) bytes
static SelArgs sel_args(const float* q, SelRows cuts, SelRows forced, int n_samples, int total_cuts, int total_forced, int max_cuts,
                        int n_vars, double p_max, double p_max_ub, void* ws, int* order, int* n_kept) {
    SelArgs a;
    a.q = q; a.c_ptr = cuts.ptr; a.c_col = cuts.col; a.c_val = cuts.val; a.c_off = cuts.off;
    a.f_ptr = forced.ptr; a.f_col = forced.col; a.f_val = forced.val; a.f_off = forced.off;
    a.n_samples = n_samples; a.total_cuts = total_cuts; a.total_forced = total_forced; a.max_cuts = max_cuts; a.n_vars = n_vars;
    a.words = (max_cuts + 63) / 64; a.p_max = p_max; a.p_max_ub = p_max_ub;
    a.bits = (unsigned long long*)ws; a.order = order; a.n_kept = n_kept;
    return a;
}

extern "C" size_t gcnn_select_workspace_bytes(int32_t total_cuts, int32_t total_forced, int32_t max_cuts) {
    return select_ws_bytes(total_cuts, total_forced, max_cuts);
}

extern "C" int gcnn_select_cuts(const float* quality, const int32_t* cut_ptr, const int32_t* cut_col, const float* cut_val,
                                const int32_t* cut_offsets, int32_t n_samples, int32_t total_cuts, int32_t max_cuts, int32_t n_vars,
                                const int32_t* forced_ptr, const int32_t* forced_col, const float* forced_val,
                                const int32_t* forced_offsets, int32_t total_forced, double p_max, double p_max_ub, int32_t* order,
                                int32_t* n_kept, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_samples < 1 || total_cuts < 0 || total_forced < 0 || max_cuts < 0 || n_vars < 0 || !n_kept) return GCNN_E_BADARG;
    if (!finite_thresholds(p_max, p_max_ub)) return GCNN_E_BADARG;
    if (max_cuts > SEL_MAX_CUTS) return GCNN_E_UNSUPPORTED;
    if (n_samples > 1 && (!cut_offsets || (total_forced > 0 && !forced_offsets))) return GCNN_E_BADARG;
    if (total_cuts > 0 && (!quality || !cut_ptr || !order)) return GCNN_E_BADARG;
    if (total_forced > 0 && !forced_ptr) return GCNN_E_BADARG;
    if (!workspace || workspace_bytes < select_ws_bytes(total_cuts, total_forced, max_cuts)) return GCNN_E_WORKSPACE;
    SelArgs a = sel_args(quality, SelRows{cut_ptr, cut_col, cut_val, cut_offsets},
                         SelRows{forced_ptr, forced_col, forced_val, total_forced > 0 ? forced_offsets : nullptr}, n_samples,
                         total_cuts, total_forced, max_cuts, n_vars, p_max, p_max_ub, workspace, order, n_kept);
    return launch_select(a, (hipStream_t)stream);
}

// ---- the single-state calls: upload, plan + forward (infer_run), then ranking or selection on what lies in the arena -----------
static int select_layout(const gcnn_dims* d, int32_t n_forced, int32_t n_forced_entries, gcnn_select_layout* L) {
    if (!L || n_forced < 0 || n_forced_entries < 0) return GCNN_E_BADARG;
    Carver extra{0};
    size_t rel[3];
    forced_block(extra, n_forced, n_forced_entries, rel);
    int rc = infer_layout(d, extra.off, 16, &L->infer);
    if (rc) return rc;
    if (d->n_cuts > SEL_MAX_CUTS) return GCNN_E_UNSUPPORTED;
    for (int i = 0; i < 3; ++i) L->forced_off[i] = L->infer.in_bytes - extra.off + rel[i];   // the forced block closes the upload
    L->n_kept_off = L->infer.out_off[2] + 16;
    L->ws_off = L->infer.arena_bytes;
    L->infer.arena_bytes += (select_ws_bytes(d->n_cuts, n_forced, d->n_cuts) + 255) & ~(size_t)255;
    return 0;
}

extern "C" int gcnn_infer_select_layout_for(const gcnn_dims* d, int32_t n_forced, int32_t n_forced_entries,
                                            gcnn_select_layout* L) {
    return layout_out(L, [&](gcnn_select_layout* l) { return select_layout(d, n_forced, n_forced_entries, l); });
}

// What every call that uploads from pinned memory into a caller-owned arena refuses: a missing pointer, an arena shorter than the
// layout's or not 256-byte aligned, and -- for a call that selects -- a threshold that is not finite.
static int call_check(const float* params, const void* host_in, const void* host_out, const void* arena, size_t arena_bytes,
                      size_t need_bytes, bool select, double p_max, double p_max_ub) {
    if (!params || !host_in || !host_out || !arena || arena_bytes < need_bytes || ((uintptr_t)arena & 255)) return GCNN_E_BADARG;
    if (select && !finite_thresholds(p_max, p_max_ub)) return GCNN_E_BADARG;
    return 0;
}

// The end of a single-state call, once infer_run has left scores, cut rows (kg) and plan flags in the arena: with n_forced >= 0 the
// selection (forced: the uploaded rows on the device, wherever the caller's upload put them; ws: its workspace; n_kept lands at
// n_kept_off of the output block), else the ranking on request; then the flags go behind the outputs and ONE download brings
// L.out_bytes home: scores | order | flags | whatever the caller's layout keeps behind them.
// infer_order: its launches alone (the selection, or the ranking on request); infer_tail: those, the flags and the download.
static int infer_order(const gcnn_dims* d, const gcnn_infer_layout& L, char* A, const gcnn_graph& kg, int32_t n_forced, SelRows forced,
                       void* ws, size_t n_kept_off, int32_t want_order, double p_max, double p_max_ub, hipStream_t st) {
    char* out = A + L.dev_off[6];
    if (n_forced >= 0) {
        SelArgs a = sel_args((const float*)out, SelRows{kg.l_ptr, kg.l_oth, kg.l_coef, nullptr}, forced, 1, d->n_cuts, n_forced,
                             d->n_cuts, d->n_vars, p_max, p_max_ub, ws, (int*)(out + L.out_off[1]), (int*)(out + n_kept_off));
        return launch_select(a, st);
    }
    return want_order ? infer_rank(d, A, L, st) : 0;
}
static int infer_tail(const gcnn_dims* d, const gcnn_infer_layout& L, char* A, const gcnn_graph& kg, const int* flags,
                      int32_t n_forced, SelRows forced, void* ws, size_t n_kept_off, int32_t want_order, double p_max, double p_max_ub,
                      void* host_out, hipStream_t st) {
    char* out = A + L.dev_off[6];
    const int rc = infer_order(d, L, A, kg, n_forced, forced, ws, n_kept_off, want_order, p_max, p_max_ub, st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out + L.out_off[2], flags, 16, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(host_out, out, L.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
// the three forced arrays of one state at base + off[0..2] (forced_block)
static SelRows forced_rows(const char* base, const size_t* off) {
    return SelRows{(const int*)(base + off[0]), (const int*)(base + off[1]), (const float*)(base + off[2]), nullptr};
}

// gcnn_infer (n_forced = -1: scores, ranked when want_order) and gcnn_infer_select (the upload carries the forced rows too)
static int state_call(const gcnn_dims* d, int32_t n_forced, int32_t n_forced_entries, const float* params, const void* host_in,
                      void* host_out, void* arena, size_t arena_bytes, int32_t want_order, double p_max, double p_max_ub, void* stream) {
    const bool select = n_forced >= 0;
    gcnn_select_layout SL; memset(&SL, 0, sizeof(SL));
    int rc = select ? select_layout(d, n_forced, n_forced_entries, &SL) : infer_layout(d, 0, 0, &SL.infer);
    if (rc) return rc;
    const gcnn_infer_layout& L = SL.infer;
    if ((rc = call_check(params, host_in, host_out, arena, arena_bytes, L.arena_bytes, select, p_max, p_max_ub))) return rc;
    if (!select && want_order && d->n_cuts > 4096) return GCNN_E_UNSUPPORTED;
    if (edges_without_nodes(*d)) return GCNN_E_BADARG;   // (the Python session raises its index error for these before it gets here)
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    gcnn_graph kg;
    const int* flags = nullptr;
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));      // ONE upload: zero block + the seven arrays (+ forced)
    if ((rc = infer_run(d, params, A, L, st, &kg, &flags))) return rc;
    return infer_tail(d, L, A, kg, flags, n_forced, forced_rows(A, SL.forced_off), A + SL.ws_off, SL.n_kept_off, want_order, p_max,
                      p_max_ub, host_out, st);
}

extern "C" int gcnn_infer(const gcnn_dims* d, const float* params, const void* host_in, void* host_out, void* arena,
                          size_t arena_bytes, int32_t want_order, void* stream) {
    return state_call(d, -1, 0, params, host_in, host_out, arena, arena_bytes, want_order, 0.0, 0.0, stream);
}

extern "C" int gcnn_infer_select(const gcnn_dims* d, int32_t n_forced, int32_t n_forced_entries, const float* params,
                                 const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max,
                                 double p_max_ub, void* stream) {
    if (n_forced < 0) return GCNN_E_BADARG;
    return state_call(d, n_forced, n_forced_entries, params, host_in, host_out, arena, arena_bytes, 1, p_max, p_max_ub, stream);
}
