// gcnn_select.hpp -- host side of the cut selection (k_select.hpp): gcnn_select_cuts and the single-call gcnn_infer_select.
// Included at the end of gcnn_capi.hip (it shares that file's statics: ProfScope, the single-state call's layout and forward), but
// kept apart so that its launch names form their own inventory (tests/test_select_build.py).
#include "k_select.hpp"

static size_t select_ws_bytes(int total_cuts, int total_forced, int max_cuts) {
    const size_t words = (size_t)(std::max(max_cuts, 0) + 63) / 64;
    return std::max<size_t>(((size_t)std::max(total_cuts, 0) + (size_t)std::max(total_forced, 0)) * words * 16, 16);
}

static int launch_select(SelArgs& a, hipStream_t st) {
    const int n_rows = a.total_cuts + a.total_forced;
    if (n_rows > 0 && a.total_cuts > 0) {
        ProfScope prof("k_sel_pairs", st);
        hipLaunchKernelGGL(k_sel_pairs, dim3(std::min(n_rows, 65535)), dim3(SEL_NT), 0, st, a);
        LAUNCHCHK();
    }
    ProfScope prof("k_sel_filter", st);
    hipLaunchKernelGGL(k_sel_filter, dim3(a.n_samples), dim3(SEL_NT), 0, st, a);
    LAUNCHCHK();
    return 0;
}

static bool finite_threshold(double x) { return x == x && x - x == 0.0; }

extern "C" size_t gcnn_select_workspace_bytes(int32_t total_cuts, int32_t total_forced, int32_t max_cuts) {
    return select_ws_bytes(total_cuts, total_forced, max_cuts);
}

extern "C" int gcnn_select_cuts(const float* quality, const int32_t* cut_ptr, const int32_t* cut_col, const float* cut_val,
                                const int32_t* cut_offsets, int32_t n_samples, int32_t total_cuts, int32_t max_cuts, int32_t n_vars,
                                const int32_t* forced_ptr, const int32_t* forced_col, const float* forced_val,
                                const int32_t* forced_offsets, int32_t total_forced, double p_max, double p_max_ub, int32_t* order,
                                int32_t* n_kept, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_samples < 1 || total_cuts < 0 || total_forced < 0 || max_cuts < 0 || n_vars < 0 || !n_kept) return GCNN_E_BADARG;
    if (!finite_threshold(p_max) || !finite_threshold(p_max_ub)) return GCNN_E_BADARG;
    if (max_cuts > SEL_MAX_CUTS) return GCNN_E_UNSUPPORTED;
    if (n_samples > 1 && (!cut_offsets || (total_forced > 0 && !forced_offsets))) return GCNN_E_BADARG;
    if (total_cuts > 0 && (!quality || !cut_ptr || !order)) return GCNN_E_BADARG;
    if (total_forced > 0 && !forced_ptr) return GCNN_E_BADARG;
    if (!workspace || workspace_bytes < select_ws_bytes(total_cuts, total_forced, max_cuts)) return GCNN_E_WORKSPACE;
    SelArgs a;
    a.q = quality; a.c_ptr = cut_ptr; a.c_col = cut_col; a.c_val = cut_val; a.c_off = cut_offsets;
    a.f_ptr = forced_ptr; a.f_col = forced_col; a.f_val = forced_val; a.f_off = total_forced > 0 ? forced_offsets : nullptr;
    a.n_samples = n_samples; a.total_cuts = total_cuts; a.total_forced = total_forced; a.max_cuts = max_cuts; a.n_vars = n_vars;
    a.words = (max_cuts + 63) / 64; a.p_max = p_max; a.p_max_ub = p_max_ub;
    a.bits = (unsigned long long*)workspace; a.order = order; a.n_kept = n_kept;
    return launch_select(a, (hipStream_t)stream);
}

// ---- single call: gcnn_infer's upload / plan / forward, then the selection on the cut rows already in the arena ---------------
static int select_layout(const gcnn_dims* d, int32_t n_forced, int32_t n_forced_entries, gcnn_select_layout* L) {
    if (!L || n_forced < 0 || n_forced_entries < 0) return GCNN_E_BADARG;
    const size_t F = n_forced, EF = n_forced_entries;
    const size_t extra_in = al16(4 * (F + 1)) + al16(4 * EF) + al16(4 * EF);
    int rc = infer_layout(d, extra_in, 16, &L->infer);
    if (rc) return rc;
    if (d->n_cuts > SEL_MAX_CUTS) return GCNN_E_UNSUPPORTED;
    const size_t in_forced = L->infer.in_bytes - extra_in;   // the forced block closes the upload
    L->forced_off[0] = in_forced;
    L->forced_off[1] = L->forced_off[0] + al16(4 * (F + 1));
    L->forced_off[2] = L->forced_off[1] + al16(4 * EF);
    L->n_kept_off = L->infer.out_off[2] + 16;
    L->ws_off = L->infer.arena_bytes;
    L->infer.arena_bytes += (select_ws_bytes(d->n_cuts, n_forced, d->n_cuts) + 255) & ~(size_t)255;
    return 0;
}

extern "C" int gcnn_infer_select_layout_for(const gcnn_dims* d, int32_t n_forced, int32_t n_forced_entries,
                                            gcnn_select_layout* L) {
    return select_layout(d, n_forced, n_forced_entries, L);
}

// The selection on scores and cut rows that lie in the arena of a single-state call (out: its output block); the forced rows
// wherever the caller's upload put them.
static int select_in_arena(const gcnn_dims* d, int32_t n_forced, const gcnn_graph& kg, const void* f_ptr, const void* f_col,
                           const void* f_val, char* out, size_t order_off, size_t n_kept_off, void* ws, double p_max,
                           double p_max_ub, hipStream_t st) {
    SelArgs a;
    a.q = (const float*)out; a.c_ptr = kg.l_ptr; a.c_col = kg.l_oth; a.c_val = kg.l_coef; a.c_off = nullptr;
    a.f_ptr = (const int*)f_ptr; a.f_col = (const int*)f_col; a.f_val = (const float*)f_val; a.f_off = nullptr;
    a.n_samples = 1; a.total_cuts = d->n_cuts; a.total_forced = n_forced; a.max_cuts = d->n_cuts; a.n_vars = d->n_vars;
    a.words = (d->n_cuts + 63) / 64; a.p_max = p_max; a.p_max_ub = p_max_ub;
    a.bits = (unsigned long long*)ws; a.order = (int*)(out + order_off); a.n_kept = (int*)(out + n_kept_off);
    return launch_select(a, st);
}

extern "C" int gcnn_infer_select(const gcnn_dims* d, int32_t n_forced, int32_t n_forced_entries, const float* params,
                                 const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max,
                                 double p_max_ub, void* stream) {
    gcnn_select_layout SL;
    int rc = select_layout(d, n_forced, n_forced_entries, &SL);
    if (rc) return rc;
    const gcnn_infer_layout& L = SL.infer;
    if (!params || !host_in || !host_out || !arena || arena_bytes < L.arena_bytes || ((uintptr_t)arena & 255)) return GCNN_E_BADARG;
    if (!finite_threshold(p_max) || !finite_threshold(p_max_ub)) return GCNN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    gcnn_graph kg;
    const int* flags = nullptr;
    rc = infer_forward(d, params, host_in, A, L, st, &kg, &flags);   // the upload carries the forced rows too
    if (rc) return rc;
    char* out = A + L.dev_off[6];
    rc = select_in_arena(d, n_forced, kg, A + SL.forced_off[0], A + SL.forced_off[1], A + SL.forced_off[2], out, L.out_off[1],
                         SL.n_kept_off, A + SL.ws_off, p_max, p_max_ub, st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out + L.out_off[2], flags, 16, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(host_out, out, L.out_bytes, hipMemcpyDeviceToHost, st));  // ONE download: scores | order | flags | n_kept
    return 0;
}
