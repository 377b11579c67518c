// gcnn_lpremove.hpp -- host side of the removal of rows from a resident LP (k_lpremove.hpp): gcnn_lp_rows_remove, the removal alone,
// and gcnn_lp_round_remove, the removal (and an append behind it) inside the call of the round that follows.  Included at the end
// of gcnn_capi.hip behind gcnn_lpappend.hpp (it shares lpa_layout / lpa_check / lpa_enqueue and gcnn_lpres.hpp's lpr_check /
// lpr_run), kept apart so that its launch names form their own inventory (tests/test_lpremove_build.py).
#include "k_lpremove.hpp"

// scratch carving: part_a | part_b | vcnt + vpart (one cleared block) | row_map | row_new
struct LpdScratch { size_t part_a, part_b, vcnt, vpart, clear_bytes, row_map, row_new, bytes; };
static LpdScratch lpd_scratch(const gcnn_lp_dims* d) {
    LpdScratch s; Carver c{0};
    const size_t nrc = lp_chunks(d->n_rows), nvc = lp_chunks(d->n_cols);
    s.part_a = c.take(16 * (nrc + 1), 16);
    s.part_b = c.take(16 * (nrc + 1), 16);
    s.vcnt = c.take(4 * (size_t)d->n_cols, 16);
    s.vpart = c.take(4 * (nvc + 1), 16);
    s.clear_bytes = c.off - s.vcnt;
    s.row_map = c.take(4 * (size_t)d->n_state_rows, 16);
    s.row_new = c.take(4 * (size_t)d->n_rows, 16);
    s.bytes = c.off;
    return s;
}

// the resident dims and the removal's counts -> the dims after the removal; false where either is malformed, where a count exceeds
// what is resident, or where the whole edit (b: the block appended behind it, or null) leaves no row at all
static bool lpd_dims_after(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, gcnn_lp_dims* mid) {
    if (!lp_dims_ok(d) || !m) return false;
    if (m->n_rows < 1 || m->row_nnz < 0 || m->n_state_rows < 0 || m->n_state_edges < 0 || m->n_lhs_rows < 0 || m->n_lhs_edges < 0) return false;
    if (m->n_rows > d->n_rows || m->row_nnz > d->row_nnz || m->n_state_rows > d->n_state_rows || m->n_state_edges > d->n_state_edges)
        return false;
    if (m->n_lhs_rows > m->n_rows || m->n_state_rows - m->n_lhs_rows > m->n_rows || m->n_lhs_rows > m->n_state_rows) return false;
    if (m->n_lhs_edges > m->row_nnz || m->n_lhs_edges > m->n_state_edges || (int64_t)m->n_state_edges - m->n_lhs_edges > m->row_nnz) return false;
    if (m->res_lhs_rows < 0 || m->res_lhs_rows > d->n_state_rows || m->res_lhs_edges < 0 || m->res_lhs_edges > d->n_state_edges) return false;
    if (m->n_lhs_rows > m->res_lhs_rows || m->n_lhs_edges > m->res_lhs_edges) return false;
    if (m->n_state_rows - m->n_lhs_rows > d->n_state_rows - m->res_lhs_rows ||
        m->n_state_edges - m->n_lhs_edges > d->n_state_edges - m->res_lhs_edges)
        return false;
    *mid = *d;
    mid->n_rows -= m->n_rows; mid->row_nnz -= m->row_nnz; mid->n_state_rows -= m->n_state_rows; mid->n_state_edges -= m->n_state_edges;
    if (!lp_dims_ok(mid)) return false;
    if (b && (b->res_lhs_rows != m->res_lhs_rows - m->n_lhs_rows || b->res_lhs_edges != m->res_lhs_edges - m->n_lhs_edges)) return false;
    return (int64_t)mid->n_rows + (b ? b->n_rows : 0) >= 1;
}

static int lpd_layout(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, int32_t present, int32_t n_forced,
                      int32_t n_forced_entries, gcnn_lp_remove_layout* L) {
    gcnn_lp_dims mid;
    if (!L || !lpd_dims_after(d, m, b, &mid)) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    L->list_bytes = (4 * (size_t)m->n_rows + 255) & ~(size_t)255;
    size_t inner_in, inner_arena;
    int rc;
    if (b) {                                                    // the fused append's call behind the list, its flags in front of ours
        gcnn_lp_append_layout AL;
        rc = lpa_layout(&mid, b, present, n_forced, n_forced_entries, &AL, 16);
        if (rc == GCNN_E_BADARG) return rc;
        L->block_bytes = AL.block_bytes;
        for (int i = 0; i < 5; ++i) L->block_off[i] = L->list_bytes + AL.block_off[i];
        L->round = AL.round;
        inner_in = AL.in_bytes; inner_arena = AL.arena_bytes;
        L->out_bytes = AL.out_bytes; L->append_flags_off = AL.flags_off;
        L->round_off = L->list_bytes + AL.round_off; L->append_scratch_off = L->list_bytes + AL.scratch_off;
    } else {
        rc = lpr_round_layout(&mid, present, n_forced, n_forced_entries, &L->round, 16);
        if (rc == GCNN_E_BADARG) return rc;
        inner_in = L->round.in_bytes; inner_arena = L->round.arena_bytes;
        L->out_bytes = L->round.out_bytes;
        L->round_off = L->list_bytes;
    }
    L->in_bytes = L->list_bytes + inner_in;
    L->flags_off = L->out_bytes - 16;                           // the removal's four flag words close the download
    L->scratch_bytes = lpd_scratch(d).bytes;
    L->scratch_off = L->list_bytes + ((inner_arena + 255) & ~(size_t)255);
    L->arena_bytes = L->scratch_off + L->scratch_bytes;
    return rc;
}
extern "C" int gcnn_lp_remove_layout_for(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, int32_t present,
                                         int32_t n_forced, int32_t n_forced_entries, gcnn_lp_remove_layout* L) {
    return lpd_layout(d, m, b, present, n_forced, n_forced_entries, L);
}

// byte spans of a set of derived arrays / of the raw rows for given sizes, and whether any span of one list meets one of another
struct LpdSpan { uintptr_t lo, hi; };
static void lpd_span(std::vector<LpdSpan>& out, const void* p, size_t bytes) {
    if (p && bytes) out.push_back(LpdSpan{(uintptr_t)p, (uintptr_t)p + bytes});
}
static std::vector<LpdSpan> lpd_set_spans(const gcnn_lp_rows_set* s, const gcnn_lp_dims* d) {
    std::vector<LpdSpan> out;
    const size_t R = d->n_rows, C = d->n_state_rows, E = d->n_state_edges, V = d->n_cols;
    lpd_span(out, s->cons_feats, 16 * C); lpd_span(out, s->edge_row, 4 * E); lpd_span(out, s->edge_col, 4 * E);
    lpd_span(out, s->edge_coef, 4 * E); lpd_span(out, s->l_ptr, 4 * (C + 1)); lpd_span(out, s->v_ptr, 4 * (V + 1));
    lpd_span(out, s->v_oth, 4 * E); lpd_span(out, s->v_coef, 4 * E); lpd_span(out, s->row_place, 8 * R); lpd_span(out, s->row_scale, 8 * R);
    return out;
}
static std::vector<LpdSpan> lpd_raw_spans(const void* const raw[5], const gcnn_lp_dims* d) {
    std::vector<LpdSpan> out;
    const size_t R = d->n_rows, N = d->row_nnz;
    lpd_span(out, raw[0], 4 * (R + 1)); lpd_span(out, raw[1], 4 * N); lpd_span(out, raw[2], 8 * N); lpd_span(out, raw[3], 8 * R);
    lpd_span(out, raw[4], 8 * R);
    return out;
}
static bool lpd_meet(const std::vector<LpdSpan>& a, const std::vector<LpdSpan>& b) {
    for (const LpdSpan& x : a)
        for (const LpdSpan& y : b)
            if (x.lo < y.hi && y.lo < x.hi) return true;
    return false;
}
static bool lpd_raw_ok(const void* const raw[5], const gcnn_lp_dims* d) {
    return raw[0] && (d->n_rows == 0 || (raw[3] && raw[4])) && (d->row_nnz == 0 || (raw[1] && raw[2]));
}

// Everything a removal decides before anything is enqueued.  dst_dims: the sizes the destinations must hold (the dims after the
// removal, or after the append behind it for the raw rows, which the append then extends in place).
static int lpd_check(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, gcnn_lp_dims* mid,
                     const void* const raw_src[5], const void* const raw_dst[5], const gcnn_lp_dims* raw_dst_dims,
                     const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst) {
    if (!lpd_dims_after(d, m, b, mid)) return GCNN_E_BADARG;
    if (!lpd_raw_ok(raw_src, d) || !lpd_raw_ok(raw_dst, raw_dst_dims ? raw_dst_dims : mid)) return GCNN_E_BADARG;
    if (!lpa_set_ok(src, d->n_rows, d->n_state_rows, d->n_state_edges)) return GCNN_E_BADARG;
    if (!lpa_set_ok(dst, mid->n_rows, mid->n_state_rows, mid->n_state_edges)) return GCNN_E_BADARG;
    if (d->n_state_edges > 0 && (d->n_cols == 0 || d->n_state_rows == 0)) return GCNN_E_BADARG;
    if (lpd_meet(lpd_set_spans(src, d), lpd_set_spans(dst, mid))) return GCNN_E_BADARG;
    if (lpd_meet(lpd_raw_spans(raw_src, d), lpd_raw_spans(raw_dst, raw_dst_dims ? raw_dst_dims : mid))) return GCNN_E_BADARG;
    if (d->n_state_rows > (1 << 24) || d->n_cols > (1 << 24)) return GCNN_E_UNSUPPORTED;
    return 0;
}

// Everything the removal enqueues: one fill, three launches.  counts: null, or where the caller keeps the cleared removed counters
// (vcnt + vpart, LpdScratch::clear_bytes) and has enqueued their fill itself (gcnn_lpedits.hpp: one fill for all sessions).
static int lpd_enqueue(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_dims* mid, const int32_t* list,
                       const void* const raw_src[5], void* const raw_dst[5], const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst,
                       char* scratch, int32_t* flags_dev, hipStream_t st, char* counts = nullptr) {
    const LpdScratch s = lpd_scratch(d);
    LpdArgs x; memset(&x, 0, sizeof(x));
    x.src = lpa_set(src); x.dst = lpa_set(dst);
    x.list = list; x.n_list = m->n_rows;
    x.raw_ptr = (const int*)raw_src[0]; x.raw_col = (const int*)raw_src[1]; x.raw_val = (const double*)raw_src[2];
    x.raw_lhs = (const double*)raw_src[3]; x.raw_rhs = (const double*)raw_src[4];
    x.out_ptr = (int*)raw_dst[0]; x.out_col = (int*)raw_dst[1]; x.out_val = (double*)raw_dst[2];
    x.out_lhs = (double*)raw_dst[3]; x.out_rhs = (double*)raw_dst[4];
    x.R0 = d->n_rows; x.N0 = d->row_nnz; x.C0 = d->n_state_rows; x.E0 = d->n_state_edges;
    x.R1 = mid->n_rows; x.N1 = mid->row_nnz; x.C1 = mid->n_state_rows; x.E1 = mid->n_state_edges;
    x.L1 = m->res_lhs_rows - m->n_lhs_rows; x.EL1 = m->res_lhs_edges - m->n_lhs_edges;
    x.V = d->n_cols; x.nvc = lp_chunks(x.V); x.nrc = lp_chunks(x.R0);
    x.part_a = (int*)(scratch + s.part_a); x.part_b = (int*)(scratch + s.part_b);
    char* cnt = counts ? counts : scratch + s.vcnt;
    x.vcnt = (int*)cnt; x.vpart = (int*)(cnt + (s.vpart - s.vcnt)); x.row_map = (int*)(scratch + s.row_map);
    x.row_new = (int*)(scratch + s.row_new);
    x.nb_var = (x.V + LP_NT / LP_SUB - 1) / (LP_NT / LP_SUB); x.nb_edges = lp_chunks(x.E0); x.nb_raw = lp_chunks(x.N0);
    x.flags_out = flags_dev;
    if (!counts) HIPCHK(hipMemsetAsync(cnt, 0, s.clear_bytes, st));      // the removed counters (no launch of the library's own)
    {
        ProfScope prof("k_lpd_mark", st);
        GCNN_LAUNCH(k_lpd_mark, dim3(x.nrc), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_lpd_rows", st);
        GCNN_LAUNCH(k_lpd_rows, dim3(x.nrc + 1 + lp_chunks(x.V + 1)), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    if (x.nb_var + x.nb_edges + x.nb_raw > 0) {
        ProfScope prof("k_lpd_vars", st);
        GCNN_LAUNCH(k_lpd_vars, dim3(x.nb_var + x.nb_edges + x.nb_raw), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    return 0;
}

extern "C" int gcnn_lp_rows_remove(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const int32_t* list, const int32_t* row_ptr,
                                   const int32_t* row_col, const double* row_val, const double* row_lhs, const double* row_rhs,
                                   int32_t* out_ptr, int32_t* out_col, double* out_val, double* out_lhs, double* out_rhs,
                                   const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst, void* scratch, size_t scratch_bytes,
                                   int32_t* flags, void* stream) {
    gcnn_lp_dims mid;
    const void* const raw_src[5] = {row_ptr, row_col, row_val, row_lhs, row_rhs};
    void* const raw_dst[5] = {out_ptr, out_col, out_val, out_lhs, out_rhs};
    const int rc = lpd_check(d, m, nullptr, &mid, raw_src, raw_dst, nullptr, src, dst);
    if (rc) return rc;
    if (!list || !scratch || ((uintptr_t)scratch & 15) || !flags) return GCNN_E_BADARG;
    if (scratch_bytes < lpd_scratch(d).bytes) return GCNN_E_WORKSPACE;
    return lpd_enqueue(d, m, &mid, list, raw_src, raw_dst, src, dst, (char*)scratch, flags, (hipStream_t)stream);
}

extern "C" int gcnn_lp_round_remove(const gcnn_lp_dims* d, const gcnn_lp_remove_dims* m, const gcnn_lp_append_dims* b, int32_t present,
                                    int32_t n_forced, int32_t n_forced_entries, const int32_t* row_ptr, const int32_t* row_col,
                                    const double* row_val, const double* row_lhs, const double* row_rhs, int32_t* out_ptr,
                                    int32_t* out_col, double* out_val, double* out_lhs, double* out_rhs, const gcnn_lp_rows_set* src,
                                    const gcnn_lp_rows_set* transit, const gcnn_lp_rows_set* dst, const gcnn_lp_resident* resident,
                                    const float* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes,
                                    int32_t want_order, double p_max, double p_max_ub, void* stream) {
    gcnn_lp_remove_layout L;
    int rc = lpd_layout(d, m, b, present, n_forced, n_forced_entries, &L);
    if (rc) return rc;
    gcnn_lp_dims mid, after;
    const void* const raw_src[5] = {row_ptr, row_col, row_val, row_lhs, row_rhs};
    void* const raw_dst[5] = {out_ptr, out_col, out_val, out_lhs, out_rhs};
    const gcnn_lp_rows_set* first = b ? transit : dst;          // what the removal writes
    if (b && (!lpd_dims_after(d, m, b, &mid) || !lpa_dims_after(&mid, b, &after))) return GCNN_E_BADARG;
    if ((rc = lpd_check(d, m, b, &mid, raw_src, raw_dst, b ? &after : nullptr, src, first))) return rc;
    if (b) {
        if ((rc = lpa_check(&mid, b, &after, out_ptr, out_col, out_val, out_lhs, out_rhs, resident ? resident->col_obj : nullptr, transit, dst)))
            return rc;
        const std::vector<LpdSpan> last = lpd_set_spans(dst, &after);
        if (lpd_meet(lpd_set_spans(src, d), last) || lpd_meet(lpd_set_spans(transit, &mid), last)) return GCNN_E_BADARG;
    } else {
        after = mid;
    }
    if (!arena || ((uintptr_t)arena & 255) || arena_bytes < L.arena_bytes) return GCNN_E_BADARG;
    char* A = (char*)arena;
    gcnn_lp_round_layout RL;
    if ((rc = lpr_check(&after, present, n_forced, n_forced_entries, resident, params, host_in, host_out, A + L.round_off, L.round.arena_bytes,
                        n_forced >= 0 ? 1 : want_order, p_max, p_max_ub, b ? 32 : 16, &RL)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));          // ONE upload: the list | the block | the round | forced rows
    char* out = A + L.round_off + RL.dev_off[6];
    if ((rc = lpd_enqueue(d, m, &mid, (const int32_t*)A, raw_src, raw_dst, src, first, A + L.scratch_off, (int32_t*)(out + L.flags_off), st)))
        return rc;
    if (b) {
        int32_t* const raw[2] = {out_ptr, out_col};
        double* const rawd[3] = {out_val, out_lhs, out_rhs};
        if ((rc = lpa_enqueue(&mid, b, (const int*)(A + L.block_off[0]), (const int*)(A + L.block_off[1]), (const double*)(A + L.block_off[2]),
                              (const double*)(A + L.block_off[3]), (const double*)(A + L.block_off[4]), b->row_nnz, 0, raw, rawd,
                              resident->col_obj, transit, dst, A + L.append_scratch_off, (int32_t*)(out + L.append_flags_off), st)))
            return rc;
    }
    return lpr_run(&after, RL, present, n_forced, resident, params, nullptr, host_out, A + L.round_off, n_forced >= 0 ? 1 : want_order, p_max,
                   p_max_ub, stream);                                                   // ONE download, the flags of both edits in it
}
