// gcnn_lpappend.hpp -- host side of the incremental append to a resident LP (k_lpappend.hpp): its layout, check and launches
// (lpa_layout, lpa_check, lpa_enqueue) and gcnn_lp_rows_append, the append alone.  The append inside the call of the round that
// follows it (gcnn_lp_round_append) is one case of the round with edits, gcnn_lpremove.hpp.  Included at the end of gcnn_capi.hip
// behind gcnn_lpres.hpp (it shares that file's layout and everything they share), kept apart so that its launch names form their
// own inventory (tests/test_lpappend_build.py).
#include "k_lpappend.hpp"

// scratch carving: row_stat | row_part | blk_flags | cnt + vpart (one cleared block) | vsplit | ent_rank | tmp_row | tmp_coef
struct LpaScratch { size_t row_stat, row_part, blk_flags, cnt, vpart, clear_bytes, vsplit, ent_rank, tmp_row, tmp_coef, bytes; };
static LpaScratch lpa_scratch(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b) {
    LpaScratch s; Carver c{0};
    const size_t V = d->n_cols, nrc = lp_chunks(b->n_rows), nvc = lp_chunks(d->n_cols);
    s.row_stat = c.take(16 * (size_t)b->n_rows, 16);
    s.row_part = c.take(16 * (nrc + 1), 16);
    s.blk_flags = c.take(4 * (nrc + 1), 16);
    s.cnt = c.take(8 * V, 16);
    s.vpart = c.take(4 * (nvc + 1), 16);
    s.clear_bytes = c.off - s.cnt;
    s.vsplit = c.take(4 * V, 16);
    s.ent_rank = c.take(8 * (size_t)b->row_nnz, 16);
    s.tmp_row = c.take(4 * (size_t)b->n_state_edges, 16);
    s.tmp_coef = c.take(4 * (size_t)b->n_state_edges, 16);
    s.bytes = c.off;
    return s;
}

// the resident dims and the block -> the dims after the append; false where either is malformed or the sums leave int32
static bool lpa_dims_after(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b, gcnn_lp_dims* after) {
    if (!lp_dims_ok(d) || !b) return false;
    if (b->n_rows < 1 || b->row_nnz < 0 || b->n_state_rows < 0 || b->n_state_edges < 0 || b->n_lhs_rows < 0 || b->n_lhs_edges < 0) return false;
    if (b->n_lhs_rows > b->n_rows || b->n_state_rows - b->n_lhs_rows > b->n_rows || b->n_lhs_rows > b->n_state_rows) return false;
    if (b->n_lhs_edges > b->row_nnz || b->n_lhs_edges > b->n_state_edges || (int64_t)b->n_state_edges - b->n_lhs_edges > b->row_nnz) return false;
    if (b->res_lhs_rows < 0 || b->res_lhs_rows > d->n_state_rows || b->res_lhs_edges < 0 || b->res_lhs_edges > d->n_state_edges) return false;
    const int64_t lim = 2147483647;
    if ((int64_t)d->n_rows + b->n_rows >= lim || (int64_t)d->row_nnz + b->row_nnz > lim ||
        (int64_t)d->n_state_edges + b->n_state_edges > lim)
        return false;
    *after = *d;
    after->n_rows += b->n_rows; after->row_nnz += b->row_nnz; after->n_state_rows += b->n_state_rows; after->n_state_edges += b->n_state_edges;
    return lp_dims_ok(after);
}

// more_out: a block behind the append's flag words, for a caller that extends the call (gcnn_lpremove.hpp)
static int lpa_layout(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b, int32_t present, int32_t n_forced, int32_t n_forced_entries,
                      gcnn_lp_append_layout* L, size_t more_out = 0) {
    gcnn_lp_dims after;
    if (!L || !lpa_dims_after(d, b, &after)) return GCNN_E_BADARG;
    memset(L, 0, sizeof(*L));
    const size_t dR = b->n_rows, dN = b->row_nnz;
    // the block in front of the round's upload: row_ptr [dR + 1] from 0, row_col, row_val, row_lhs, row_rhs -- the 8-byte arrays first,
    // so that no array needs padding and the whole block costs at most 255 bytes of alignment
    size_t o = 0;
    L->block_off[2] = o; o += 8 * dN; L->block_off[3] = o; o += 8 * dR; L->block_off[4] = o; o += 8 * dR;
    L->block_off[0] = o; o += 4 * (dR + 1); L->block_off[1] = o; o += 4 * dN;
    L->block_bytes = (o + 255) & ~(size_t)255;
    const int rc = lpr_round_layout(&after, present, n_forced, n_forced_entries, &L->round, 16 + more_out);
    if (rc == GCNN_E_BADARG) return rc;
    L->in_bytes = L->block_bytes + L->round.in_bytes;
    L->flags_off = L->round.out_bytes - 16 - more_out;         // the append's four flag words close the download
    L->out_bytes = L->round.out_bytes;
    L->scratch_bytes = lpa_scratch(d, b).bytes;
    L->round_off = L->block_bytes;
    L->scratch_off = L->round_off + ((L->round.arena_bytes + 255) & ~(size_t)255);
    L->arena_bytes = L->scratch_off + L->scratch_bytes;
    return rc;
}
extern "C" int gcnn_lp_append_layout_for(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b, int32_t present, int32_t n_forced,
                                         int32_t n_forced_entries, gcnn_lp_append_layout* L) {
    return layout_out(L, [&](gcnn_lp_append_layout* l) { return lpa_layout(d, b, present, n_forced, n_forced_entries, l); });
}

static bool lpa_set_ok(const gcnn_lp_rows_set* s, int R, int C, int E) {
    if (!s || !s->l_ptr || !s->v_ptr) return false;
    if (R > 0 && (!s->row_place || !s->row_scale)) return false;
    if (C > 0 && (!s->cons_feats || ((uintptr_t)s->cons_feats & 15))) return false;
    if (E > 0 && (!s->edge_row || !s->edge_col || !s->edge_coef || !s->v_oth || !s->v_coef)) return false;
    return true;
}
static LpaSet lpa_set(const gcnn_lp_rows_set* s) {
    return LpaSet{s->cons_feats, s->edge_row, s->edge_col, s->edge_coef, s->l_ptr, s->v_ptr, s->v_oth, s->v_coef, s->row_place, s->row_scale};
}

// Everything the append enqueues.  blk_*: where the launches read the block (the upload slot with offsets from 0, or the raw rows'
// tail with absolute offsets: ent_base says which); raw_*: non-null in the fused call, where k_lpa_stats copies the block to.
// counts: null, or where the caller keeps the cleared count tables (cnt + vpart, LpaScratch::clear_bytes) and has enqueued their
// fill itself (gcnn_lpedits.hpp: one fill for all sessions).
static int lpa_enqueue(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b, const int* blk_ptr,
                       const int* blk_col, const double* blk_val, const double* blk_lhs, const double* blk_rhs, int nnz_bound, int ent_base,
                       int32_t* const raw[2], double* const rawd[3], const double* col_obj, const gcnn_lp_rows_set* src,
                       const gcnn_lp_rows_set* dst, char* scratch, int32_t* flags_dev, hipStream_t st, char* counts = nullptr) {
    const LpaScratch s = lpa_scratch(d, b);
    LpArgs a; memset(&a, 0, sizeof(a));
    a.row_ptr = blk_ptr; a.row_col = blk_col; a.row_val = blk_val; a.row_lhs = blk_lhs; a.row_rhs = blk_rhs; a.col_obj = col_obj;
    a.R = b->n_rows; a.V = d->n_cols; a.nnz_r = nnz_bound; a.n_model_vars = d->n_model_vars; a.C = b->n_state_rows; a.E1 = b->n_state_edges;
    a.infinity = d->infinity; a.eps = d->sum_epsilon; a.obj_norm = d->obj_norm;
    a.row_stat = (double*)(scratch + s.row_stat); a.row_part = (int*)(scratch + s.row_part); a.cut_part = a.row_part;
    a.blk_flags = (int*)(scratch + s.blk_flags);
    a.nrc = lp_chunks(a.R); a.n_stat_blocks = a.nrc;
    LpaArgs x; memset(&x, 0, sizeof(x));
    x.src = lpa_set(src); x.dst = lpa_set(dst);
    x.R0 = d->n_rows; x.N0 = d->row_nnz; x.C0 = d->n_state_rows; x.E0 = d->n_state_edges; x.L0 = b->res_lhs_rows; x.EL0 = b->res_lhs_edges;
    x.dR = b->n_rows; x.dN = b->row_nnz; x.dC = b->n_state_rows; x.dE = b->n_state_edges; x.dL = b->n_lhs_rows; x.dEL = b->n_lhs_edges;
    x.V = d->n_cols; x.nvc = lp_chunks(x.V); x.ent_base = ent_base;
    if (raw) { x.raw_ptr = raw[0]; x.raw_col = raw[1]; x.raw_val = rawd[0]; x.raw_lhs = rawd[1]; x.raw_rhs = rawd[2]; }
    char* cnt = counts ? counts : scratch + s.cnt;
    x.cnt = (int*)cnt; x.vpart = (int*)(cnt + (s.vpart - s.cnt)); x.vsplit = (int*)(scratch + s.vsplit);
    x.ent_rank = (int*)(scratch + s.ent_rank); x.tmp_row = (int*)(scratch + s.tmp_row); x.tmp_coef = (float*)(scratch + s.tmp_coef);
    x.nb_new = a.nrc; x.nb_rows = lp_chunks(x.C0); x.nb_edges = lp_chunks(x.E0); x.nb_lprows = lp_chunks(x.R0);
    x.flags_out = flags_dev;
    if (!counts) HIPCHK(hipMemsetAsync(cnt, 0, s.clear_bytes, st));      // the count tables (no launch of the library's own)
    {
        ProfScope prof("k_lpa_stats", st);
        GCNN_LAUNCH(k_lpa_stats, dim3(a.nrc), dim3(LP_NT), 0, st, a, x);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_lpa_scan", st);
        GCNN_LAUNCH(k_lpa_scan, dim3(lp_chunks(x.V + 1)), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    {
        ProfScope prof("k_lpa_move", st);
        GCNN_LAUNCH(k_lpa_move, dim3(x.nb_new + x.nb_rows + x.nb_edges + x.nb_lprows + 1), dim3(LP_NT), 0, st, a, x);
        LAUNCHCHK();
    }
    if (x.V > 0 && x.dE > 0) {
        ProfScope prof("k_lpa_order", st);
        GCNN_LAUNCH(k_lpa_order, dim3((x.V + LP_NT / LP_SUB - 1) / (LP_NT / LP_SUB)), dim3(LP_NT), 0, st, x);
        LAUNCHCHK();
    }
    return 0;
}

static int lpa_check(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b, gcnn_lp_dims* after, const void* row_ptr, const void* row_col,
                     const void* row_val, const void* row_lhs, const void* row_rhs, const double* col_obj,
                     const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst) {
    if (!lpa_dims_after(d, b, after)) return GCNN_E_BADARG;
    if (!row_ptr || !row_lhs || !row_rhs || (after->row_nnz > 0 && (!row_col || !row_val)) || (d->n_cols > 0 && !col_obj)) return GCNN_E_BADARG;
    if (!lpa_set_ok(src, d->n_rows, d->n_state_rows, d->n_state_edges)) return GCNN_E_BADARG;
    if (!lpa_set_ok(dst, after->n_rows, after->n_state_rows, after->n_state_edges)) return GCNN_E_BADARG;
    if (after->n_state_edges > 0 && (after->n_cols == 0 || after->n_state_rows == 0)) return GCNN_E_BADARG;
    if (after->n_state_rows > (1 << 24) || after->n_cols > (1 << 24)) return GCNN_E_UNSUPPORTED;
    return 0;
}

extern "C" int gcnn_lp_rows_append(const gcnn_lp_dims* d, const gcnn_lp_append_dims* b, const int32_t* row_ptr, const int32_t* row_col,
                                   const double* row_val, const double* row_lhs, const double* row_rhs, const double* col_obj,
                                   const gcnn_lp_rows_set* src, const gcnn_lp_rows_set* dst, void* scratch, size_t scratch_bytes,
                                   int32_t* flags, void* stream) {
    gcnn_lp_dims after;
    const int rc = lpa_check(d, b, &after, row_ptr, row_col, row_val, row_lhs, row_rhs, col_obj, src, dst);
    if (rc) return rc;
    if (!scratch || ((uintptr_t)scratch & 15) || !flags) return GCNN_E_BADARG;
    if (scratch_bytes < lpa_scratch(d, b).bytes) return GCNN_E_WORKSPACE;
    return lpa_enqueue(d, b, row_ptr + d->n_rows, row_col, row_val, row_lhs + d->n_rows, row_rhs + d->n_rows, after.row_nnz,
                       d->row_nnz, nullptr, nullptr, col_obj, src, dst, (char*)scratch, flags, (hipStream_t)stream);
}
