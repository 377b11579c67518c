// gcnn_ibatch.hpp -- host side of gcnn_infer_batch (include/gcnn_hip.h): 1..64 host states in one upload, one forward pass over their
// disjoint union, one download.  Included from gcnn_capi.hip's list of host files (it shares that file's statics: ProfScope, the
// carver, by_key_stage, forward_impl; and gcnn_select.hpp's call_check, sel_args and launcher), kept apart so that its launch names
// form their own inventory (tests/test_ibatch_build.py).  It also holds what every call on a union shares -- gcnn_lpbatch.hpp and
// gcnn_mbatch.hpp, included after it, use them: the sums and the table (ibatch_sums), the one layout (union_layout), where an
// uploaded union lies (union_at), the index pass's arguments and grid (union_args, union_grid) and the end of a run (union_tail).
//
// By-variable order of the union: the by-variable stage of gcnn_graph_build (by_key_stage: a stable rocprim radix sort of (variable
// id, input position), k_seg_offsets and k_gather_edges) on the shifted list, not a generalised k_iplan_*.  The single-state plan
// scans its per-variable counts in one block's LDS (32,768 variables) and ranks each variable's segment quadratically (2,048
// edges); a union of 64 states passes the first bound at BASELINE sizes, and lifting it needs a device-wide scan, i.e. what the
// radix sort already is.  The sort is stable, so the plan equals what BipartiteGraph builds from the collated union, and it has
// no degree limit.  The by-left stage of gcnn_graph_build is not used: k_ib_unpack finds those offsets state by state, which
// keeps a state with bad or unsorted ids from moving a neighbour's segments (k_ibatch.hpp).
#include "k_ibatch.hpp"

static_assert(IB_MAX_STATES == GCNN_IBATCH_MAX && IB_TS == GCNN_IBATCH_TABLE_STRIDE && IB_COLS == GCNN_IBATCH_TABLE_COLS, "table shape");
static_assert(IB_TS >= IB_MAX_STATES + 1 && IB_TS % 4 == 0, "one offset per state and the total, 16-byte columns");

struct IbSums {
    long long c, v, k, e1, e2, f, fe; int max_cuts;
    gcnn_dims dims() const { return gcnn_dims{(int)c, (int)v, (int)k, (int)e1, (int)e2}; }   // the union's totals
};
static int ibatch_sums(int n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode,
                       IbSums* t, int32_t* table) {
    if (n_states < 1 || n_states > GCNN_IBATCH_MAX || !dims) return GCNN_E_BADARG;
    if (mode < GCNN_IBATCH_SCORES || mode > GCNN_IBATCH_SELECT) return GCNN_E_BADARG;
    IbSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i <= n_states; ++i) {
        if (table) {
            table[IB_C * IB_TS + i] = (int)s.c; table[IB_V * IB_TS + i] = (int)s.v; table[IB_K * IB_TS + i] = (int)s.k;
            table[IB_E1 * IB_TS + i] = (int)s.e1; table[IB_E2 * IB_TS + i] = (int)s.e2;
            table[IB_F * IB_TS + i] = (int)s.f; table[IB_FE * IB_TS + i] = (int)s.fe;
        }
        if (i == n_states) break;
        const gcnn_dims& d = dims[i];
        const int nf = (mode == GCNN_IBATCH_SELECT && n_forced) ? n_forced[i] : 0;
        const int nfe = (mode == GCNN_IBATCH_SELECT && n_forced_entries) ? n_forced_entries[i] : 0;
        if (d.n_cons < 0 || d.n_vars < 0 || d.n_cuts < 0 || d.n_cons_edges < 0 || d.n_cut_edges < 0 || nf < 0 || nfe < 0) return GCNN_E_BADARG;
        if (nf == 0 && nfe > 0) return GCNN_E_BADARG;
        // edges with nothing to point at: every id would be out of range and there is no node of the state's own to park them on
        if (edges_without_nodes(d)) return GCNN_E_UNSUPPORTED;
        s.c += d.n_cons; s.v += d.n_vars; s.k += d.n_cuts; s.e1 += d.n_cons_edges; s.e2 += d.n_cut_edges; s.f += nf; s.fe += nfe;
        if (d.n_cuts <= SEL_MAX_CUTS) s.max_cuts = std::max(s.max_cuts, d.n_cuts);
        // (checked as the sums grow, so that the table's int32 entries cannot wrap)
        if (s.c > (1 << 24) || s.v > (1 << 24) || s.k > (1 << 24) || s.e1 > (1 << 30) || s.e2 > (1 << 30) || s.f > (1 << 24) || s.fe > (1 << 30))
            return GCNN_E_UNSUPPORTED;
    }
    if (t) *t = s;
    return 0;
}

// union_layout: the one layout of a union of t's sizes -- every offset of gcnn_ibatch_layout.  What tells gcnn_infer_batch's union
// from gcnn_infer_models': `n_close` closing by-left and by-variable entries (1, or one per model), `table_bytes`, `sel_offsets`
// (the zero block also carries the cut rows' offsets over the whole union), `fwd_ws_bytes` (dev_off[12]) and `extra` arena blocks
// behind the selection workspace, whose offsets go to `extra_off`.
static void union_layout(const IbSums& t, int n_states, int mode, size_t n_close, size_t table_bytes, bool sel_offsets, size_t fwd_ws_bytes,
                         std::initializer_list<size_t> extra, size_t* extra_off, gcnn_ibatch_layout* L) {
    L->total = t.dims();
    L->n_forced = (int)t.f; L->n_forced_entries = (int)t.fe; L->max_cuts = t.max_cuts; L->n_states = n_states;
    const size_t S = n_states, M = n_close, C = t.c, V = t.v, K = t.k, E1 = t.e1, E2 = t.e2, F = t.f, FE = t.fe;
    // the table; the zero block: flags | l_ptr cons | l_ptr cut | the union's cut offsets; the seven arrays of gcnn_infer's upload,
    // stacked; the forced rows
    const size_t sizes[9] = {table_bytes, al16(16 * S) + al16(4 * (C + M)) + al16(4 * (K + M)) + (sel_offsets ? al16(4 * (K + 1)) : 0),
                             16 * C, 8 * E1, 4 * E1, 56 * V, 24 * K, 8 * E2, 4 * E2};
    Carver in{0};
    for (int i = 0; i < 9; ++i) L->in_off[i] = in.take(sizes[i], 16);
    forced_block(in, F, FE, &L->in_off[9]);
    L->in_bytes = in.off;
    L->out_off[0] = 0; L->out_off[1] = al16(4 * K); L->out_off[2] = L->out_off[1] + al16(4 * K);
    L->out_off[3] = L->out_off[2] + al16(4 * S);
    L->out_bytes = L->out_off[3] + 16 * S;
    // left: union row ids of the constraint edges | var, constraint edges (= by-left oth) | var, cut edges | iota | sorted keys |
    // permutation | v_ptr | v_oth | v_coef | forced columns in the union's column space | sort temp | outputs | forward workspace |
    // selection workspace
    const size_t blocks[14] = {4 * E1, 4 * E1, 4 * E2, 4 * E1, 4 * E1, 4 * E1, 4 * (V + M), 4 * E1, 4 * E1, 4 * FE,
                               sort_temp_bytes((int)E1), L->out_bytes, fwd_ws_bytes,
                               mode == GCNN_IBATCH_SELECT ? select_ws_bytes((int)K, (int)F, t.max_cuts) : 0};
    Carver dev{(in.off + 255) & ~(size_t)255};
    for (int i = 0; i < 14; ++i) L->dev_off[i] = dev.take(blocks[i], 256);
    for (size_t bytes : extra) *extra_off++ = dev.take(bytes, 256);
    L->arena_bytes = dev.off;
}

static int ibatch_layout(int n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int mode,
                         gcnn_ibatch_layout* L) {
    if (!L) return GCNN_E_BADARG;
    IbSums t;
    const int rc = ibatch_sums(n_states, dims, n_forced, n_forced_entries, mode, &t, nullptr);
    if (rc) return rc;
    memset(L, 0, sizeof(*L));
    const gcnn_dims total = t.dims();
    union_layout(t, n_states, mode, 1, 4 * (size_t)IB_COLS * IB_TS, false, sizeof(float) * gcnn_workspace_floats(&total), {}, nullptr, L);
    return 0;
}

extern "C" int gcnn_infer_batch_layout_for(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced,
                                           const int32_t* n_forced_entries, int32_t mode, gcnn_ibatch_layout* L) {
    return layout_out(L, [&](gcnn_ibatch_layout* l) { return ibatch_layout(n_states, dims, n_forced, n_forced_entries, mode, l); });
}

extern "C" int gcnn_infer_batch_fill_table(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced,
                                           const int32_t* n_forced_entries, int32_t* table) {
    if (!table) return GCNN_E_BADARG;
    // (forced rows are counted whenever they are given: a table filled for SELECT serves the other modes too; checked in full before
    // the first word is written: a refused call leaves the table as it was)
    const int rc = ibatch_sums(n_states, dims, n_forced, n_forced_entries, GCNN_IBATCH_SELECT, nullptr, nullptr);
    return rc ? rc : ibatch_sums(n_states, dims, n_forced, n_forced_entries, GCNN_IBATCH_SELECT, nullptr, table);
}

// Where a union lies in device memory: the table, the zero block, the seven stacked arrays, the forced rows and the output block.
// gcnn_infer_batch uploads all of them as one block at the arena's start; gcnn_lp_batch (gcnn_lpbatch.hpp) uploads the table and the
// forced rows with its snapshots and builds the seven arrays in place.  The plan and the workspaces are at L.dev_off in either case.
struct IbAt {
    const int* table; char* zero; const char* arr[7];   // arr: gcnn_ibatch_layout.in_off[2..8]
    const char* forced[3];                               // in_off[9..11]
    char* out;                                           // scores | order | n_kept | flags, at L.out_off
};

// what the forward pass itself would refuse, before anything is enqueued
static int ibatch_precheck(const gcnn_ibatch_layout& L, const float* params, void* arena) {
    layout_init();
    gcnn_graph g; memset(&g, 0, sizeof(g));
    return check_common(&L.total, params, &g, &g, (float*)arena, gcnn_workspace_floats(&L.total));
}

// an upload that lies at the arena's start (gcnn_infer_batch, gcnn_infer_models)
static IbAt union_at(char* A, const gcnn_ibatch_layout& L) {
    IbAt at;
    at.table = (const int*)(A + L.in_off[0]); at.zero = A + L.in_off[1];
    for (int i = 0; i < 7; ++i) at.arr[i] = A + L.in_off[2 + i];
    for (int i = 0; i < 3; ++i) at.forced[i] = A + L.in_off[9 + i];
    at.out = A + L.dev_off[11];
    return at;
}

// the index pass's arguments for a union at `at` whose by-left arrays carry `n_close` closing entries each (union_layout)
static IbArgs union_args(const IbAt& at, const gcnn_ibatch_layout& L, char* A, size_t n_close) {
    IbArgs ia; memset(&ia, 0, sizeof(ia));
    ia.table = at.table; ia.n_states = L.n_states;
    ia.packed[0] = (const int*)at.arr[1]; ia.packed[1] = (const int*)at.arr[5];
    ia.left = (int*)(A + L.dev_off[0]); ia.var[0] = (int*)(A + L.dev_off[1]); ia.var[1] = (int*)(A + L.dev_off[2]);
    ia.flags = (int*)at.zero;
    ia.l_ptr[0] = (int*)(at.zero + al16(16 * (size_t)L.n_states));
    ia.l_ptr[1] = ia.l_ptr[0] + al16(4 * ((size_t)L.total.n_cons + n_close)) / 4;
    ia.iota = (int*)(A + L.dev_off[3]);
    ia.f_col_in = (const int*)at.forced[1]; ia.f_col = (int*)(A + L.dev_off[9]);
    return ia;
}

// the index pass's grid: one item per edge of either set, one closing position per state and set, one per forced entry
static dim3 union_grid(const gcnn_ibatch_layout& L) {
    const long long items = (long long)L.total.n_cons_edges + L.total.n_cut_edges + 2 * L.n_states + L.n_forced_entries;
    return dim3((unsigned)std::min<long long>((items + 255) / 256, 1024));
}

// union_tail: how a run on a union ends -- in selection mode the launch pair over all states (`cut_ptr`: the cut rows' offsets
// over the whole union), then the flags into the output block.
static int union_tail(int mode, const gcnn_ibatch_layout& L, char* A, const IbAt& at, const IbArgs& ia, const int* cut_ptr,
                      double p_max, double p_max_ub, hipStream_t st) {
    if (mode == GCNN_IBATCH_SELECT) {
        SelArgs a = sel_args((const float*)(at.out + L.out_off[0]),
                             SelRows{cut_ptr, ia.var[1], (const float*)at.arr[6], at.table + IB_K * IB_TS},
                             SelRows{(const int*)at.forced[0], ia.f_col, (const float*)at.forced[2],
                                     L.n_forced > 0 ? at.table + IB_F * IB_TS : nullptr},
                             L.n_states, L.total.n_cuts, L.n_forced, L.max_cuts, L.total.n_vars, p_max, p_max_ub, A + L.dev_off[13],
                             (int*)(at.out + L.out_off[1]), (int*)(at.out + L.out_off[2]));
        const int rc = launch_select(a, st);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(at.out + L.out_off[3], ia.flags, 16 * (size_t)L.n_states, hipMemcpyDeviceToDevice, st));
    return 0;
}

// ibatch_run: everything of gcnn_infer_batch between its upload and its download, on a union that lies at `at` (infer_run's
// counterpart): the index pass, the by-variable stage, ONE forward pass, ranking or selection, the flags into the output block.
static int ibatch_run(int n_states, int mode, const gcnn_ibatch_layout& L, const float* params, char* A, const IbAt& at, double p_max,
                      double p_max_ub, hipStream_t st) {
    int rc;
    const gcnn_dims& T = L.total;
    const int E1 = T.n_cons_edges, V = T.n_vars;
    const IbArgs ia = union_args(at, L, A, 1);
    {
        ProfScope prof("k_ib_unpack", st);
        hipLaunchKernelGGL(k_ib_unpack, union_grid(L), dim3(256), 0, st, ia);
        LAUNCHCHK();
    }
    gcnn_graph cg, kg; memset(&cg, 0, sizeof(cg)); memset(&kg, 0, sizeof(kg));
    cg.l_ptr = ia.l_ptr[0]; cg.l_oth = ia.var[0]; cg.l_coef = (const float*)at.arr[2];
    cg.v_ptr = (int*)(A + L.dev_off[6]); cg.v_oth = (int*)(A + L.dev_off[7]); cg.v_coef = (float*)(A + L.dev_off[8]);
    kg.l_ptr = ia.l_ptr[1]; kg.l_oth = ia.var[1]; kg.l_coef = (const float*)at.arr[6];
    kg.v_ptr = cg.v_ptr;   // never read: conv v->k gathers by cut only and nothing is differentiated
    if (E1 > 0) {          // gcnn_graph_build's by-variable stage on the union's list
        ProfScope prof("k_ib_by_variable", st);
        if ((rc = by_key_stage(A + L.dev_off[10], sort_temp_bytes(E1), ia.var[0], ia.iota, (int*)(A + L.dev_off[4]), (int*)(A + L.dev_off[5]),
                               V, E1, ia.left, cg.l_coef, (int*)cg.v_ptr, (int*)cg.v_oth, (float*)cg.v_coef, st))) return rc;
    } else {
        HIPCHK(hipMemsetAsync((void*)cg.v_ptr, 0, ((size_t)V + 1) * sizeof(int), st));
    }
    float* scores = (float*)(at.out + L.out_off[0]);
    // ONE forward pass over the union (the longest segments are not known here: 0)
    rc = forward_impl(&T, params, (const float*)at.arr[0], (const float*)at.arr[3], (const float*)at.arr[4],
                      &cg, &kg, (float*)(A + L.dev_off[12]), gcnn_workspace_floats(&T), scores, 0, nullptr, 0.f, st);
    if (rc) return rc;
    if (mode == GCNN_IBATCH_RANK && T.n_cuts > 0) {
        ProfScope prof("k_ib_rank", st);
        hipLaunchKernelGGL(k_ib_rank, dim3(n_states), dim3(256), 0, st, (const float*)scores, at.table, (int*)(at.out + L.out_off[1]));
        LAUNCHCHK();
    }
    return union_tail(mode, L, A, at, ia, kg.l_ptr, p_max, p_max_ub, st);
}

extern "C" int gcnn_infer_batch(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                int32_t mode, const float* params, const void* host_in, void* host_out, void* arena,
                                size_t arena_bytes, double p_max, double p_max_ub, void* stream) {
    gcnn_ibatch_layout L;
    int rc = ibatch_layout(n_states, dims, n_forced, n_forced_entries, mode, &L);
    if (rc) return rc;
    if ((rc = call_check(params, host_in, host_out, arena, arena_bytes, L.arena_bytes, mode == GCNN_IBATCH_SELECT, p_max, p_max_ub))) return rc;
    if ((rc = ibatch_precheck(L, params, arena))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* A = (char*)arena;
    HIPCHK(hipMemcpyAsync(A, host_in, L.in_bytes, hipMemcpyHostToDevice, st));   // ONE upload
    const IbAt at = union_at(A, L);
    if ((rc = ibatch_run(n_states, mode, L, params, A, at, p_max, p_max_ub, st))) return rc;
    HIPCHK(hipMemcpyAsync(host_out, at.out, L.out_bytes, hipMemcpyDeviceToHost, st));   // ONE download: scores | order | n_kept | flags
    return 0;
}
