"""The graph plans of the inference calls, restated in NumPy, and the cases that put every seam of their launches on the line.

Two plans build their structures on the device with code no other path uses: the single-state plan of gcnn_infer (k_infer.hpp:
count, scan + place, order -- extra blocks of k_infer_s1/s2/s3, or k_iplan_place / k_iplan_order) and the union plan of
gcnn_infer_batch (k_ibatch.hpp: k_ib_unpack, then the stable by-variable stage).  Both are integer data plus copied floats, so
`plan_single` and `plan_union` restate them entry by entry: the three steps of the kernels on bounds-checked arrays (`Arr`: any
index outside [0, n) raises `OutOfBounds`, where NumPy would wrap a negative one), together with the launch formulas of
gcnn_capi.hip / gcnn_ibatch.hpp and the maps that say which block, thread and trip of a launch handles a position, an edge or a
variable.  tests/test_plancases.py proves the restatement against plain NumPy statements, pins every formula to the source text,
proves that each case sits on the seam it names and that each defect of `DEFECTS` changes a named output of a named case;
tests/test_gpu_plan_seams.py runs the cases on the device.  NumPy only."""
from __future__ import annotations

import functools

import numpy as np

f32, i32 = np.float32, np.int32
INT_MAX = 0x7FFFFFFF
POISON = int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])      # what an unwritten word of the poisoned arena reads as
MAX_VARS, MAX_DEG, FUSE_MAX_VARS, LDS_DEG = 32768, 2048, 4096, 256      # IPLAN_* of k_infer.hpp
FUSE_MAX_ROWS = 16384                                                   # launch_edge_fwd: a.n_own <= 16384
IB_MAX_STATES = 64

# Defects the restatement can be given (tests/test_plancases.py: each must change a named output of a named case).  A run of the
# suite with one of them added to ACTIVE is how "the GPU test would notice" is checked by hand; it is empty in the repository.
DEFECTS = ("count_lt", "per_floor", "no_pre_n", "no_wave_base", "pad_zero", "lds_lt", "maxdeg_ge", "order_one_trip", "place_one_trip",
           "no_clamp_lptr", "no_clamp_var", "no_clamp_voth", "ib_lptr0_from_data", "ib_rows_from_0", "ib_search_lt",
           "ib_no_clamp_var", "ib_no_clamp_left")
ACTIVE: frozenset = frozenset()


class OutOfBounds(IndexError):
    pass


class Arr:
    """A 1-D array that refuses every index outside [0, n)."""

    def __init__(self, name, n=None, fill=POISON, dtype=np.int64, data=None):
        self.name = name
        self.a = np.full(n, fill, dtype) if data is None else np.array(data, dtype)

    def _chk(self, i):
        i = np.asarray(i)
        if i.size and (int(i.min()) < 0 or int(i.max()) >= self.a.size):
            raise OutOfBounds(f"{self.name}[{int(i.min())}..{int(i.max())}] of {self.a.size}")
        return i

    def __getitem__(self, i):
        return self.a[self._chk(i)]

    def __setitem__(self, i, v):
        self.a[self._chk(i)] = v

    def add(self, i, v=1):
        np.add.at(self.a, self._chk(i), v)


def cdiv(a, b):
    return -(-a // b)


# ---- launch formulas (gcnn_capi.hip, gcnn_ibatch.hpp); SOURCE_PINS holds the text each one restates ---------------------------------
SOURCE_PINS = {
    "gcnn_capi.hip": (
        'const int max_tiles = GCNN_KNOB("GCNN_SPLIT_MAX_TILES", 256);',
        "const int t = n[i] > 0 ? cdiv(n[i], 16) : 0; total += t;",
        "return total <= max_tiles;",
        "if (rows_split(n, ngroups, blk0)) return RowsForm{true, 4};",
        "const int nwaves = (forced == 4 || forced == 8) ? forced : (total > 1024 ? 8 : 4);",
        "const int n[3] = {m.v.n, m.c.n, m.k.n}, ns[3] = {4, 3, 3};",
        "plan->blocks0 = std::min(cdiv(plan->s[0].n_edges + 1, f.nwaves * 64), 32);",
        "plan->blocks1 = std::min(cdiv(plan->s[1].n_edges + 1, f.nwaves * 64), 8);",
        "return launch_rows(g_infer_s1, f, m.blk0[3] + 3 + plan->blocks0 + plan->blocks1, st, m, *plan);",
        "if (!count && a.n_own <= 16384 && plan->n_vars <= IPLAN_FUSE_MAX_VARS) {",
        "const int place_blocks = std::max(1, std::min(cdiv(plan->s[0].n_edges, 256), 256));",
        "dim3(std::max(1, std::min(cdiv(ia.s[0].n_edges, 1024), 64))), dim3(1024)",
        "const RowsForm f = rows_form(&a.n, &ns, 1, blk0);",
        "if (plan && tail == CF_PROJ && plan->n_vars <= IPLAN_FUSE_MAX_VARS) {",
        "const int grid = blk0[1] + std::min(cdiv(plan->n_vars, f.nwaves * 4), 48);",
        "hipLaunchKernelGGL(k_iplan_order, dim3(std::min(cdiv(plan->n_vars, 16), 2048)), dim3(256), 0, st, *plan);",
        "return launch(r.name, r.k[i], r.lds_once[i], 120 * 1024, grid, f.nwaves * 64,",
        "if (d->n_vars > IPLAN_MAX_VARS) return GCNN_E_UNSUPPORTED;",
    ),
    "gcnn_ibatch.hpp": (
        "const long long items = (long long)L.total.n_cons_edges + L.total.n_cut_edges + 2 * L.n_states + L.n_forced_entries;",
        "return dim3((unsigned)std::min<long long>((items + 255) / 256, 1024));",
        "hipLaunchKernelGGL(k_ib_unpack, union_grid(L), dim3(256), 0, st, ia);",
        "if (E1 > 0) {          // gcnn_graph_build's by-variable stage on the union's list",
    ),
    "k_infer.hpp": (
        "#define IPLAN_MAX_VARS 32768", "#define IPLAN_MAX_DEG 2048", "#define IPLAN_FUSE_MAX_VARS 4096", "#define IPLAN_LDS_DEG 256",
        "for (int i = lb * nt + (int)threadIdx.x; i <= s.n_edges; i += nb * nt) {",
        "const int lo = i == 0 ? -1 : min(max(left[i - 1], -1), s.n_left);",
        "const int hi = i == s.n_edges ? s.n_left : min(max(left[i], -1), s.n_left);",
        "if (bad_v) { v = 0; var[i] = 0; }",
        "if (set == 0 && a.n_vars > 0) atomicAdd(&a.vcount[v], 1);",
        "const int per = (n + NT - 1) / NT, b = min(n, t * per), e = min(n, b + per);",
        "for (int w = 0; w < wv; ++w) base += wsum[w];",
        "if (t == NT - 1) pre[n] = base + sum;",
        "for (int e = bid * NT + threadIdx.x; e < n; e += nblk * NT) {",
        "iplan_place_body<1024>(a, pre, blockIdx.x, gridDim.x);",
        "iplan_place_body<256>(ia, pre, b - edge_blocks, gridDim.x - edge_blocks)",
        "for (int v = bid * (NT / 16) + grp; v < a.n_vars; v += nblk * (NT / 16)) {",
        "if (n > IPLAN_MAX_DEG) {", "} else if (n <= IPLAN_LDS_DEG) {", "const int n4 = (n + 3) & ~3;",
        "seg[grp][k] = k < n ? a.v_pos[beg + k] : 0x7fffffff;",
        "a.v_oth[beg + rank] = min(max(left[x], 0), max(n_left - 1, 0));",
        "iplan_order_body<256>(a, blockIdx.x, gridDim.x)", "iplan_order_body<NWAVES * 64>(ia, b - conv_blocks, gridDim.x - conv_blocks);",
        "else iplan_count_body(ia, b - m.blk0[3] - 3, NWAVES * 64);",
    ),
    "k_ibatch.hpp": (
        "#define IB_MAX_STATES 64",
        "const long long n1 = (long long)tab[IB_E1][S] + S, n2 = (long long)tab[IB_E2][S] + S, nf = tab[IB_FE][S];",
        "for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {",
        "while (hi - s > 1) { const int mid = (s + hi) >> 1; if (tab[IB_FE][mid] <= i) s = mid; else hi = mid; }",
        "while (hi - s > 1) { const int mid = (s + hi) >> 1; if (eoff[mid] + mid <= item) s = mid; else hi = mid; }",
        "int vr = tab[IB_V][s];",
        "a.f_col[i] = (c >= 0 && c < nv) ? c + vr : -1;",
        "int m = 0, er = e0, lr = l0, vr = v0;",                 # without models: the union's own offsets
        "int* l_ptr = a.l_ptr[set] + l0 + m;",
        "l_ptr[0] = er;",
        "const int lo = j == 0 ? -1 : min(max(src[j - 1], -1), n_left);",
        "const int hb = j == E ? n_left : min(max(src[j], -1), n_left);",
        "for (int k = max(lo + 1, 1); k <= min(hb, n_left - 1); ++k) {",
        "l_ptr[k] = er + j;",
        "a.var[set][e0 + j] = vr + (bad_v ? 0 : v);",
        "a.left[e0 + j] = lr + min(max(l, 0), max(n_left - 1, 0));",
        "ib_unpack_body<false>(a, tab, nullptr, nullptr, nullptr);",
    ),
}


def rows_waves(n):
    """Waves per block of a row launch over row sets `n` (rows_form): the split form (one block of four waves per tile) while
    the tiles number at most 256, else blocks of eight waves past 1,024 tiles and of four below."""
    tiles = sum(cdiv(x, 16) if x > 0 else 0 for x in n)
    return 4 if tiles <= 256 else (8 if tiles > 1024 else 4)


def launch_single(C, V, K, E1, E2):
    """What gcnn_infer launches for the plan: per step its form, threads per block and blocks."""
    nt = 64 * rows_waves((V, C, K))                      # launch_embed_fwd: the count step rides in the embedding launch
    L = dict(count_nt=nt, blocks0=min(cdiv(E1 + 1, nt), 32), blocks1=min(cdiv(E2 + 1, nt), 8))
    L["place_fused"] = C <= FUSE_MAX_ROWS and V <= FUSE_MAX_VARS
    L["place_nt"] = 256 if L["place_fused"] else 1024
    L["place_blocks"] = max(1, min(cdiv(E1, 256), 256)) if L["place_fused"] else max(1, min(cdiv(E1, 1024), 64))
    L["order_fused"] = V <= FUSE_MAX_VARS
    w3 = rows_waves((C,))                                # launch_conv_fwd of conv v->c: its rows are the constraints
    L["order_groups"] = 4 * w3 if L["order_fused"] else 16
    L["order_blocks"] = min(cdiv(V, 4 * w3), 48) if L["order_fused"] else min(cdiv(V, 16), 2048)
    L["names"] = ["k_infer_s1 (embeddings + plan: count)",
                  "k_infer_s2 (conv v->c edge pass + plan: place)" if L["place_fused"] else "k_iplan_place",
                  "k_infer_s3 (conv row program + plan: order)" if L["order_fused"] else "k_iplan_order"]
    return L


def count_where(i, nt, nb):
    """(block, thread, trip) of position i of an edge set's count sweep over nb blocks of nt threads."""
    return (i % (nb * nt)) // nt, i % nt, i // (nb * nt)


def scan_where(v, V, nt):
    """(thread, wave, position inside the thread's chunk, per) of variable v in the scan of V counts by nt threads."""
    per = cdiv(V, nt)
    return v // per, v // per // 64, v % per, per


def place_where(e, L):
    return count_where(e, L["place_nt"], L["place_blocks"])


def order_where(v, L):
    """(block, lane group, trip) of variable v in the order step."""
    g, nb = L["order_groups"], L["order_blocks"]
    return (v % (nb * g)) // g, v % g, v // (nb * g)


def unpack_launch(items):
    return min(cdiv(items, 256), 1024)


def unpack_where(item, items):
    return count_where(item, 256, unpack_launch(items))


# ---- the packer (gcnn_host_pack_edges): what the upload holds ------------------------------------------------------------------------
def pack(ei, ef, n_left):
    """([2,E] int32 as uploaded, [E] fp32): a list not sorted by row is stably sorted by row -- unless a row id is out of range,
    then it travels as it is and the device reports it."""
    ei, ef = np.asarray(ei, i32).reshape(2, -1), np.asarray(ef, f32).reshape(-1)
    rows = ei[0]
    if rows.size and (np.diff(rows) < 0).any() and rows.min() >= 0 and rows.max() < n_left:
        p = np.argsort(rows, kind="stable")
        return ei[:, p], ef[p]
    return ei, ef


# ---- the single-state plan ---------------------------------------------------------------------------------------------------------
def _clamp(x, lo, hi):
    return min(max(x, lo), hi)


def _range_writes(arr, lo, hi, val, writers):
    """arr[k] = val[i] for every k in [lo[i], hi[i]], in the order of i; `writers` collects (k, value) of every write."""
    n = np.maximum(hi - lo + 1, 0)
    k = np.repeat(lo, n) + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    v = np.repeat(val, n)
    arr[k] = v                                      # (NumPy keeps the last of repeated indices: the highest position)
    writers.append((k, v))


def _contested(writers):
    """{entry: set of values} for the entries that writes of different values reach (only a list out of order has any): the
    device keeps whichever lands last."""
    if not writers:
        return {}
    kv = np.unique(np.stack([np.concatenate([k for k, _ in writers]), np.concatenate([v for _, v in writers])], 1), axis=0)
    ks, n = np.unique(kv[:, 0], return_counts=True)
    return {int(k): {int(x) for x in kv[kv[:, 0] == k, 1]} for k in ks[n > 1]}


def _count(set_id, inds, E, n_left, V, l_ptr, vcount, flags, D):
    """iplan_count_body over one edge set: the launch's blocks and trips cover the positions 0..E once.  Returns the contested
    by-left offsets."""
    clamp = (lambda x: x) if "no_clamp_lptr" in D else (lambda x: np.clip(x, -1, n_left))
    pos = np.arange(E + (0 if "count_lt" in D else 1))
    left, var = inds[np.arange(E)], inds[E + np.arange(E)]
    lo = np.where(pos == 0, -1, clamp(np.concatenate([[-1], left])[pos]))
    hi = np.where(pos == E, n_left, clamp(np.concatenate([left, [n_left]])[pos]))
    bad_v = (var < 0) | (var >= V)
    flags[0] |= int(((left < 0) | (left >= n_left) | bad_v).any())
    flags[1 + set_id] |= int((np.diff(left) < 0).any())
    if "no_clamp_var" not in D:
        var = np.where(bad_v, 0, var)
        inds[E + np.arange(E)] = var
    if set_id == 0 and V > 0:
        vcount.add(var)
    writers = []
    _range_writes(l_ptr, lo + 1, hi, pos, writers)
    return _contested(writers)


def scan(cnt, n, nt, D=frozenset()):
    """iplan_scan: `pre` (n + 1 entries, the total last) of the counts, by nt threads in waves of 64."""
    pre = Arr("pre", n + 1)
    if n:
        pre[np.arange(n)] = cnt[np.arange(n)]
    per = n // nt if "per_floor" in D else cdiv(n, nt)
    sums, spans = np.zeros(nt, np.int64), []
    for t in range(nt):
        b = min(n, t * per)
        e = min(n, b + per)
        spans.append((b, e))
        if e > b:
            idx = np.arange(b, e)
            c = pre[idx]
            pre[idx] = np.cumsum(c) - c
            sums[t] = c.sum()
    inc = np.cumsum(sums.reshape(-1, 64), 1)                       # inclusive over each wave
    wbase = np.concatenate([[0], np.cumsum(inc[:, 63])[:-1]])        # the waves before
    base = inc.reshape(-1) - sums + (0 if "no_wave_base" in D else np.repeat(wbase, 64))
    for t, (b, e) in enumerate(spans):
        if e > b:
            pre.add(np.arange(b, e), base[t])
    if "no_pre_n" not in D:
        pre[n] = base[nt - 1] + sums[nt - 1]
    return pre


def plan_single(C, V, K, ei1, ef1, ei2, D=None):
    """The plan gcnn_infer leaves in the arena for packed lists ei1 [2,E1] (+ coefficients ef1) and ei2 [2,E2].  Returns a dict:
    l_ptr0, l_ptr1, inds0, inds1 (the lists as the arena holds them after the count step), vcount, cursor, v_ptr, v_pos, v_oth,
    v_coef, flags, and: `alt` {name: {entry: set of values}} for by-left offsets several positions write (a list out of order),
    `zeroed` (variables whose segment was zero-filled), `path` (per variable: "zero", "lds" or "global")."""
    D = ACTIVE if D is None else frozenset(D)
    E1, E2 = np.shape(ei1)[1], np.shape(ei2)[1]
    L = launch_single(C, V, K, E1, E2)
    inds = [Arr("inds0", data=np.asarray(ei1, np.int64).reshape(-1)), Arr("inds1", data=np.asarray(ei2, np.int64).reshape(-1))]
    coef = Arr("cons_coef", data=np.asarray(ef1, f32).reshape(-1), dtype=f32)
    l_ptr = [Arr("l_ptr0", C + 1, 0), Arr("l_ptr1", K + 1, 0)]         # the zero block travels zeroed with the upload
    vcount, cursor, flags = Arr("vcount", V, 0), Arr("cursor", V, 0), Arr("flags", 4, 0)
    alt = {f"l_ptr{s}": _count(s, inds[s], E, n_left, V, l_ptr[s], vcount, flags, D) for s, (E, n_left) in enumerate(((E1, C), (E2, K)))}
    # place: every block scans the counts, block 0 keeps v_ptr; each edge takes the next slot of its variable's segment
    pre = scan(vcount, V, L["place_nt"], D)
    v_ptr = Arr("v_ptr", V + 1)
    v_ptr[np.arange(V + 1)] = pre[np.arange(V + 1)]
    v_pos, v_oth = Arr("v_pos", E1), Arr("v_oth", E1)
    v_coef = Arr("v_coef", E1, fill=np.array([POISON], i32).view(f32)[0], dtype=f32)
    placed = min(E1, L["place_blocks"] * L["place_nt"]) if "place_one_trip" in D else E1
    var = inds[0][E1 + np.arange(placed)]                             # sanitised by the count step
    by_var = np.argsort(var, kind="stable")                            # arrival order taken as input order: only the set is defined
    starts = np.searchsorted(var[by_var], var[by_var])
    v_pos[pre[var[by_var]] + cursor[var[by_var]] + np.arange(placed) - starts] = by_var
    cursor.add(var)
    # order: the rank of an input position inside its segment is its place in the stable order
    n_order = min(V, L["order_blocks"] * L["order_groups"]) if "order_one_trip" in D else V
    oth_hi = max(C - 1, 0)
    zeroed, path = [], ["none"] * V
    for v in range(n_order):
        beg = int(v_ptr[v])
        n = int(v_ptr[v + 1]) - beg
        if n <= 0:
            path[v] = "lds"
            continue
        idx = beg + np.arange(n)
        if (n >= MAX_DEG) if "maxdeg_ge" in D else (n > MAX_DEG):
            flags[3] |= 1
            v_oth[idx], v_coef[idx] = 0, 0.0
            zeroed.append(v)
            path[v] = "zero"
            continue
        x = v_pos[idx]
        if (n < LDS_DEG) if "lds_lt" in D else (n <= LDS_DEG):
            path[v] = "lds"
            seg = np.concatenate([x, np.full(((n + 3) & ~3) - n, 0 if "pad_zero" in D else INT_MAX, np.int64)])
        else:
            path[v] = "global"
            seg = x
        rank = (seg[None, :] < x[:, None]).sum(1)
        left = inds[0][x]
        v_oth[beg + rank] = left if "no_clamp_voth" in D else np.clip(left, 0, oth_hi)
        v_coef[beg + rank] = coef[x]
    out = dict(l_ptr0=l_ptr[0].a, l_ptr1=l_ptr[1].a, inds0=inds[0].a, inds1=inds[1].a, vcount=vcount.a, cursor=cursor.a, v_ptr=v_ptr.a,
               v_pos=v_pos.a, v_oth=v_oth.a, v_coef=v_coef.a, flags=flags.a)
    out = {k: (a if a.dtype == f32 else a.astype(i32)) for k, a in out.items()}
    out.update(alt=alt, zeroed=zeroed, path=path, launch=L)
    return out


def forward_gathers(p, C, V, K):
    """The row gathers the forward makes through the plan (forward_enqueue): an edge pass is launched for a non-empty receiver set
    only; each receiver walks its segment and gathers a row of the other side's table.  Raises OutOfBounds where an offset leaves
    the lists or an id leaves its table."""
    E1, E2 = p["inds0"].size // 2, p["inds1"].size // 2
    for name, ptr, oth, n_own, n_tab, E in (("conv v->c", p["l_ptr0"], p["inds0"][E1:], C, V, E1), ("conv c->v", p["v_ptr"], p["v_oth"], V, C, E1),
                                            ("conv v->k", p["l_ptr1"], p["inds1"][E2:], K, V, E2)):
        if n_own <= 0:
            continue
        lists, table = Arr(name + " edges", data=oth), Arr(name + " table rows", n_tab, 0)
        for r in range(n_own):
            b, e = int(ptr[r]), int(ptr[r + 1])
            if e > b:
                table[lists[np.arange(b, e)]]


# ---- the union plan ----------------------------------------------------------------------------------------------------------------
def union_table(keys, fshapes=None):
    """Offsets of every state in the union: columns C, V, K, E1, E2, F, FE, each with S + 1 entries (ibatch_sums)."""
    S = len(keys)
    cols = np.zeros((7, S + 1), np.int64)
    for s, k in enumerate(keys):
        f = fshapes[s] if fshapes else (0, 0)
        cols[:, s + 1] = cols[:, s] + np.array(list(k) + list(f))
    return cols


def _search(keys, item, S, D):
    """The kernel's binary search, for every item at once: the last state s with keys[s] <= item."""
    s, hi = np.zeros(item.size, np.int64), np.full(item.size, S, np.int64)
    while (hi - s > 1).any():
        go = hi - s > 1
        mid = (s + hi) >> 1
        down = (keys[mid] < item) if "ib_search_lt" in D else (keys[mid] <= item)
        s, hi = np.where(go & down, mid, s), np.where(go & ~down, mid, hi)
    return s


def plan_union(keys, packed1, packed2, fshapes=None, f_cols=None, D=None):
    """What k_ib_unpack and the by-variable stage leave in the arena.  keys: per state (C, V, K, E1, E2); packed1 / packed2: per
    state the packed [2,E] lists with their coefficients ((ei, ef)); fshapes / f_cols: per state (F, FE) and the forced columns.
    Returns left, var0, var1, iota, l_ptr0, l_ptr1, f_col, flags [S,4], v_ptr, v_oth, v_coef and `alt` as plan_single."""
    D = ACTIVE if D is None else frozenset(D)
    S = len(keys)
    tab = union_table(keys, fshapes)
    Ct, Vt, Kt, E1t, E2t, _, FEt = (int(x) for x in tab[:, S])
    none = [np.zeros(0, np.int64)]
    src = [Arr(f"packed{i}", data=np.concatenate([np.asarray(ei, np.int64).reshape(-1) for ei, _ in p] + none))
           for i, p in enumerate((packed1, packed2))]
    coef = np.concatenate([np.asarray(ef, f32).reshape(-1) for _, ef in packed1] + [np.zeros(0, f32)])
    f_in = Arr("f_col_in", data=np.concatenate([np.asarray(c, np.int64) for c in (f_cols or [])] + none))
    left, iota = Arr("left", E1t), Arr("iota", E1t)
    var = [Arr("var0", E1t), Arr("var1", E2t)]
    l_ptr = [Arr("l_ptr0", Ct + 1, 0), Arr("l_ptr1", Kt + 1, 0)]
    flags, f_col = Arr("flags", 4 * S, 0), Arr("f_col", FEt)
    alt = {}
    if FEt:                                            # the forced entries
        i = np.arange(FEt)
        s = _search(tab[6], i, S, D)
        c, nv = f_in[i], tab[1][s + 1] - tab[1][s]
        f_col[i] = np.where((c >= 0) & (c < nv), c + tab[1][s], -1)
    for st, (eoff, loff) in enumerate(((tab[3], tab[0]), (tab[4], tab[2]))):
        item = np.arange(int(eoff[S]) + S)             # per state its edges and one closing position
        s = _search(eoff + np.arange(S + 1), item, S, D)
        e0, E = eoff[s], eoff[s + 1] - eoff[s]
        j = item - e0 - s
        l0, n_left = loff[s], loff[s + 1] - loff[s]
        v0, nv = tab[1][s], tab[1][s + 1] - tab[1][s]
        writers = []
        if "ib_lptr0_from_data" not in D:
            _range_writes(l_ptr[st], l0[j == 0], l0[j == 0], e0[j == 0], writers)
        clamp = lambda x, hi: np.clip(x, -1, hi)  # noqa: E731 -- (beside the loop's own bounds below it changes nothing)
        lo, hb = np.full(item.size, -1), n_left.copy()
        lo[j > 0] = clamp(src[st][(2 * e0 + j - 1)[j > 0]], n_left[j > 0])
        hb[j != E] = clamp(src[st][(2 * e0 + j)[j != E]], n_left[j != E])
        first = 0 if ("ib_rows_from_0" in D or "ib_lptr0_from_data" in D) else 1
        _range_writes(l_ptr[st], l0 + np.maximum(lo + 1, first), l0 + np.minimum(hb, n_left - 1), e0 + j, writers)
        alt[f"l_ptr{st}"] = _contested(writers)
        m = j < E
        at, l, v = (e0 + j)[m], src[st][(2 * e0 + j)[m]], src[st][(2 * e0 + E + j)[m]]
        bad_l, bad_v = (l < 0) | (l >= n_left[m]), (v < 0) | (v >= nv[m])
        flags.a[4 * np.unique(s[m][bad_l | bad_v])] |= 1
        nxt = m & (j + 1 < E)
        unsorted = src[st][(2 * e0 + j + 1)[nxt]] < src[st][(2 * e0 + j)[nxt]]
        flags.a[4 * np.unique(s[nxt][unsorted]) + 1 + st] |= 1
        var[st][at] = v0[m] + (v if "ib_no_clamp_var" in D else np.where(bad_v, 0, v))
        if st == 0:
            left[at] = l0[m] + (l if "ib_no_clamp_left" in D else np.clip(l, 0, np.maximum(n_left[m] - 1, 0)))
            iota[at] = at
    l_ptr[0][Ct] = E1t
    l_ptr[1][Kt] = E2t
    out = dict(left=left.a, var0=var[0].a, var1=var[1].a, iota=iota.a, l_ptr0=l_ptr[0].a, l_ptr1=l_ptr[1].a, f_col=f_col.a, flags=flags.a)
    # by-variable stage (by_key_stage): a stable sort of (variable id, input position); an empty list leaves v_ptr zero
    if E1t:
        Arr("union variables", Vt, 0)[var[0].a]                         # a key outside [0, V) would leave the segment offsets
        perm = np.argsort(var[0].a, kind="stable")
        out.update(v_ptr=np.searchsorted(var[0].a[perm], np.arange(Vt + 1)), v_oth=left.a[Arr("left", data=left.a)._chk(iota.a[perm])],
                   v_coef=coef[iota.a[perm]])
    else:
        out.update(v_ptr=np.zeros(Vt + 1, np.int64), v_oth=np.zeros(0, np.int64), v_coef=np.zeros(0, f32))
    out = {k: (a if a.dtype == f32 else a.astype(i32)) for k, a in out.items()}
    out["flags"] = out["flags"].reshape(S, 4)
    out["alt"] = alt
    out["items"] = E1t + E2t + 2 * S + FEt
    return out


def union_gathers(p, keys):
    """forward_gathers for the union: the union's totals."""
    t = union_table(keys)[:, -1]
    q = dict(l_ptr0=p["l_ptr0"], l_ptr1=p["l_ptr1"], v_ptr=p["v_ptr"], v_oth=p["v_oth"], inds0=np.concatenate([p["left"], p["var0"]]),
             inds1=np.concatenate([np.zeros_like(p["var1"]), p["var1"]]))
    forward_gathers(q, int(t[0]), int(t[1]), int(t[2]))


# ---- fill ------------------------------------------------------------------------------------------------------------------------------
def distinct_coefs(rng, E):
    """E distinct fp32 values in (-1, 1), in random order: a misplaced or swapped edge shows in the copied coefficients."""
    return (((rng.permutation(E) + 1.0) / (E + 1.0)) * 2.0 - 1.0).astype(f32).reshape(-1, 1)


def sorted_rows(rng, E, n_rows, lo=0, hi=None):
    """E row ids in [lo, hi), sorted."""
    hi = n_rows if hi is None else hi
    return np.sort(rng.integers(lo, hi, E)) if E else np.zeros(0, np.int64)


def cols_of_degrees(rng, degs):
    """Variable ids with these degrees, shuffled."""
    return rng.permutation(np.repeat(np.arange(len(degs)), degs))


def state(seed, C, V, K, rows1, cols1, rows2, cols2):
    """The model's 10-tuple: standard normal features, distinct coefficients per list."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(f32)  # noqa: E731
    ei1, ei2 = np.stack([rows1, cols1]).astype(i32).reshape(2, -1), np.stack([rows2, cols2]).astype(i32).reshape(2, -1)
    return (f(C, 4), ei1, distinct_coefs(rng, ei1.shape[1]), f(V, 14), f(K, 6), ei2, distinct_coefs(rng, ei2.shape[1]), C, V, K)


def random_state(seed, C, V, K, E1, E2):
    rng = np.random.default_rng(seed + 1000)
    return state(seed, C, V, K, sorted_rows(rng, E1, C), rng.integers(0, max(V, 1), E1), sorted_rows(rng, E2, K), rng.integers(0, max(V, 1), E2))


def other_contents(st, seed=99):
    """A state of the same sizes and other contents (what the arena is made to hold before it is poisoned)."""
    C, V, K = st[7:]
    return random_state(seed, C, V, K, np.shape(st[1])[1], np.shape(st[5])[1])


def packed_lists(st):
    ei1, ef1 = pack(st[1], st[2], st[7])
    ei2, ef2 = pack(st[5], st[6], st[9])
    return ei1, ef1, ei2, ef2


def expected_single(st, D=None):
    ei1, ef1, ei2, _ = packed_lists(st)
    return plan_single(st[7], st[8], st[9], ei1, ef1, ei2, D)


@functools.lru_cache(maxsize=None)
def expected_case(cid):
    """The restated plan of a case (single or union), computed once."""
    if cid in SINGLE:
        return expected_single(single(cid))
    states, forced = union(cid)
    return expected_union(states, packed_forced(states, forced))


def packed_forced(states, forced):
    """Per state the host CSR (ptr, col, val) of its forced rows, entries of a row in input order (ops.pack_rows)."""
    if forced is None:
        return None
    out = []
    for st, (fi, fv, F) in zip(states, forced):
        p = np.argsort(fi[0], kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(fi[0], minlength=F))]).astype(i32)
        out.append((ptr, fi[1][p].astype(i32), np.asarray(fv, f32)[p]))
    return out


def expected_union(states, forced=None, D=None):
    """forced: None or per state the packed (ptr, col, val)."""
    keys = [(s[7], s[8], s[9], np.shape(s[1])[1], np.shape(s[5])[1]) for s in states]
    lists = [packed_lists(s) for s in states]
    fshapes = [(len(f[0]) - 1, len(f[1])) for f in forced] if forced else None
    return plan_union(keys, [(l[0], l[1]) for l in lists], [(l[2], l[3]) for l in lists], fshapes, [f[1] for f in forced] if forced else None, D)


# ---- cases: the single-state plan -------------------------------------------------------------------------------------------------
# Every builder returns the state; `claims(id)` (below) says what it puts on which seam, and tests/test_plancases.py proves it.
SEAM_DEGS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 258, 1023, 2047, 2048)
BIG_C = FUSE_MAX_ROWS + 1            # 16,385 constraints: k_iplan_place, and eight waves in both row launches


def _with_degrees(seed, C, degs, K=3, E2=7):
    rng = np.random.default_rng(seed)
    cols = cols_of_degrees(rng, degs)
    V = len(degs)
    return state(seed, C, V, K, sorted_rows(rng, cols.size, C), cols, sorted_rows(rng, E2, K), rng.integers(0, V, E2))


def _degs_tail(V, degs, at):
    """V variables of degree 1, 0 or 2 in turn, the seam degrees `degs` from variable `at` on."""
    d = np.array([(1, 0, 2)[i % 3] for i in range(V)])
    d[at:at + len(degs)] = degs
    return d


def _rows_case(kind):
    rng = np.random.default_rng(31)
    C, V, K = 300, 40, 6
    if kind == "first_empty":
        rows1, rows2 = sorted_rows(rng, 500, C, 7), sorted_rows(rng, 9, K, 2)
    elif kind == "last_empty":
        rows1, rows2 = sorted_rows(rng, 500, C, 0, C - 9), sorted_rows(rng, 9, K, 0, K - 3)
    elif kind == "run_at_block":                      # rows 100..104 empty; the position that fills them is 256, then 8,192 (below)
        rows1 = np.concatenate([sorted_rows(rng, 256, C, 0, 100), sorted_rows(rng, 244, C, 105)])
        rows2 = sorted_rows(rng, 9, K)
    elif kind == "run_at_trip":
        C = 700
        rows1 = np.concatenate([sorted_rows(rng, 8192, C, 0, 300), sorted_rows(rng, 300, C, 304)])
        rows2 = sorted_rows(rng, 9, K)
    elif kind == "one_row":
        rows1, rows2 = np.full(500, 123), np.full(9, 4)
    elif kind == "C1":
        C, rows1, rows2 = 1, np.zeros(30, np.int64), sorted_rows(rng, 9, K)
    else:                                             # K1
        K, rows1, rows2 = 1, sorted_rows(rng, 500, C), np.zeros(9, np.int64)
    return state(32, C, V, K, rows1, rng.integers(0, V, rows1.size), rows2, rng.integers(0, V, rows2.size))


def _scan_special(kind):
    V, C = 1000, 200                                  # fused place: per = ceil(1000 / 256) = 4
    rng = np.random.default_rng(41)
    d = rng.integers(1, 4, V)
    if kind == "empty_start":
        d[:9] = 0
    elif kind == "empty_end":
        d[-9:] = 0
    elif kind == "empty_chunks":                      # empty variables across the ends of thread chunks and of a wave's chunks
        for t in (1, 63, 64, 200):
            d[4 * t - 2:4 * t + 2] = 0
    else:                                             # one_var
        d[:] = 0
        d[517] = 1500
    return _with_degrees(42, C, d)


def _twins(K):
    """Pairs of identical cuts (features, support, coefficients) at the seams of the ranking network."""
    rng = np.random.default_rng(50 + K)
    C, V = 40, 30
    pairs = [(a, b) for a, b in ((0, K - 1), (255, 256), (1023, 1024), (4094, 4095)) if a < b < K]
    st = state(51, C, V, K, sorted_rows(rng, 90, C), rng.integers(0, V, 90), np.repeat(np.arange(K), 2), rng.integers(0, V, 2 * K))
    k, ei, ef = st[4].copy(), st[5].copy(), st[6].copy()
    done = set()
    for a, b in pairs:
        if b in done:                                 # (0, K - 1) and (K - 2, K - 1) share a cut: three of a kind
            a, b = b, a
        k[b] = k[a]
        ei[1, 2 * b:2 * b + 2] = ei[1, 2 * a:2 * a + 2]
        ef[2 * b:2 * b + 2] = ef[2 * a:2 * a + 2]
        done.update((a, b))
    return st[:4] + (k, ei, ef) + st[7:], pairs


BAD_C, BAD_V, BAD_K, BAD_E1, BAD_E2 = 50, 30, 20, 700, 600


def _bad(which, value, where):
    """One id out of range in one of the four lists of a 700 / 600 edge state: negative or equal to the size; at the first edge,
    the last edge or the last position of block 0 (255)."""
    st = list(random_state(60, BAD_C, BAD_V, BAD_K, BAD_E1, BAD_E2))
    lst, row = {"cons_row": (1, 0), "cons_var": (1, 1), "cut_row": (5, 0), "cut_var": (5, 1)}[which]
    size = {"cons_row": BAD_C, "cons_var": BAD_V, "cut_row": BAD_K, "cut_var": BAD_V}[which]
    ei = st[lst].copy()
    ei[row, {"first": 0, "last": ei.shape[1] - 1, "block_end": 255}[where]] = -3 if value == "neg" else size
    st[lst] = ei
    return tuple(st)


def _single_cases():
    c = {}
    for E1 in (0, 1, 254, 255, 256, 257, 8190, 8191, 8192, 8193):
        c[f"count/E1/{E1}"] = functools.partial(random_state, 10, 37, 29, 3, E1, 5)
    for E1 in (510, 511, 512, 513, 16382, 16383, 16384, 16385):
        c[f"count/E1/512/{E1}"] = functools.partial(random_state, 11, BIG_C, 64, 3, E1, 5)
    for E2 in (0, 1, 2046, 2047, 2048, 2049):
        c[f"count/E2/{E2}"] = functools.partial(random_state, 12, 37, 29, 7, 40, E2)
    for kind in ("first_empty", "last_empty", "run_at_block", "run_at_trip", "one_row", "C1", "K1"):
        c[f"rows/{kind}"] = functools.partial(_rows_case, kind)
    for V in (1, 2, 255, 256, 257, 511, 512, 513, 4095, 4096):
        c[f"scan/256/V{V}"] = functools.partial(random_state, 13, 90, V, 4, 3 * V + 5, 9)
    for kind in ("empty_start", "empty_end", "empty_chunks", "one_var"):
        c[f"scan/256/{kind}"] = functools.partial(_scan_special, kind)
    for V in (1, 1023, 1024, 1025, 2047, 2048, 2049, 4096):
        c[f"scan/1024/V{V}"] = functools.partial(random_state, 14, BIG_C, V, 4, 2 * V + 5, 9)
    for V in (4097, 32767, 32768):
        c[f"scan/1024/big/V{V}"] = functools.partial(random_state, 15, 500, V, 4, 40000, 9)
    for E1 in (65536, 65537):
        c[f"place/trip/fused/{E1}"] = functools.partial(random_state, 16, 900, 700, 4, E1, 9)
        c[f"place/trip/alone/{E1}"] = functools.partial(random_state, 17, 900, 4097, 4, E1, 9)
    c["deg"] = functools.partial(_with_degrees, 18, 2100, np.array(SEAM_DEGS))
    c["deg/2049"] = functools.partial(_with_degrees, 19, 2100, np.array(SEAM_DEGS + (2049,)))
    seam = (0, 3, 4, 5, 16, 17, 255, 256, 257)
    for V, C in ((16, 60), (17, 60), (768, 60), (769, 60), (32, BIG_C), (33, BIG_C), (1536, BIG_C), (1537, BIG_C)):
        c[f"order/trip/V{V}"] = functools.partial(_with_degrees, 20, C, _degs_tail(V, (), 0))
    c["order/trip/degs/4w"] = functools.partial(_with_degrees, 21, 60, _degs_tail(768 + 40, seam, 768 + 3))
    c["order/trip/degs/8w"] = functools.partial(_with_degrees, 22, BIG_C, _degs_tail(1536 + 40, seam, 1536 + 3))
    c["order/2048"] = functools.partial(_with_degrees, 23, 300, _degs_tail(MAX_VARS, seam, MAX_VARS - 16 + 2))
    for K in (1, 2, 257, 1025, 4096):
        c[f"twins/K{K}"] = functools.partial(lambda K: _twins(K)[0], K)
    for which in ("cons_row", "cons_var", "cut_row", "cut_var"):
        for value in ("neg", "size"):
            for where in ("first", "last", "block_end"):
                c[f"bad/{which}/{value}/{where}"] = functools.partial(_bad, which, value, where)
    return c


SINGLE = _single_cases()
SINGLE_IDS = tuple(SINGLE)


@functools.lru_cache(maxsize=None)
def single(cid):
    return SINGLE[cid]()


def twin_pairs(cid):
    return _twins(int(cid.rsplit("K", 1)[1]))[1]


# states gcnn_infer has no row to park an id on: (C, V, K, E1, E2)
DEGENERATE = {"V0_E1": (5, 0, 3, 6, 0), "C0_E1": (0, 5, 3, 6, 0), "K0_E2": (5, 4, 0, 6, 4), "V0_E2": (5, 0, 3, 0, 4)}


def degenerate(name):
    C, V, K, E1, E2 = DEGENERATE[name]
    rng = np.random.default_rng(70)
    z = lambda E: np.zeros(E, np.int64)  # noqa: E731
    rows1 = sorted_rows(rng, E1, C) if C else z(E1)
    rows2 = sorted_rows(rng, E2, K) if K else z(E2)
    return state(71, C, V, K, rows1, rng.integers(0, V, E1) if V else z(E1), rows2, rng.integers(0, V, E2) if V else z(E2))


# ---- cases: the union plan ---------------------------------------------------------------------------------------------------------
def _small(seed, C=None, V=None, K=None, E1=None, E2=None):
    rng = np.random.default_rng(seed)
    pick = lambda x, lo, hi: int(rng.integers(lo, hi)) if x is None else x  # noqa: E731
    return random_state(seed, pick(C, 2, 14), pick(V, 2, 12), pick(K, 1, 6), pick(E1, 1, 40), pick(E2, 1, 16))


def forced_rows(rng, st, F, per_row=3):
    """F forced rows on random columns, as `GCNN.select_cuts_many` takes them."""
    rows = np.repeat(np.arange(F), per_row)
    vals = rng.standard_normal(rows.size)
    return np.stack([rows, rng.integers(0, st[8], rows.size)]).astype(i32), (vals / np.sqrt(per_row)).astype(f32), F


def union_bad_clean():
    """The states of ib/bad before one of them gets its bad ids: what the neighbours' entries are compared with."""
    return [_small(160), _small(161, C=9, V=7, K=4, E1=30, E2=12), _small(162)]


def _union_cases():
    u = {}
    for S in (1, 2, 3, 17, 64):
        u[f"ib/S{S}"] = functools.partial(lambda S: ([_small(100 + S + i) for i in range(S)], None), S)
    # no constraint edges | no cut edges | no constraint rows, each between regular states and beside each other
    u["ib/empty"] = lambda: ([_small(120), _small(121, E1=0), _small(122), _small(123, E2=0), _small(124, C=0, E1=0), _small(125, E1=0),
                              _small(126)], None)
    # state 0 owns items 0..255 (255 edges and its closing position), state 1 starts at item 256 = block 1, thread 0
    u["ib/seam"] = lambda: ([_small(130, E1=255, C=40, V=30), _small(131), _small(132)], None)
    for items in (262144, 262145):                    # E1 + E2 + 2 S + FE with S = 2
        u[f"ib/trip/{items}"] = functools.partial(
            lambda items: ([random_state(140, 5000, 3000, 50, 100000, 31000), random_state(141, 4000, 2500, 40, 100000, items - 231004)], None), items)

    def forced():
        rng = np.random.default_rng(150)
        states = [_small(150 + i, V=9) for i in range(6)]
        return states, [forced_rows(rng, s, F) for s, F in zip(states, (2, 0, 0, 3, 0, 1))]
    u["ib/forced"] = forced

    def bad():
        states = union_bad_clean()
        b = list(states[1])
        ei = b[1].copy()
        ei[0, 11], ei[1, 20] = -2, 7                  # a row id in the middle (the list travels unsorted) and a variable id
        b[1] = ei
        return [states[0], tuple(b), states[2]], None
    u["ib/bad"] = bad
    return u


UNION = _union_cases()
UNION_IDS = tuple(UNION)


@functools.lru_cache(maxsize=None)
def union(cid):
    return UNION[cid]()
