"""Edge lists and sample batches at the seams of the general path's graph plan and of the store's collation, and a restatement of
both (host only, NumPy only).

The graph plan: `gcnn_graph_check` (`k_check_edges`) and `gcnn_graph_build` (`k_iota`, a stable radix sort of (id, position),
`k_seg_offsets`, `k_gather_edges`), kernels in csrc/k_misc.hpp, launchers in csrc/gcnn_capi.hip.  The collation: `gcnn_collate`
(`k_collate`) behind `SampleStore.batch`.  Integer kernels: every comparison is exact, coefficients and features as their 32 bits.

THE RESTATEMENT -- index bookkeeping only, every function takes `defect`, one of DEFECTS:
  check_grid / build_grid / collate_grid   the launch formulas; their constants are read out of the two source files (`constants`)
  check_flags(left, var, n_left, n_var)    (bad, unsorted) as k_check_edges defines them, item by item over the grid's trips
  seg_offsets(keys, n_seg)                 k_seg_offsets: item i in [0, n] writes ptr[k] = i for k in (keys[i-1], keys[i]], ends -1 and
                                           n_seg; also the trip and the thread that writes each entry
  sort_bits(n_seg)                         the count of key bits the radix sort looks at
  csr(left, var, coef, n_left, n_var, left_sorted)   l_ptr, l_oth, l_coef, l_perm, v_ptr, v_oth, v_coef
  chunks(words)                            the eight (w0, w1) of a sample's segment of one array
  collate(samples, ids)                    the 16 arrays of a batch as int32 words, from a store of sample-local arrays
An entry that a defective restatement never writes holds PATTERN.  tests/test_batchcases.py requires each defect to change an exact
expected output on a named case.

CASES.  check_ids / check_case: a sorted, valid list per size with ONE planted entry (an id of -1 or n at a seam position of either
row, or a descent between two seam positions).  BUILD_IDS / build_case: small lists at every host-side detail (sort bits at a power
of two, runs of empty segments, ties with pairwise distinct coefficients, no edge), each left-sorted and not, and eight large ones
across the second grid trip of k_seg_offsets / k_gather_edges / k_iota.  pool / BATCHES: hand-built samples whose arrays have the
word counts at which k_collate's chunk split and copy loop change, and batches across its item loop's second trip."""
import functools
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcnn-cut-selector_amd", "csrc")
PATTERN = 0x5A5AA5A5          # what no kernel of this module writes: not an offset, an id, a small integer's or a normal draw's bits
DEFECTS = {
    "check": ("check_one_trip", "check_reads_past_end", "upper_le", "neg_ok", "var_unchecked", "ties_unsorted"),
    "build": ("build_one_trip", "no_closing", "no_leading", "gap_single", "bits_short", "unstable", "perm_from_var"),
    "collate": ("collate_one_trip", "inner_one_trip", "per_floor", "no_clamp", "add_prev", "ptr_tail_missing"),
}
CSR_FIELDS = ("l_ptr", "l_oth", "l_coef", "l_perm", "v_ptr", "v_oth", "v_coef")


def cdiv(a, b):
    return -(-a // b)


# ---- the constants are the source's ---------------------------------------------------------------------------------------------------
def _one(pattern, text, what):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, f"{what}: expected one form of /{pattern}/ in the source, found {sorted(found)}"
    (m,) = found
    return tuple(int(x) for x in m) if isinstance(m, tuple) else int(m)


@functools.lru_cache(maxsize=None)
def constants():
    """The launch constants, cut out of gcnn_capi.hip and k_misc.hpp: a changed constant moves the cases (or fails here)."""
    misc = open(os.path.join(CSRC, "k_misc.hpp")).read()
    capi = open(os.path.join(CSRC, "gcnn_capi.hip")).read()
    c = {}
    c["check_per"], c["check_max"], c["check_threads"] = _one(
        r"k_check_edges, dim3\(std::min\(cdiv\(n_edges, (\d+)\), (\d+)\)\), dim3\((\d+)\)", capi, "check launch")
    c["build_per"], c["build_max"] = _one(r"const int grid = std::min\(cdiv\(n_edges \+ 1, (\d+)\), (\d+)\);", capi, "build grid")
    c["build_threads"] = _one(r"hipLaunchKernelGGL\(k_(?:iota|seg_offsets|gather_edges), dim3\(grid\), dim3\((\d+)\)", capi, "build block")
    c["chunks"] = _one(r"#define COLLATE_CHUNKS (\d+)", misc, "chunks")
    c["collate_max"] = _one(r"const int bx = std::min\(batch \* COLLATE_CHUNKS, (\d+)\);", capi, "collate grid")
    c["collate_threads"] = _one(r"k_collate, dim3\(bx, n_jobs\), dim3\((\d+)\)", capi, "collate block")
    c["collate_stride"] = _one(r"for \(int i = threadIdx\.x; i < n; i \+= (\d+)\) dst\[i\] = src\[i\] \+ add;", misc, "copy loop")
    c["max_jobs"] = _one(r"constexpr int COLLATE_MAX_JOBS = (\d+);", misc, "job limit")
    assert c["check_per"] == c["check_threads"] and c["build_per"] == c["build_threads"] and c["collate_stride"] == c["collate_threads"]
    return c


def check_grid(n_edges):
    c = constants()
    return min(cdiv(n_edges, c["check_per"]), c["check_max"])


def build_grid(n_edges):
    c = constants()
    return min(cdiv(n_edges + 1, c["build_per"]), c["build_max"])


def collate_grid(batch):
    c = constants()
    return min(batch * c["chunks"], c["collate_max"])


def check_seam():
    """Items of k_check_edges' first trip at a capped grid: item CHECK_SEAM is the first of the second."""
    c = constants()
    return c["check_max"] * c["check_threads"]


def build_seam():
    c = constants()
    return c["build_max"] * c["build_threads"]


def collate_seam():
    """Samples k_collate's grid serves in one trip of the item loop."""
    c = constants()
    return c["collate_max"] // c["chunks"]


def inner_seam():
    """Words of a sample's segment that one trip of the copy loop moves: one more and a chunk takes a second trip."""
    c = constants()
    return c["chunks"] * c["collate_stride"]


# ---- gcnn_graph_check ----------------------------------------------------------------------------------------------------------------
def check_flags(left, var, n_left, n_var, defect=None):
    """(bad, unsorted) of k_check_edges: ids in [0, n); only the left row is looked at for order, ties count as sorted."""
    left, var = np.asarray(left, np.int64), np.asarray(var, np.int64)
    n = left.size
    if n == 0:
        return 0, 0
    ei = np.concatenate([left, var])                           # the [2, E] list as the kernel reads it: row 1 follows row 0
    stride = check_grid(n) * constants()["check_threads"]
    i = np.arange(min(n, stride) if defect == "check_one_trip" else n)
    l, v = ei[i], ei[n + i]
    over = (lambda x, m: x > m) if defect == "upper_le" else (lambda x, m: x >= m)
    bad = over(l, n_left)
    if defect != "neg_ok":
        bad = bad | (l < 0)
    if defect != "var_unchecked":
        bad = bad | over(v, n_var)
        if defect != "neg_ok":
            bad = bad | (v < 0)
    guard = np.ones(i.size, bool) if defect == "check_reads_past_end" else i + 1 < n
    nxt = ei[i + 1]                                             # item n - 1 would read var[0]; the guard keeps it out
    descent = (nxt <= l) if defect == "ties_unsorted" else (nxt < l)
    return int(bad.any()), int((guard & descent).any())


# ---- gcnn_graph_build ----------------------------------------------------------------------------------------------------------------
def seg_offsets(keys, n_seg, defect=None):
    """(ptr, trip, thread): ptr[k] = first position whose key >= k, ptr[n_seg] = n, as k_seg_offsets' items write it; trip and
    global thread of the item that writes each entry (-1 where nobody does, and ptr holds PATTERN there)."""
    keys = np.asarray(keys, np.int64)
    n = keys.size
    stride = build_grid(n) * constants()["build_threads"]
    items = np.arange(n + 1)
    lo = np.concatenate([[-1], np.maximum(keys, -1)])
    hi = np.concatenate([np.minimum(keys, n_seg), [n_seg]])
    live = np.ones(n + 1, bool)
    if defect == "build_one_trip":
        live &= items < stride
    if defect == "no_closing":
        live[n] = False
    if defect == "no_leading":
        live[0] = False
    cnt = np.where(live, np.maximum(hi - lo, 0), 0)
    if defect == "gap_single":                                 # ptr[key] alone, not the run of empty segments in front of it
        lo, cnt = hi - 1, np.minimum(cnt, 1)
    item = np.repeat(items, cnt)
    k = np.repeat(lo + 1, cnt) + (np.arange(item.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    ptr = np.full(n_seg + 1, PATTERN, np.int32)
    trip, thread = np.full(n_seg + 1, -1, np.int64), np.full(n_seg + 1, -1, np.int64)
    ptr[k], trip[k], thread[k] = item, item // stride, item % stride
    return ptr, trip, thread


def sort_bits(n_seg, defect=None):
    bits = 1
    while (1 << bits) < n_seg + 1 and bits < 31:
        bits += 1
    return bits - 1 if defect == "bits_short" else bits


def _by_key(key, n_seg, defect):
    """(order, ptr) of one side: a stable order on the key's low sort_bits bits -- the plain stable order for ids in [0, n_seg)."""
    key = np.asarray(key, np.int32)
    low = key & np.int32((1 << sort_bits(n_seg, defect)) - 1)
    if defect == "unstable":
        order = np.lexsort((-np.arange(key.size), low))
    else:
        order = np.argsort(low, kind="stable")
    return order.astype(np.int32), seg_offsets(key[order], n_seg, defect)[0]


def csr(left, var, coef, n_left, n_var, left_sorted, defect=None):
    """(l_ptr, l_oth, l_coef, l_perm, v_ptr, v_oth, v_coef) of gcnn_graph_build.  left_sorted: the by-left order is the input's."""
    left, var = np.asarray(left, np.int32), np.asarray(var, np.int32)
    coef = np.asarray(coef, np.float32).reshape(-1)
    if left.size == 0:
        e = np.zeros(0, np.int32)
        return (np.zeros(n_left + 1, np.int32), e, coef[:0], e, np.zeros(n_var + 1, np.int32), e, coef[:0])
    v_order, v_ptr = _by_key(var, n_var, defect)
    if left_sorted:
        l_order, l_ptr = np.arange(left.size, dtype=np.int32), seg_offsets(left, n_left, defect)[0]
    else:
        l_order, l_ptr = _by_key(left, n_left, defect)
    l_perm = v_order if defect == "perm_from_var" else l_order
    return l_ptr, var[l_order], coef[l_order], l_perm, v_ptr, left[v_order], coef[v_order]


def max_degrees(plan):
    """(l_max_deg, v_max_deg): the longest segment of either order."""
    return tuple(int(np.diff(plan[i].astype(np.int64)).max()) if plan[i].size > 1 else 0 for i in (0, 4))


# ---- check cases -----------------------------------------------------------------------------------------------------------------------
CHECK_N_LEFT, CHECK_N_VAR = 1000, 777


def check_sizes():
    s = check_seam()
    return (1, 2, 255, 256, 257, s - 1, s, s + 1, 2 * s + 1)


def _check_positions(n):
    s = check_seam()
    return sorted({p for p in (0, 255, 256, s - 1, s, n - 1) if 0 <= p < n})


def _descents(n):
    s = check_seam()
    return sorted({p for p in (0, 255, s - 1, s, n - 2) if 0 <= p and p + 1 < n})


@functools.lru_cache(maxsize=None)
def check_base(n):
    """A valid list of n edges sorted by left id, left ids in [1, n_left) with the largest legal id last, var[0] = 0 below it (so the
    word after the left row is smaller than the left row's last), and the largest legal variable id present."""
    rng = np.random.default_rng(n)
    left = np.sort(rng.integers(1, CHECK_N_LEFT, n)).astype(np.int32)
    left[-1] = CHECK_N_LEFT - 1
    var = rng.integers(0, CHECK_N_VAR, n).astype(np.int32)
    var[-1] = CHECK_N_VAR - 1
    var[0] = 0
    left.setflags(write=False)
    var.setflags(write=False)
    return left, var


def check_plants(n):
    """{kind: [(row, position, value)]} of every variant of size n: entries to overwrite in check_base(n), or a whole-row fill
    (position None)."""
    left, _ = check_base(n)
    out = {"ok": [], "ties": [(0, None, 5)], "max-only": [(0, None, CHECK_N_LEFT - 1), (1, None, CHECK_N_VAR - 1)]}
    for p in _check_positions(n):
        for row, name, limit in ((0, "left", CHECK_N_LEFT), (1, "var", CHECK_N_VAR)):
            out[f"{name}=-1@{p}"] = [(row, p, -1)]
            out[f"{name}=n@{p}"] = [(row, p, limit)]
    for p in _descents(n):
        out[f"descent@{p}"] = [(0, p + 1, int(left[p]) - 1)]  # left[p] >= 1; what follows is no smaller than it was: one descent
    return out


def check_ids():
    return [f"E{n}/{kind}" for n in check_sizes() for kind in check_plants(n)]


def check_case(cid):
    size, kind = cid.split("/", 1)
    n = int(size[1:])
    rows = [a.copy() for a in check_base(n)]
    for row, pos, value in check_plants(n)[kind]:
        if pos is None:
            rows[row][:] = value
        else:
            rows[row][pos] = value
    return dict(id=cid, left=rows[0], var=rows[1], n_left=CHECK_N_LEFT, n_var=CHECK_N_VAR)


# ---- build cases ------------------------------------------------------------------------------------------------------------------------
def distinct_coef(n, salt=0x2A5A5):
    """Pairwise distinct, exact in fp32: the order of ties shows."""
    return (np.arange(n, dtype=np.int64) ^ salt).astype(np.float32)


def _small(name):
    """(left, var, n_left, n_var) of a small case, in an order that is NOT sorted by left id (where it has two left ids)."""
    rng = np.random.default_rng(sum(name.encode()))
    kind, _, arg = name.partition("/")
    if kind == "E":
        n, nl, nv = int(arg), 37, 23
        return rng.integers(0, nl, n), rng.integers(0, nv, n), nl, nv
    if kind == "nseg":                                         # ids 0 and n_seg - 1 both present on both sides
        ns, n = int(arg), 41
        def ids():
            a = rng.integers(0, ns, n)
            a[[3, 17]] = ns - 1, 0
            return a
        return ids(), ids(), ns, ns
    big = 300001
    if name == "first-only":
        return np.zeros(6, int), np.zeros(6, int), big, big
    if name == "last-only":
        return np.full(6, big - 1), np.full(6, big - 1), big, big
    if name == "first-last":                                   # one item of k_seg_offsets writes a run of 300,000 entries
        return np.array([big - 1, 0, big - 1, 0, 0, big - 1]), np.array([0, big - 1, big - 1, 0, big - 1, 0]), big, big
    if name == "lead-trail":                                   # a leading and a trailing run of empty segments
        return rng.integers(400, 600, 700), rng.integers(300, 320, 700), 1000, 900
    if name == "one-seg":
        return np.full(300, 4), np.full(300, 2), 9, 5
    if name == "ties":
        return rng.integers(0, 3, 2000), rng.integers(0, 2, 2000), 3, 2
    if name == "E0":
        return np.zeros(0, int), np.zeros(0, int), 5, 7
    if name == "E0-void":
        return np.zeros(0, int), np.zeros(0, int), 0, 0
    raise KeyError(name)


SMALL = (["E/1", "E/255", "E/256", "E/257"] + [f"nseg/{n}" for n in (1, 2, 255, 256, 257, 65535, 65536, 65537)]
         + ["first-only", "last-only", "first-last", "lead-trail", "one-seg", "ties", "E0", "E0-void"])
N_MANY = 300000


def large_specs():
    """id -> (E, left segments, variable segments, left_sorted): four sizes around the second trip of the build's grid, 5 and about
    300,000 segments, sorted and not; the side that is not named has the other count."""
    s = build_seam()
    out = {}
    for n, many, srt in ((s - 1, False, True), (s - 1, True, False), (s, False, True), (s, True, False), (s + 1, False, False),
                         (s + 1, True, True), (2 * s + 1, True, True), (2 * s + 1, False, False)):
        out[f"L{n}/{'many' if many else 'seg5'}/{'sorted' if srt else 'unsorted'}"] = (n, many, srt)
    return out


def forced_changes(n):
    """Positions of the sorted keys at which a large case of n edges changes key, on both sides: the items around the grid's trips."""
    s = build_seam()
    got = [p for p in (s - 1, s, s + 1, 2 * s) if 0 < p < n]
    return got if got else [n - 2, n - 1]


def _sorted_keys(rng, n, many):
    """(sorted keys, n_seg): 5 segments, or N_MANY + 1 of which about two in three have an edge; a key change at every forced
    position."""
    cuts = set(forced_changes(n))
    if many:
        cuts |= set(rng.choice(np.arange(1, n), 200000, replace=False).tolist())
        n_seg = N_MANY + 1
    else:
        for p in (1000, 2000, 3000, 4000):
            if len(cuts) < 4:
                cuts.add(p)
        n_seg = 5
    bounds = np.array(sorted(cuts) + [n])
    runs = np.diff(np.concatenate([[0], bounds]))
    ids = np.sort(rng.choice(n_seg, runs.size, replace=False)) if many else np.arange(runs.size)
    return np.repeat(ids, runs).astype(np.int32), n_seg


@functools.lru_cache(maxsize=2)
def build_case(cid):
    """dict(id, left, var, coef, n_left, n_var, left_sorted).  left_sorted says what gcnn_graph_check must report."""
    if cid in large_specs():
        n, many, srt = large_specs()[cid]
        rng = np.random.default_rng(n + many)
        left, nl = _sorted_keys(rng, n, many)
        var, nv = _sorted_keys(rng, n, not many)
        var = var[rng.permutation(n)]
        if not srt:
            left = left[rng.permutation(n)]
        return dict(id=cid, left=left, var=var, coef=distinct_coef(n), n_left=nl, n_var=nv, left_sorted=srt)
    name, _, form = cid.rpartition("/")
    left, var, nl, nv = _small(name)
    left, var = np.asarray(left, np.int32), np.asarray(var, np.int32)
    if form == "sorted":
        order = np.argsort(left, kind="stable")
        left, var = left[order], var[order]
    srt = bool(np.all(np.diff(left) >= 0))
    assert form == "sorted" or not srt or np.unique(left).size < 2
    return dict(id=cid, left=left, var=var, coef=distinct_coef(left.size), n_left=nl, n_var=nv, left_sorted=srt)


def _forms(name):
    left = np.asarray(_small(name)[0])
    return ("sorted", "unsorted") if np.unique(left).size > 1 else ("sorted",)


SMALL_IDS = [f"{name}/{form}" for name in SMALL for form in _forms(name)]
LARGE_IDS = list(large_specs())
BUILD_IDS = SMALL_IDS + LARGE_IDS


def expected_csr(cid, left_sorted=None, defect=None):
    c = build_case(cid)
    return csr(c["left"], c["var"], c["coef"], c["n_left"], c["n_var"], c["left_sorted"] if left_sorted is None else left_sorted, defect)


# ---- collation -----------------------------------------------------------------------------------------------------------------------------
K_CONS, K_VAR, K_CUT, K_E1, K_E2 = range(5)
# name, unit kind (which offset table indexes it), words per unit, kind whose batch offset is added (-1: none), segment offsets?
JOBS = [("cons_feats", K_CONS, 4, -1, 0), ("var_feats", K_VAR, 14, -1, 0), ("cut_feats", K_CUT, 6, -1, 0), ("improvements", K_CUT, 1, -1, 0)]
for _slot, (_kl, _ke) in enumerate(((K_CONS, K_E1), (K_CUT, K_E2))):
    JOBS += [(f"{_slot}.l_ptr", _kl, 1, _ke, 1), (f"{_slot}.l_oth", _ke, 1, K_VAR, 0), (f"{_slot}.l_coef", _ke, 1, -1, 0),
             (f"{_slot}.v_ptr", K_VAR, 1, _ke, 1), (f"{_slot}.v_oth", _ke, 1, _kl, 0), (f"{_slot}.v_coef", _ke, 1, -1, 0)]
NAMES = [j[0] for j in JOBS]
SEAM_WORDS = (0, 1, 7, 8, 9, 15, 16, 17)


def large_words():
    w = inner_seam()
    return (w - 8, w - 1, w, w + 1, w + 8, w + 9, 2 * w + 1)


def chunks(words, defect=None):
    """The (w0, w1) of the chunks of a segment of `words` words."""
    n = constants()["chunks"]
    per = words // n if defect == "per_floor" else cdiv(words, n)
    if defect == "no_clamp":
        return [(c * per, c * per + per) for c in range(n)]
    return [(min(words, c * per), min(words, min(words, c * per) + per)) for c in range(n)]


def _specs():
    """(n_cons, n_vars, n_cuts, cons edges, cut edges) of every sample of the pool: 40 tiny ones, then the large."""
    W = SEAM_WORDS
    tiny = [(0, 0, 0, 0, 0),                                   # 0: nothing at all
            (5, 6, 0, 9, 0), (4, 5, 3, 0, 0), (3, 4, 0, 0, 0),  # 1 .. 3: no cut, no edge, neither
            (1, 1, 1, 1, 1), (2, 9, 2, 8, 16), (4, 17, 4, 16, 8), (0, 7, 5, 0, 17)]
    for rot in (1, 2, 3, 5):
        for i, w in enumerate(W):
            nc, nv, nk = w, max(W[(i + rot) % 8], 3), W[(i + 2 * rot + 1) % 8]
            tiny.append((nc, nv, nk, min(W[(i + 3 * rot) % 8], nc * nv), min(W[(i + rot + 4) % 8], nk * nv)))
    a, b, c, d, e, f, g = large_words()
    large = [(a // 4, 147, a // 6, a, b), (c // 4, 150, 342, b, c), (e // 4, d, 343, c, d), (d, 160, b, d, e), (a, 170, c, e, f),
             (300, e, f, f, g), (g, 146, 100, g, a), (100, g, e, d, d)]
    return tiny, large


def _sample(spec, seed, shuffle=False):
    nc, nv, nk, e1, e2 = spec
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)

    def edges(nl, e):
        flat = np.sort(rng.choice(nl * nv, e, replace=False)) if e else np.zeros(0, np.int64)
        if shuffle:
            flat = rng.permutation(flat)
        ei = np.stack([flat // max(nv, 1), flat % max(nv, 1)]).astype(np.int32)
        return {"indices": ei, "values": f(e, 1)}

    state = ({"values": f(nc, 4)}, edges(nc, e1), {"values": f(nv, 14)}, {"values": f(nk, 6)}, edges(nk, e2))
    return state, rng.uniform(0.0, 0.2, nk)


@functools.lru_cache(maxsize=None)
def pool():
    """The samples, (state, improvements) pairs as `utils.load_sample` returns them; sample 12's edge lists are not sorted."""
    tiny, large = _specs()
    return tuple(_sample(s, 100 + i, shuffle=(i == 12)) for i, s in enumerate(tiny + large))


def n_tiny():
    return len(_specs()[0])


def sample_sizes(sample):
    s = sample[0]
    return (s[0]["values"].shape[0], s[2]["values"].shape[0], s[3]["values"].shape[0], s[1]["indices"].shape[1], s[4]["indices"].shape[1])


def words_of(sample):
    """{array name: words of this sample's segment}."""
    size = sample_sizes(sample)
    return {name: size[kind] * width for name, kind, width, _, _ in JOBS}


def _words(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32)


@functools.lru_cache(maxsize=None)
def store():
    """(arrays, sizes[5, n], offsets[5, n + 1]): every array of the pool as the store keeps it -- int32 words, sample-local values,
    both orders of both edge sets per sample, segment offsets without their closing entry."""
    parts = {name: [] for name in NAMES}
    sizes = []
    for sample in pool():
        (cons, cons_edge, var, cut, cut_edge), imp = sample
        size = sample_sizes(sample)
        sizes.append(size)
        parts["cons_feats"].append(_words(cons["values"]))
        parts["var_feats"].append(_words(var["values"]))
        parts["cut_feats"].append(_words(cut["values"]))
        parts["improvements"].append(_words(np.asarray(imp).astype(np.float32)))
        for slot, (edge, nl) in enumerate(((cons_edge, size[0]), (cut_edge, size[2]))):
            ei = edge["indices"]
            plan = dict(zip(CSR_FIELDS, csr(ei[0], ei[1], edge["values"], nl, size[1], False)))
            for f in ("l_ptr", "v_ptr"):
                parts[f"{slot}.{f}"].append(plan[f][:-1])
            for f in ("l_oth", "v_oth"):
                parts[f"{slot}.{f}"].append(plan[f])
            for f in ("l_coef", "v_coef"):
                parts[f"{slot}.{f}"].append(_words(plan[f]))
    arrays = {name: np.concatenate(p).astype(np.int32) for name, p in parts.items()}
    sizes = np.asarray(sizes, np.int64).T.copy()
    offsets = np.concatenate([np.zeros((5, 1), np.int64), np.cumsum(sizes, axis=1)], axis=1)
    return arrays, sizes, offsets


def tables(ids):
    """(src_off[5, B], dst_off[5, B + 1]) of a batch: where each chosen sample starts in the store, and in the batch."""
    _, sizes, offsets = store()
    ids = np.asarray(ids, np.int64)
    dst = np.zeros((5, ids.size + 1), np.int64)
    np.cumsum(sizes[:, ids], axis=1, out=dst[:, 1:])
    return np.ascontiguousarray(offsets[:, ids]), dst


def collate(ids, defect=None, guard=0):
    """{name: int32 words} of the batch `ids` of the pool, as k_collate's items copy them: sample-local values shifted by the batch
    offsets, the closing entry of the four ptr arrays; `guard` words of PATTERN behind each array show a copy past its end."""
    arrays, _, _ = store()
    src_off, dst_off = tables(ids)
    batch, nch, stride = len(ids), constants()["chunks"], constants()["collate_stride"]
    grid = collate_grid(batch)
    out = {}
    for name, kind, width, add_kind, is_ptr in JOBS:
        src, so, dof = arrays[name], src_off[kind], dst_off[kind]
        aof = dst_off[add_kind] if add_kind >= 0 else None
        total = int(dof[batch]) * width + (1 if is_ptr else 0)
        dst = np.full(total + guard, PATTERN, np.int32)
        if is_ptr and defect != "ptr_tail_missing":
            dst[dof[batch]] = aof[batch]
        for item in range(min(batch * nch, grid) if defect == "collate_one_trip" else batch * nch):
            s, c = divmod(item, nch)
            w0, w1 = chunks(int(dof[s + 1] - dof[s]) * width, defect)[c]
            n = min(w1 - w0, stride) if defect == "inner_one_trip" else w1 - w0
            if n <= 0:
                continue
            add = 0 if aof is None else int(aof[max(s - 1, 0)] if defect == "add_prev" else aof[s])
            a, b = int(so[s]) * width + w0, int(dof[s]) * width + w0
            seg = src[a:a + n]
            seg = np.concatenate([seg, np.zeros(n - seg.size, np.int32)])     # (a defect's read past the store)
            m = max(0, min(n, dst.size - b))
            dst[b:b + m] = seg[:m] + np.int32(add)
        out[name] = dst
    return out


def _draw(seed, n):
    return np.random.default_rng(seed).integers(1, n_tiny(), n)


@functools.lru_cache(maxsize=None)
def batches():
    """id -> sample ids of the pool."""
    s, t = collate_seam(), n_tiny()
    out = {"b1": np.array([9])}
    for n in (s - 1, s, s + 1, 600):
        out[f"b{n}"] = _draw(n, n)
    out["void-ends"] = np.concatenate([[0], _draw(7, 30), [0]])
    out["every-tiny"] = np.arange(t)
    out["large"] = np.concatenate([[3], np.arange(t, len(pool())), [0, t + 2, 11]])
    return out


BATCH_IDS = ("b1", "b255", "b256", "b257", "b600", "void-ends", "every-tiny", "large")
