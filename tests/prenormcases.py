"""States at the places where the PreNorm fitting statistics (csrc/k_misc.hpp: k_stats, k_expand_ptr, k_stats_final / k_stats_fold;
plan in gcnn_capi.hip: prenorm_plan) change path: past the cap of ST_MAX_BLOCKS = 1,024 blocks, where a block's strided loop takes
a second trip, exactly on that cap, and at degenerate inputs (no edge, no cut, a constant column, a column far from zero).
Host only, NumPy only; tests/test_prenormcases.py checks that every case is what it claims and that a statistics pass with the
defect a case was built against leaves the bounds, tests/test_gpu_prenorm_edges.py runs the cases on the device.

A case is a dict: `state` (the model's 10-tuple; edge lists (row, col)-sorted without duplicates, so a list position is also its
by-left position), `layers` (the PreNorm layers, in call order, the case is checked on), `planted` and `lens` (below).

Planted outliers.  The bulk of every feature and coefficient is a standard normal value; at each seam position of each checked
layer one element is about 1e3 .. 1e4 of those standard deviations (OUTLIERS), so that a pass that loses it, or meets it twice,
moves mean and variance by many orders more than any bound here.  The seam positions of a source with n elements are the first
element of the second trip, the one before it, and the last (`seam_positions`).
  layers 0-4   (ST_COLS)  the row of the feature matrix / the list position of the coefficient
  layers 5,7,9 (ST_EDGE)  the coefficient at that list position
  layers 6,8,10 (ST_FLAT) the coefficient of an edge whose receiver is that row; where the row has no edge (its A row is zero,
                          and losing it changes no sum), the last row before it that has one
`planted[layer]` lists (position, index of the planted edge or None, column or None)."""
import functools
import math

import numpy as np

# ---- the constants of the plan (k_misc.hpp, prenorm_plan): named once, here ------------------------------------------------------
ST_MAX_BLOCKS = 1024      # blocks of a statistics launch, and of k_expand_ptr, at most
THREADS = 256             # threads per block: ST_COLS rows / ST_FLAT elements / k_expand_ptr segments per block and trip
EMB = 64
FLAT_ROWS = THREADS // EMB            # 4: rows of a [n, 64] matrix per block and trip
EDGE_LANES = 16                       # threads that share one edge (4 channels each)
BLOCK_EDGES = THREADS // EDGE_LANES   # 16: edges per block and trip
PER_BLOCK = {"cols": THREADS, "flat": FLAT_ROWS, "edge": BLOCK_EDGES, "expand": THREADS}
SEAM = {src: ST_MAX_BLOCKS * per for src, per in PER_BLOCK.items()}   # the first element of the second trip

# layer -> (source, the count it runs over); layers 5 / 7 / 9 also expand the by-left pointer of their list (C, C, K segments)
LAYER = {0: ("cols", "C"), 1: ("cols", "E1"), 2: ("cols", "V"), 3: ("cols", "K"), 4: ("cols", "E2"),
         5: ("edge", "E1"), 6: ("flat", "C"), 7: ("edge", "E1"), 8: ("flat", "V"), 9: ("edge", "E2"), 10: ("flat", "K")}
UNITS = (4, 1, 14, 6, 1, 1, 1, 1, 1, 1, 1)
OUTLIERS = (2000.0, -3000.0, 5000.0, -7000.0, 4000.0, -6000.0)

_f32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def grid(source, n, cap=ST_MAX_BLOCKS):
    """prenorm_plan's grid for a source over n rows (or edges)."""
    return max(1, min(cdiv(n, PER_BLOCK[source]), cap))


def seam_positions(source, n):
    """Last element; with a second trip also its first element and the one before; exactly on the cap, the last one only."""
    if n <= 0:
        return []
    s = SEAM[source]
    return sorted({n - 1} | ({s - 1, s} if n > s else set()))


def sizes(state):
    return dict(C=int(state[7]), V=int(state[8]), K=int(state[9]), E1=int(np.shape(state[1])[1]), E2=int(np.shape(state[5])[1]))


# ---- edge lists ----------------------------------------------------------------------------------------------------------------------
def _edges(rng, lens, n_cols, force=None):
    """A (row, col)-sorted [2, E] list with lens[r] distinct columns in row r; `force`: {row of length 1: its column}."""
    lens = np.asarray(lens, np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(lens.size), lens)
    j = np.arange(rows.size) - ptr[rows]
    stride = np.clip(np.minimum(rng.integers(1, 4, lens.size), n_cols // np.maximum(lens, 1)), 1, None)
    assert np.all(lens <= n_cols)
    cols = (rng.integers(0, n_cols, lens.size)[rows] + stride[rows] * j) % n_cols   # stride * len <= n_cols: distinct in a row
    for r, c in (force or {}).items():
        assert lens[r] == 1, r
        cols[ptr[r]] = c
    order = np.lexsort((cols, rows))
    return np.stack([rows[order], cols[order]]).astype(np.int32), ptr


def _lens(rng, n, total, fixed, spread):
    """n row lengths that sum to `total`: `fixed` {row: length} as given, `spread` of the other rows emptied at random, the rest 1
    or more."""
    lens = np.ones(n, np.int64)
    free = np.setdiff1d(np.arange(n), np.fromiter(fixed, np.int64, len(fixed)))
    lens[rng.choice(free, size=int(spread * free.size), replace=False)] = 0
    for r, m in fixed.items():
        lens[r] = m
    missing = total - int(lens.sum())
    assert missing >= 0, "fixed rows alone exceed the total"
    np.add.at(lens, rng.choice(free[lens[free] > 0], size=missing, replace=True), 1)      # (the emptied rows stay empty)
    assert int(lens.sum()) == total
    return lens


# ---- states -----------------------------------------------------------------------------------------------------------------------------
def _bulk(rng, shape):
    return rng.standard_normal(shape).astype(_f32)


def _build(seed, C, V, K, lens1, lens2, layers, force1=None, force2=None):
    rng = np.random.default_rng(seed)
    cei, ptr1 = _edges(rng, lens1, V, force1)
    kei, ptr2 = _edges(rng, lens2, V, force2)
    E1, E2 = cei.shape[1], kei.shape[1]
    feats = {0: _bulk(rng, (C, 4)), 2: _bulk(rng, (V, 14)), 3: _bulk(rng, (K, 6))}
    coef = {1: _bulk(rng, (E1, 1)), 4: _bulk(rng, (E2, 1))}
    n_of = dict(C=C, V=V, K=K, E1=E1, E2=E2)
    planted, used = {}, {1: {}, 4: {}}
    turn = [0]

    def value():
        turn[0] += 1
        return OUTLIERS[turn[0] % len(OUTLIERS)]

    def plant_edge(which, e):
        if e not in used[which]:
            used[which][e] = value()
            coef[which][e, 0] = used[which][e]
        return e

    for layer in layers:
        src, key = LAYER[layer]
        out = planted.setdefault(layer, [])
        for i, pos in enumerate(seam_positions(src, n_of[key])):
            if layer in feats:                      # a feature value, in a column that changes from position to position
                col = (pos + i) % feats[layer].shape[1]
                feats[layer][pos, col] = value()
                out.append((pos, None, col))
            elif src in ("cols", "edge"):           # the coefficient at that list position
                out.append((pos, plant_edge(1 if key == "E1" else 4, pos), None))
            else:                                   # an edge whose receiver is that row (or the last row before it that has one)
                which, ei, ptr = (4, kei, ptr2) if layer == 10 else (1, cei, ptr1)
                if layer == 8:                      # receiver = the variable: any edge of that column
                    hits = np.flatnonzero(ei[1] == pos)
                    while hits.size == 0:
                        pos -= 1
                        hits = np.flatnonzero(ei[1] == pos)
                    e = int(hits[0])
                else:
                    while ptr[pos + 1] == ptr[pos]:
                        pos -= 1
                    e = int(ptr[pos])
                out.append((pos, plant_edge(which, e), None))
    state = (feats[0], cei, coef[1], feats[2], feats[3], kei, coef[4], C, V, K)
    return dict(state=state, layers=tuple(layers), planted=planted, lens=(np.asarray(lens1), np.asarray(lens2)))


def _seam_small():
    """ST_FLAT at 4,097 / 4,095 / 4,096 receiver rows (layers 6, 8, 10: past the seam, below the cap, exactly on it) and ST_EDGE
    one edge past the seam and exactly on it (layers 5 and 7 on E1 = 16,385, layer 9 on E2 = 16,384).  The last constraint row is
    the first row of layer 6's second trip and holds a planted edge; the last cut row is empty, as are other rows of both lists,
    and constraint row 7 is a hub of 3,000 entries."""
    C, V, K, E1, E2 = 4097, 4095, 4096, 16385, 16384
    rng = np.random.default_rng(101)
    fixed1 = {0: 0, 100: 0, 2047: 0, 2048: 0, 4094: 0, 7: 3000, 4095: 1, 4096: 1, 300: 1}
    fixed2 = {0: 0, 4095: 0, 2000: 0, 4094: 2}
    lens1, lens2 = _lens(rng, C, E1, fixed1, 0.05), _lens(rng, K, E2, fixed2, 0.05)
    return _build(102, C, V, K, lens1, lens2, range(11), force1={300: V - 1})


def _seam_rows():
    """ST_COLS past the seam with f = 4, 1 and 14 (layers 0, 1, 2), k_expand_ptr's second trip over empty segments (layer 5: the
    constraint rows from 262,140 on are empty, the seam lies inside that run) and ST_FLAT with 64 trips (layers 6, 8)."""
    C, V, K, E1, E2 = 262145, 262146, 40, 262147, 120
    rng = np.random.default_rng(201)
    fixed1 = {r: 0 for r in list(range(262140, C)) + list(range(131000, 131012))}
    fixed1.update({SEAM["flat"] - 1: 1, SEAM["flat"]: 1, 50000: 1, 50001: 1, 50002: 1})
    lens1 = _lens(rng, C, E1, fixed1, 0.2)
    lens2 = _lens(rng, K, E2, {K - 1: 0}, 0.1)
    return _build(202, C, V, K, lens1, lens2, (0, 1, 2, 5, 6, 8),
                  force1={50000: SEAM["flat"] - 1, 50001: SEAM["flat"], 50002: V - 1})


def _seam_cuts():
    """ST_COLS past the seam with f = 6 and 1 (layers 3, 4), k_expand_ptr's second trip writing the left ids of the cut rows from
    262,144 on (layer 9), and layer 10 over 262,146 rows; a few hundred variables send to all of them."""
    C, V, K, E1, E2 = 300, 200, 262146, 1500, 262150
    rng = np.random.default_rng(301)
    fixed2 = {r: 0 for r in (1000, 1001, 1002, 1003, 262140, 262141, 262142)}
    fixed2.update({SEAM["flat"] - 1: 1, SEAM["flat"]: 1, SEAM["expand"] - 1: 1, SEAM["expand"]: 2, K - 1: 1})
    lens1 = _lens(rng, C, E1, {C - 1: 0}, 0.1)
    lens2 = _lens(rng, K, E2, fixed2, 0.001)
    return _build(302, C, V, K, lens1, lens2, (3, 4, 9, 10))


def _tiny(which):
    """one: one row of each kind and one edge in each list; no_cut_edges: E2 = 0; no_cuts: K = 0; no_cons_edges: E1 = 0 (layer 6
    then reads an all-zero A).  Nothing is planted: every position is a seam position."""
    rng = np.random.default_rng(400)
    C, V, K, E1, E2 = {"one": (1, 1, 1, 1, 1), "no_cut_edges": (3, 4, 2, 5, 0), "no_cuts": (3, 4, 0, 5, 0),
                       "no_cons_edges": (3, 4, 2, 0, 3)}[which]

    def lens(n, total):
        out = np.zeros(n, np.int64)
        np.add.at(out, np.arange(total) % max(n, 1), 1)
        return out[:n]
    cei, _ = _edges(rng, lens(C, E1), V)
    kei, _ = _edges(rng, lens(K, E2), V)
    state = (_bulk(rng, (C, 4)), cei, _bulk(rng, (E1, 1)), _bulk(rng, (V, 14)), _bulk(rng, (K, 6)), kei, _bulk(rng, (E2, 1)), C, V, K)
    return dict(state=state, layers=tuple(range(11)), planted={}, lens=None)


CONSTANT = _f32(0.3)
CONSTANT_COLS = {3: CONSTANT, 9: _f32(0.0)}     # variable-feature column -> its value in every row


def _constant():
    """V = 262,145 (ST_COLS takes a second trip) with variable-feature column 3 = float32(0.3) and column 9 = 0 in every row.  In
    exact arithmetic the mean is float64(float32(0.3)) and the variance 0.0, and the fp64 passes ARE exact in any order
    (`assert_constant_exact`): the device must return exactly these."""
    C, V, K, E1, E2 = 8, 262145, 4, 16, 8
    rng = np.random.default_rng(500)
    case = _build(501, C, V, K, _lens(rng, C, E1, {}, 0.0), _lens(rng, K, E2, {}, 0.0), ())
    for col, c in CONSTANT_COLS.items():
        case["state"][3][:, col] = c
    case["layers"] = (2,)
    return case


OFFSET, OFFSET_STEP = 1.0e4, 2.0 ** -6
OFFSET_COLS = {0: 1, 1: 0, 2: 5}      # layer -> the column that is OFFSET + a multiple of OFFSET_STEP, |multiple * step| < 1


def _offset():
    """One column of the constraint features, the constraint-edge coefficients and one column of the variable features are
    1e4 + k / 64 with |k| < 64: all exact in fp32, with a variance near 1/3 under a squared mean of 1e8.  E[x^2] - mean^2 in one
    pass, an uncentred second pass or fp32 accumulators lose it; the two centred fp64 passes do not.  n stays small (4,099 rows,
    6,001 edges) so that the derived bound, which grows with n, stays orders below what fp32 accumulators lose."""
    C, V, K, E1, E2 = 4099, 300, 40, 6001, 200
    rng = np.random.default_rng(600)
    case = _build(601, C, V, K, _lens(rng, C, E1, {}, 0.1), _lens(rng, K, E2, {}, 0.1), ())
    st = case["state"]
    for layer, col in OFFSET_COLS.items():
        x = st[{0: 0, 1: 2, 2: 3}[layer]]
        x[:, col] = (OFFSET + rng.integers(-63, 64, x.shape[0]) * OFFSET_STEP).astype(_f32)
    case["layers"] = tuple(OFFSET_COLS)
    return case


TINY = ("one", "no_cut_edges", "no_cuts", "no_cons_edges")
_MAKERS = {"seam-small": _seam_small, "seam-rows": _seam_rows, "seam-cuts": _seam_cuts, "constant": _constant, "offset": _offset}
_MAKERS.update({"tiny-" + t: functools.partial(_tiny, t) for t in TINY})
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once per process and shared: nobody writes into a case."""
    return _MAKERS[name]()


def other_features(state, seed):
    """The same dims and edge lists with other bulk values (a second loader of the same size): planted values stay."""
    rng = np.random.default_rng(seed)

    def redo(a):
        a = np.asarray(a)
        return np.where(np.abs(a) > 100, a, _bulk(rng, a.shape)).astype(_f32)
    return (redo(state[0]), state[1], redo(state[2]), redo(state[3]), redo(state[4]), state[5], redo(state[6])) + tuple(state[7:])


def raw_input(state, layer):
    """The [n, units] fp32 matrix a raw layer (0 .. 4) takes its statistics of."""
    x = np.asarray(state[{0: 0, 1: 2, 2: 3, 3: 4, 4: 6}[layer]], _f32)
    return x.reshape(x.shape[0], UNITS[layer])


# ---- the reference and the bounds ----------------------------------------------------------------------------------------------------
U64 = 2.0 ** -53


def exact_stats(col):
    """(mean, variance, mean |x|) of a vector of fp32 values: `math.fsum` gives each sum rounded once.  The deviations are taken
    from the fp64 mean in longdouble and squared there; their squares enter fsum rounded to fp64.  With m the fp64 mean and mu
    the true one, sum (x - m)^2 = sum (x - mu)^2 + n (m - mu)^2 and |m - mu| <= 2 u |mu|: the reference's variance is within a
    few u of the true one, relatively, plus 4 u^2 mu^2 -- both far inside `raw_bounds` (n + 3 >= 4 roundings there)."""
    x = np.asarray(col, np.float64).reshape(-1)
    n = x.size
    if n == 0:
        return 0.0, 0.0, 0.0
    mean = math.fsum(x.tolist()) / n
    d = x.astype(np.longdouble) - np.longdouble(mean)
    var = math.fsum((d * d).astype(np.float64).tolist()) / n
    return mean, var, math.fsum(np.abs(x).tolist()) / n


def raw_bounds(n, var, mean_abs):
    """(bound on |mean - exact mean|, bound on |variance - exact variance|) for two fp64 passes over n fp32 values in ANY order.

    Pass 1.  fp32 -> fp64 is exact.  A sum of n numbers by n - 1 fp64 additions in any order (per-thread chains, the tree inside
    a block, the chain over the blocks; an addition of 0 is exact) is S (1 + t) term by term with |t| <= gamma_(n-1) =
    (n-1) u / (1 - (n-1) u), u = 2^-53 [Higham, Accuracy and Stability, (4.4)], so |S^ - S| <= gamma_(n-1) sum|x|.  The division
    by n rounds once more: |m^ - mu| <= (gamma_(n-1) + u (1 + gamma_(n-1))) mean|x| <= 2 n u mean|x| =: bm, for every n >= 1
    with n u << 1 (the factor 2 covers the second-order terms and the reference's own rounding, u |mu|).

    Pass 2.  sum (x - m^)^2 = sum (x - mu)^2 + n (m^ - mu)^2 exactly, i.e. the quantity the device approximates is
    var + (m^ - mu)^2 <= var + bm^2.  Each term is fl(fl(x - m^)^2): two roundings of the difference (it enters squared) and
    one of the square, (1 + d)^3; the sum adds gamma_(n-1) and the division one more: all terms are non-negative, so the result
    is (var + (m^ - mu)^2) (1 + t), |t| <= gamma_(n+3).  Hence
        |v^ - var| <= gamma_(n+3) (var + bm^2) + bm^2 <= 2 (n + 3) u (var + bm^2) + bm^2."""
    bm = 2.0 * n * U64 * mean_abs
    return bm, 2.0 * (n + 3) * U64 * (var + bm * bm) + bm * bm


def conv_bounds(want_mean, want_var, gap_mean=0.0, gap_var=0.0):
    """Layers 5 .. 10 against the fp64 oracle: the project's rule for PreNorm statistics (rtol 1e-6, atol 1e-6 sd), or twice the
    distance of the oracle's own fp32 evaluation from fp64 where that is larger (the gradient tests' rule, tests/gradparity.py)."""
    return (max(1e-6 * abs(want_mean) + 1e-6 * math.sqrt(want_var), 2.0 * gap_mean), max(1e-6 * want_var, 2.0 * gap_var))


# ---- one block-strided pass with per-block partials, restated --------------------------------------------------------------------------
def items_of(source, x):
    """The elements of a source as [items, values a thread adds per item]: item i is met by thread i % 256 of block
    (i // 256) % blocks on trip i // (256 blocks).  ST_COLS: one column, an item per row.  ST_FLAT: an item per element.  ST_EDGE
    ([E, 64] joint pre-activations): an item per (edge, lane), four channels each."""
    x = np.asarray(x, np.float64)
    return x.reshape(-1, 4) if source == "edge" else x.reshape(-1, 1)


def strided_sum(items, blocks, centre=None, acc=np.float64, single_trip=False, final_rows=None, final=np.float64):
    """stats_body + k_stats_final for one unit: every thread adds its items in order (squared deviations from `centre` if given)
    into an accumulator of type `acc`, the block's 256 accumulators are added in a tree in fp64, and one thread adds the first
    `final_rows` (default: all) block partials in order in type `final`.  `single_trip`: the strided loop stops after one trip."""
    n, k = items.shape
    per = blocks * THREADS
    trips = max(1, cdiv(n, per))
    term = np.zeros((trips * per, k))
    term[:n] = items if centre is None else (items - centre) ** 2
    term = term.reshape(trips, blocks, THREADS, k)
    a = np.zeros((blocks, THREADS), acc)
    for t in range(1 if single_trip else trips):
        for j in range(k):
            a = (a.astype(np.float64) + term[t, :, :, j]).astype(acc)
    red = a.astype(np.float64)
    s = THREADS // 2
    while s > 0:
        red[:, :s] += red[:, s:2 * s]
        s //= 2
    total = final(0.0)
    for p in red[:final_rows, 0]:
        total = final(np.float64(total) + p)
    return float(total)


def strided_stats(source, x, n, count=None, no_centre=False, uncapped=False, **how):
    """(mean, variance) of one unit as gcnn_prenorm_stats computes them: grid from `grid(source, n)`, two passes.  `no_centre`:
    pass 2 adds v * v.  `uncapped`: the grid is not capped while the final kernel still adds ST_MAX_BLOCKS partial rows."""
    items = items_of(source, x)
    count = float(items.size if count is None else count)
    if count == 0:                       # gcnn_prenorm_stats: nothing to absorb, mean 0 and variance 0 without a launch
        return 0.0, 0.0
    blocks = grid(source, n, cap=1 << 30) if uncapped else grid(source, n)
    if uncapped:
        how["final_rows"] = ST_MAX_BLOCKS
    mean = strided_sum(items, blocks, **how) / count
    return mean, strided_sum(items, blocks, centre=0.0 if no_centre else mean, **how) / count


def assert_constant_exact(col, c):
    """Why == is the right assertion for a constant column.  c = k 2^e with an integer |k| < 2^24 (an fp32 value), so every
    partial sum of j <= n copies, in any order, is the integer j k times 2^e with |j k| < 2^24 n <= 2^53: exact in fp64.  The final
    n c / n is the correctly rounded quotient of two values whose true quotient is the fp64 number c: exactly c.  Pass 2 then adds
    (c - c)^2 = 0."""
    col = np.asarray(col)
    assert col.dtype == np.float32 and bool(np.all(col == c))
    m, e = math.frexp(float(c))
    k = m * 2.0 ** 24
    assert k == int(k) and abs(int(k)) * col.size <= 2 ** 53
    assert float(np.float64(c) * col.size) / col.size == float(c)
