"""Cut-selection cases at the places where k_sel_pairs / k_sel_filter (csrc/k_select.hpp) change path or sit on an edge:
  A  `chunk_case()`   pivots whose entries span more than one LDS chunk of SEL_CH = 8,192 columns (chunks start at the pivot's
                      smallest column, not at 0), hand-placed pivot / partner pairs inside random rows over all of V = 20,000;
  B  `grid_case()`    a union of 1,040 samples with more than 65,535 pivot rows: the second trip of the block-strided pivot loop;
  C  `tie_case(v)`    dyadic rows whose parallelisms and scores lie exactly ON p_max, p_max_ub and t.
Host only (NumPy + the restatement tests/cutsel_restate.py); tests/test_selcases.py checks that every case is what it claims and
that it tells a defective selection from a correct one, tests/test_gpu_select_edges.py runs them on the device.

A sample is a dict: `cut` / `forced` (lists of (cols, vals), columns local to the sample), `q` (float32 [K]) and `V`.  A case is
`stack(samples, p_max, p_max_ub)`: the edge lists of the union as the device calls take them, the three offset arrays, and the
samples.  `expected(case)` is computed once per case and shared: nobody writes into it."""
import numpy as np

import cutsel_restate as R

CH = 8192          # SEL_CH: columns per LDS chunk of the pivot row
GRID = 65535       # k_sel_pairs launches min(n_rows, GRID) blocks; block b takes the pivots b, b + GRID, ...
EPS = 2.0 ** -20

_f32 = np.float32


def _row(entries):
    """[(col, value), ...] -> (cols int64, vals float32), in the order given (duplicates stay duplicates)."""
    return (np.array([c for c, _ in entries], np.int64), np.array([v for _, v in entries], np.float32))


# ---- random rows in the manner of plant_rows (tests/test_gpu_select.py), over a pool of columns ------------------------------------
def random_rows(rng, K, pool, extras=True):
    """K rows as [(cols, vals)] with columns from `pool`: random unit rows, exact / scaled / sign-flipped copies, partial overlaps
    with P = 0.05 / 0.3 / 0.7 / 0.92, empty rows and split (duplicate) entries."""
    pool = np.asarray(pool, np.int64)
    out, bank = [], []
    for k in range(K):
        kind = int(rng.integers(0, 8)) if (extras and bank) else 0
        if kind in (1, 2):
            cols, vals = bank[rng.integers(0, len(bank))]
            vals = vals * _f32([1.0, -1.0, 2.0, -0.6][rng.integers(0, 4)])
        elif kind == 3 and pool.size >= 4:
            cols0, vals0 = bank[rng.integers(0, len(bank))]
            alpha = [0.05, 0.3, 0.7, 0.92][rng.integers(0, 4)]
            free = np.setdiff1d(pool, cols0)
            if free.size == 0:
                cols, vals = cols0, vals0
            else:
                extra = rng.choice(free, size=min(free.size, int(rng.integers(1, 6))), replace=False)
                ev = rng.standard_normal(extra.size)
                ev = ev / np.linalg.norm(ev) * np.sqrt(1 - alpha * alpha)
                cols = np.concatenate([cols0, extra])
                vals = np.concatenate([alpha * vals0.astype(np.float64), ev]).astype(np.float32)
        elif kind == 4:
            cols, vals = np.zeros(0, np.int64), np.zeros(0, np.float32)
        else:
            nnz = int(rng.integers(1, min(12, pool.size) + 1))
            cols = np.sort(rng.choice(pool, size=nnz, replace=False))
            v = rng.standard_normal(nnz)
            vals = (v / np.linalg.norm(v)).astype(np.float32)
        if cols.size:
            bank.append((cols, vals))
        if kind == 5 and cols.size:
            j = int(rng.integers(0, cols.size))
            half = _f32(vals[j] * _f32(0.5))
            cols = np.concatenate([cols, [cols[j]]])
            vals = np.concatenate([vals[:j], [half], vals[j + 1:], [_f32(vals[j] - half)]]).astype(np.float32)
        out.append((np.asarray(cols, np.int64), np.asarray(vals, np.float32)))
    return out


def random_forced(rng, F, pool, cut):
    """F forced rows: scaled copies of cut rows and random unit rows."""
    pool = np.asarray(pool, np.int64)
    full = [r for r in cut if r[0].size]
    out = []
    for _ in range(F):
        if full and rng.random() < 0.7:
            c, v = full[rng.integers(0, len(full))]
            v = v * _f32([1.0, 0.3, -0.7][rng.integers(0, 3)])
        else:
            n = int(rng.integers(1, min(8, pool.size) + 1))
            c = rng.choice(pool, size=n, replace=False)
            v = rng.standard_normal(n)
            v = (v / np.linalg.norm(v)).astype(np.float32)
        out.append((np.asarray(c, np.int64), np.asarray(v, np.float32)))
    return out


def random_sample(rng, K, V, F):
    cut = random_rows(rng, K, np.arange(V))
    return dict(cut=cut, forced=random_forced(rng, F, np.arange(V), cut), q=rng.uniform(0.0, 1.0, K).astype(np.float32), V=V)


# ---- samples -> the arrays of a device call, and their restatement -------------------------------------------------------------------
def _edges(rows, col_off=0, row_off=0):
    r = np.concatenate([np.full(c.size, i + row_off) for i, (c, _) in enumerate(rows)] + [np.zeros(0, np.int64)])
    c = np.concatenate([c + col_off for c, _ in rows] + [np.zeros(0, np.int64)])
    v = np.concatenate([v for _, v in rows] + [np.zeros(0, np.float32)])
    return r.astype(np.int32), c.astype(np.int32), v.astype(np.float32)


def stack(samples, p_max, p_max_ub, name=""):
    """The disjoint union of `samples` (cut rows, forced rows and variables each stacked in sample order)."""
    c_off = np.cumsum([0] + [len(s["cut"]) for s in samples]).astype(np.int32)
    f_off = np.cumsum([0] + [len(s["forced"]) for s in samples]).astype(np.int32)
    v_off = np.cumsum([0] + [s["V"] for s in samples]).astype(np.int64)
    cut = [_edges(s["cut"], v_off[i], c_off[i]) for i, s in enumerate(samples)]
    forced = [_edges(s["forced"], v_off[i], f_off[i]) for i, s in enumerate(samples)]
    rows, cols, vals = (np.concatenate([e[k] for e in cut]) for k in range(3))
    frows, fcols, fvals = (np.concatenate([e[k] for e in forced]) for k in range(3))
    return dict(name=name, samples=samples, rows=rows, cols=cols, vals=vals, forced_inds=np.stack([frows, fcols]).astype(np.int32),
                forced_vals=fvals, q=np.concatenate([s["q"] for s in samples]).astype(np.float32), K=int(c_off[-1]),
                F=int(f_off[-1]), V=int(v_off[-1]), max_cuts=int(np.diff(c_off).max()), p_max=p_max, p_max_ub=p_max_ub,
                c_off=c_off, f_off=f_off, v_off=v_off)


def dense(sample):
    """(cut rows, forced rows) of one sample as dense fp64 matrices."""
    K, F, V = len(sample["cut"]), len(sample["forced"]), sample["V"]
    return R.dense_rows(*_edges(sample["cut"]), K, V), R.dense_rows(*_edges(sample["forced"]), F, V)


def parallelisms(sample):
    """(|A A^T|, |B A^T|) in fp64: what `R.select(P=...)` takes."""
    A, B = dense(sample)
    return np.abs(A @ A.T), np.abs(B @ A.T)


def restate_sample(sample, p_max, p_max_ub, P=None):
    rec = {}
    order, n = R.select(sample["q"], None, None, p_max, p_max_ub, record=rec, P=P if P is not None else parallelisms(sample))
    return order, n, rec


def same(a, b):
    """Two results (order, n_kept, ...) agree."""
    return bool(np.array_equal(a[0], b[0]) and a[1] == b[1])


_EXPECTED = {}


def expected(case):
    """[(order, n_kept, record)] per sample: the restatement, computed once per case."""
    key = id(case)
    if key not in _EXPECTED:
        _EXPECTED[key] = (case, [restate_sample(s, case["p_max"], case["p_max_ub"]) for s in case["samples"]])
    return _EXPECTED[key][1]


def select_variant(q, P, p_max, p_max_ub, gt_max=np.greater, gt_ub=np.greater, lt=np.less, threshold=R.threshold):
    """The loop of `R.select` with its three comparisons and the form of t as parameters: with the defaults it IS `R.select`
    (tests/test_selcases.py asserts that); with `np.greater_equal`, `np.less_equal` or a float32 product it is the defective
    selection a tie case must tell from the correct one."""
    q = np.asarray(q, np.float32)
    K = q.size
    order = R.ranking(q)
    P_cc, P_fc = P
    Q = q[order]
    low = lt(Q, threshold(Q[0]))
    n = K

    def sweep(Pv, first):
        nonlocal order, n
        rm = np.zeros(K, bool)
        rm[first:n] = gt_max(Pv, p_max) & (low[first:n] | gt_ub(Pv, p_max_ub))
        order = np.concatenate([order[~rm], order[rm]])
        n -= int(rm.sum())

    for r in range(P_fc.shape[0]):
        sweep(P_fc[r, order[:n]], 0)
    i = 0
    while i < n - 1:
        sweep(P_cc[order[i], order[i + 1:n]], i + 1)
        i += 1
    return order.astype(np.int32), n


# ---- A: chunk seams ---------------------------------------------------------------------------------------------------------------
A_V, A_K, A_THR = 20000, 131, (0.3, 0.6)


def chunk_of(col, mn):
    return (col - mn) // CH


def _chunk_pairs(V):
    """The hand-placed pairs.  Each: the pivot (the LOWER cut index of the pair, or a forced row: the row the kernel scatters into
    LDS), its entries, and partners with the products they make per chunk of that pivot.  `removed`: the verdict when every chunk
    counts once.  Every partner's score is low (below t), so P > p_max alone removes it."""
    def pair(name, pivot, mn, pe, partners, n_chunks):
        entries = [(mn + o, v) for o, v in pe]
        for p in partners:
            p["entries"] = [(mn + o, v) for o, v in p.pop("at")]
        return dict(name=name, pivot=pivot, mn=mn, entries=entries, partners=partners, n_chunks=n_chunks)

    sum_pe = [(0, 1.0), (10, 1.0), (CH + 10, 1.0)]
    sum_at = [(10, 0.2), (CH + 10, 0.2)]
    can_pe = [(0, 1.0), (20, 1.0), (2 * CH + 20, 1.0)]
    can_at = [(20, 0.4), (2 * CH + 20, -0.4)]
    return [
        # span boundary: the widest pivot of one chunk, the narrowest of two; the partner meets the pivot in its last column only
        pair("span1", ("cut", 3), 101, [(0, 1.0), (CH - 1, 1.0)], [dict(idx=70, at=[(CH - 1, 0.8)], removed=True)], 1),
        pair("span2", ("cut", 5), 211, [(0, 1.0), (CH, 1.0)], [dict(idx=129, at=[(CH, 0.8)], removed=True)], 2),
        # the last column of chunk 0 and of chunk 1, the first of chunk 1 and of chunk 2: one partner each
        pair("seam", ("cut", 63), 307, [(0, 1.0), (CH - 1, 1.0), (CH, 1.0), (2 * CH - 1, 1.0), (2 * CH, 1.0)],
             [dict(idx=64, at=[(CH - 1, 0.8)], removed=True), dict(idx=65, at=[(CH, 0.8)], removed=True),
              dict(idx=100, at=[(2 * CH - 1, 0.8)], removed=True), dict(idx=124, at=[(2 * CH, 0.8)], removed=True)], 3),
        # 0.2 in chunk 0 and 0.2 in chunk 1: P = 0.4 > 0.3 only when both count
        pair("sum", ("cut", 10), 401, sum_pe, [dict(idx=40, at=sum_at, removed=True)], 2),
        # +0.4 in chunk 0, -0.4 in chunk 2: P = 0, kept; either chunk alone removes it
        pair("cancel", ("cut", 126), 503, can_pe, [dict(idx=127, at=can_at, removed=False)], 3),
        # the pivot's entry at mn + 100 and the partner's only entry at mn + CH + 100 share an LDS slot in different chunks: P = 0
        pair("alias", ("cut", 128), 601, [(0, 1.0), (100, 1.0), (CH + 50, 1.0)],
             [dict(idx=130, at=[(CH + 100, 0.8)], removed=False)], 2),
        # the last chunk is cut short by n_vars: mx = V - 1
        pair("top", ("cut", 20), V - 1 - CH - 1000, [(0, 1.0), (CH + 1000, 1.0)], [dict(idx=90, at=[(CH + 1000, 0.5)], removed=True)],
             2),
        # a duplicate (row, col) entry on the first column of chunk 1: 0.5 + 0.5; with one of the two P = 0.25 < 0.3
        pair("dup", ("cut", 66), 751, [(0, 1.0), (CH, 0.5), (CH, 0.5)], [dict(idx=120, at=[(CH, 0.5)], removed=True)], 2),
        # forced rows as pivots of the sum and of the cancellation
        pair("forced_sum", ("forced", 0), 809, sum_pe, [dict(idx=30, at=sum_at, removed=True)], 2),
        pair("forced_cancel", ("forced", 1), 907, can_pe, [dict(idx=110, at=can_at, removed=False)], 3),
    ]


def _chunk_sample(seed):
    V, K = A_V, A_K
    pairs = _chunk_pairs(V)
    hand = {}      # cut index -> (entries, score)
    forced = {}
    n_piv = 0
    n_par = 0
    for p in pairs:
        kind, i = p["pivot"]
        if kind == "cut":
            hand[i] = (p["entries"], 1.0 - 0.005 * n_piv)        # the pivots rank first, the best score is exactly 1: t = 0.9f
            n_piv += 1
        else:
            forced[i] = p["entries"]
        for partner in p["partners"]:
            assert partner["idx"] > i or kind == "forced"
            hand[partner["idx"]] = (partner["entries"], 0.05 + 0.01 * n_par)    # every partner is low
            n_par += 1
    assert len(hand) == n_piv + n_par, "a cut index used twice"
    used = [np.unique([c for c, _ in p["entries"]] + [c for q in p["partners"] for c, _ in q["entries"]]) for p in pairs]
    all_used = np.concatenate(used)
    assert np.unique(all_used).size == all_used.size and all_used.min() >= 0 and all_used.max() == V - 1, "pairs share a column"
    # the random rows draw from all of V except the hand-placed columns, so a pair's verdict depends on its own products alone
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(V), all_used)
    fill = random_rows(rng, K - len(hand), pool)
    fill_q = rng.uniform(0.25, 0.93, len(fill)).astype(np.float32)
    cut, q, k = [], np.zeros(K, np.float32), 0
    for i in range(K):
        if i in hand:
            cut.append(_row(hand[i][0]))
            q[i] = hand[i][1]
        else:
            cut.append(fill[k])
            q[i] = fill_q[k]
            k += 1
    return dict(cut=cut, forced=[_row(forced[r]) for r in sorted(forced)], q=q, V=V), pairs


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def chunk_seed():
    """(seed, rejected): the first seed of the random fill whose restatement keeps clear margins (eps = 1e-9, one ulp around t)."""
    def find():
        for seed in range(20):
            sample, _ = _chunk_sample(seed)
            if R.margins_ok(restate_sample(sample, *A_THR)[2], *A_THR):
                return seed, seed
        raise AssertionError("no seed of the random fill has clear margins")
    return _cached("chunk_seed", find)


def chunk_case():
    def make():
        sample, pairs = _chunk_sample(chunk_seed()[0])
        case = stack([sample], *A_THR, name="chunks")
        case["pairs"] = pairs
        return case
    return _cached("chunks", make)


def chunk_union_case():
    """A as sample 1 of three: c_off, f_off and a column offset that are not zero."""
    def make():
        rng = np.random.default_rng(77)
        first, last = random_sample(rng, 20, 50, 1), random_sample(rng, 70, 30, 0)
        return stack([first, chunk_case()["samples"][0], last], *A_THR, name="chunks-in-union")
    return _cached("chunks-in-union", make)


def pair_partials(pair, partner):
    """{chunk of the pivot: sum of the products pivot x partner in that chunk}, in fp64 from the float32 values."""
    piv = {}
    for c, v in pair["entries"]:
        piv[c] = piv.get(c, 0.0) + float(_f32(v))
    out = {}
    for c, v in partner["entries"]:
        if c in piv:
            ch = chunk_of(c, pair["mn"])
            out[ch] = out.get(ch, 0.0) + piv[c] * float(_f32(v))
    return out


# ---- B: more pivots than blocks -----------------------------------------------------------------------------------------------------
B_SAMPLES, B_V, B_THR, B_SEED = 1040, 16, (0.1, 0.5), 5


def _grid_samples():
    samples = []
    for s in range(B_SAMPLES):
        for attempt in range(20):
            rng = np.random.default_rng([B_SEED, s, attempt])
            sample = random_sample(rng, int(rng.integers(40, 91)), B_V, int(rng.integers(0, 3)))
            if R.margins_ok(restate_sample(sample, *B_THR)[2], *B_THR):
                break
        else:
            raise AssertionError(f"sample {s}: no seed with clear margins")
        samples.append(sample)
    return samples


def grid_case():
    """The union, with `beyond` (samples all of whose pivot rows are global rows >= GRID), `straddle` (the sample that holds row
    GRID - 1 and row GRID) and `alias`: (sample a, row ga, sample b) -- cut 0 of sample b is global row ga + GRID, the second pivot
    of the block whose first pivot is row ga.  Row ga has entries in its LDS slots 0 and 5; cut 0 of b has none in slot 5, cut 1 of b
    has its only entry there: P = 0, unless the vector still holds the earlier pivot."""
    def make():
        samples = _grid_samples()
        start = np.cumsum([0] + [len(s["cut"]) + len(s["forced"]) for s in samples])
        alias = None
        for b in range(B_SAMPLES):
            ga = int(start[b]) - GRID
            if ga < 0:
                continue
            a = int(np.searchsorted(start, ga, side="right")) - 1
            la = ga - int(start[a])
            if la >= len(samples[a]["cut"]) - 1:          # a forced row or the last cut: take the next sample
                continue
            sa, sb = dict(samples[a]), dict(samples[b])
            sa["cut"] = list(sa["cut"]); sb["cut"] = list(sb["cut"]); sb["q"] = sb["q"].copy()
            sa["cut"][la] = _row([(1, 1.0), (6, 1.0)])
            sb["cut"][0], sb["cut"][1] = _row([(2, 1.0)]), _row([(7, 1.0)])
            sb["q"][0], sb["q"][1] = 2.0, 1.9
            Pb = parallelisms(sb)
            stale = Pb[0].copy()
            stale[0, 1] = stale[1, 0] = 1.0                   # what a vector that still holds row ga makes of the pair
            seen = not same(restate_sample(sb, *B_THR, P=(stale, Pb[1])), restate_sample(sb, *B_THR, P=Pb))
            if seen and all(R.margins_ok(restate_sample(s, *B_THR)[2], *B_THR) for s in (sa, sb)):
                samples[a], samples[b] = sa, sb
                alias = (a, ga, b)
                break
        assert alias is not None
        case = stack(samples, *B_THR, name="grid")
        case["start"] = start
        case["beyond"] = [s for s in range(B_SAMPLES) if start[s] >= GRID]
        case["straddle"] = [s for s in range(B_SAMPLES) if start[s] < GRID < start[s + 1]]
        case["alias"] = alias
        return case
    return _cached("grid", make)


# ---- C: exact ties ----------------------------------------------------------------------------------------------------------------
C_THR = (0.25, 0.5)
TIE_VARIANTS = ("below", "equal", "tform", "forced-below", "forced-equal", "forced-tform")


def t_float32_form(q0):
    """t as a float32 product: 0.9 rounded to float32 first (what NumPy >= 2 and a careless kernel compute)."""
    return _f32(_f32(0.9) * _f32(q0))


def tie_case(variant):
    """Pivot e_0 with the best score q0; partners c * e_0 + 0.5 * e_private:
        cut 1  c = 0.25          low       kept     P == p_max
        cut 2  c = 0.25 + 2^-20  q == t    kept     not low: Q < t is strict
        cut 3  c = 0.25 + 2^-20  q3        removed when q3 < t ("below": nextafter(t, 0); "tform": the float32 product, one ulp
                                           below t for q0 = 0.75), kept for q3 == t ("equal")
        cut 4  c = 0.5           not low   kept     P == p_max_ub
        cut 5  c = 0.5 + 2^-20   not low   removed
    "forced-*": e_0 is a forced row and cut 0 lies on a column of its own; the verdicts are the same.
    `want`: (order, n_kept) worked out by hand; `P`: the intended parallelisms with the pivot, cut by cut."""
    forced = variant.startswith("forced-")
    kind = variant.split("-")[-1]
    q0 = _f32(0.75 if kind == "tform" else 1.0)
    t = R.threshold(q0)
    q3 = {"below": np.nextafter(t, _f32(0)), "equal": t, "tform": t_float32_form(q0)}[kind]
    coef = [0.25, 0.25 + EPS, 0.25 + EPS, 0.5, 0.5 + EPS]
    cut = [_row([(9, 1.0)] if forced else [(0, 1.0)])] + [_row([(0, c), (j + 1, 0.5)]) for j, c in enumerate(coef)]
    q = np.array([q0, _f32(0.1) * q0, t, q3, _f32(0.95 * float(q0)), _f32(0.96 * float(q0))], np.float32)
    sample = dict(cut=cut, forced=[_row([(0, 1.0)])] if forced else [], q=q, V=10)
    case = stack([sample], *C_THR, name="tie-" + variant)
    case["P"] = np.array(coef)
    case["t"], case["q0"] = t, q0
    # ranking: 0, 5, 4, then 2 and 3 (2 first: q2 >= q3, ties in index order), 1
    case["want"] = ([0, 4, 2, 3, 1, 5], 5) if kind == "equal" else ([0, 4, 2, 1, 5, 3], 4)
    return case
