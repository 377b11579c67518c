"""Cases of the hybrid selection from cut rows (tests/test_hybridcases.py proves on the host that each discriminates,
tests/test_gpu_hybrid.py runs them on the device).  Three families:

  random   `synthetic.make_lp_snapshot(problem, i, scale=0.3)`, four problems x i = 0..3.  The device may add in another order, so
           features and quality are compared within `hybrid_restate`'s bounds -- and the integers (order, n_kept) with `==`, which
           is sound because test_hybridcases.py asserts the margins (`hybrid_restate.margins`) far above those bounds.
  exact    every sum is exact in any order, so the device must give the restatement's very bits:
             * `plants()`: columns with lp = k/64; rows of small integers whose squares add up to a perfect square (one entry;
               sixteen of +-1: norm 4; (1,2,2): 3; (1,1,1,2,3): 4; (1,1,1,1,1,2): 3; (1,1,1,1,1,2,4): 5), col_obj = sixteen ones
               (|obj| = 4).  A row of n equal powers of two has a power-of-two norm only for n = 1, 4, 16, and parallelism 7/8
               needs the sixteen (15 - 1 = 14 of 16), integer support 3/3 needs three entries: hence the integer norms.  Every
               quotient that is formed is either exact or a single correctly rounded division of exact operands.
             * `tie(kind, forced)`: `selcases.tie_case` with cut rows: a pivot e_0 and partners whose normalised entry on column 0
               is exactly p_max, p_max + 2^-20, p_max_ub, p_max_ub + 2^-20 (p_max = 1/4, p_max_ub = 1/2).  c + 2^-20 as a / |a|
               takes a row of integers with |a| = 2^20: (2^18 + 1, 1015279, 421, 38, 15) and (2^19 + 1, 908091, 1839, 158, 33)
               (Lagrange's four squares for 2^40 - a_0^2).  Partner 3's quality is the threshold 0.9 * q0 itself ("equal":
               kept), one ulp below ("below": low, removed), or one of the two float32 neighbours of 0.675 ("f32up" =
               0.675000011920929: kept; "f32down" = 0.6749999523162842: removed) for q0 = 0.75.
  seams    `make_lp_snapshot` with K = 255 / 256 / 257 / 513 (chunks of 256 cuts), cut lengths 1 .. 40 around the 16 lanes,
           V = 255 / 256 / 257 and 70,000 (more than 256 column chunks), K = 4,096 (served), 4,097 (refused), 0."""
from __future__ import annotations

import numpy as np

import hybrid_restate as H
from gcnn_cut_selector_amd import lpstate, synthetic

PROBLEMS = ("setcov", "combauc", "capfac", "indset")
RANDOM = [(p, i) for p in PROBLEMS for i in range(4)]
INF = 1e20
T_THR = (0.25, 0.5)
TIE_KINDS = ("equal", "below", "f32up", "f32down")
F32_UP, F32_DOWN = 0.675000011920929, 0.6749999523162842
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def random_case(problem, i):
    return _cached(("random", problem, i), lambda: synthetic.make_lp_snapshot(problem, i, scale=0.3))


def reference(case, snap):
    """`hybrid_restate.restate(snap)`, computed once per case and left unchanged."""
    return _cached(("ref",) + tuple(case), lambda: H.restate(snap))


def forced_dense(forced, V):
    """Forced rows as `select_cuts` takes them -> dense fp64 [F, V]."""
    if forced is None:
        return None
    inds, vals, n = forced
    d = np.zeros((n, V))
    np.add.at(d, (np.asarray(inds[0], np.int64), np.asarray(inds[1], np.int64)), np.asarray(vals, np.float32).astype(np.float64))
    return d


def expected(case, snap, forced=None, p_max=0.1, p_max_ub=0.5, **variant):
    """(order, n_kept, record) of the restatement's selection (with `variant`: one of hybrid_restate's variants)."""
    ref = reference(case, snap)
    record = {}
    order, n_kept = H.select(variant.pop("quality", ref["quality"]), ref["rows"], forced_dense(forced, ref["dims"]["n_cols"]), p_max,
                             p_max_ub, record=record, **variant)
    return order, n_kept, record


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def _snapshot(cuts, col_type, col_obj, col_lp):
    """cuts: [(columns, values, lhs, rhs)] -> CutSnapshot (columns sorted within a cut)."""
    ptr, col, val, lhs, rhs = [0], [], [], [], []
    for c, v, lo, hi in cuts:
        o = np.argsort(c)
        col += list(np.asarray(c)[o]); val += list(np.asarray(v, np.float64)[o])
        ptr.append(len(col)); lhs.append(lo); rhs.append(hi)
    return lpstate.CutSnapshot(cut_ptr=np.array(ptr, np.int32), cut_col=np.array(col, np.int32), cut_val=np.array(val, np.float64),
                               cut_lhs=np.array(lhs, np.float64), cut_rhs=np.array(rhs, np.float64),
                               col_type=np.asarray(col_type, np.int8), col_obj=np.asarray(col_obj, np.float64),
                               col_lp=np.asarray(col_lp, np.float64), infinity=INF)


INT_PAIRS = {(3, 3): (1, 2, 2), (1, 5): (1, 1, 1, 2, 3), (3, 6): (1, 1, 1, 1, 1, 2), (2, 7): (1, 1, 1, 1, 1, 2, 4)}   # (nint, nnz): row
FUSED_I = tuple(range(3, 11))


def plants():
    """-> (CutSnapshot, where): `where` names the planted cuts' indices."""
    def make():
        V = 64
        col_obj = np.zeros(V); col_obj[:16] = 1.0
        col_type = np.full(V, 3); col_type[32:48] = np.arange(16) % 3            # integer kinds 0, 1, 2
        col_lp = (np.arange(V) * 7 % 64) / 64.0
        cuts, where = [], {"fused": [], "int": {}}
        act = lambda c, v: float(np.sum(np.asarray(v, np.float64) * col_lp[np.asarray(c)]))  # noqa: E731 -- exact: dyadic terms
        for i in FUSED_I:                                                        # efficacy i/64, parallelism 14/16
            c, v = np.arange(16), np.ones(16)
            v[i] = -1.0
            where["fused"].append(len(cuts))
            cuts.append((c, v, -INF, act(c, v) - i / 16.0))
        for j, ((nint, nnz), row) in enumerate(INT_PAIRS.items()):              # efficacy (j + 2)/1024 (small: the term's last bit survives the sum), parallelism 0
            c = np.concatenate([32 + (np.arange(nint) + 3 * j) % 16, 16 + (np.arange(nnz - nint) + 5 * j) % 16])
            norm = float(np.sqrt(sum(x * x for x in row)))
            where["int"][(nint, nnz)] = len(cuts)
            cuts.append((c, row, -INF, act(c, row) - norm * (j + 2) / 1024.0))
        # single-entry cuts on continuous zero-objective columns with lhs = -inf, rhs = 0: quality = col_lp[j] exactly
        x = 0.7
        col_lp[48], col_lp[49] = x, np.nextafter(x, 1.0)                         # neighbouring doubles, the larger at the higher index
        where["neighbours"] = (len(cuts), len(cuts) + 1)
        cuts += [([48], [1.0], -INF, 0.0), ([49], [1.0], -INF, 0.0)]
        col_lp[50], col_lp[51] = 0.71, 0.0                                       # equal qualities: rhs-sided first, lhs-sided later
        where["sides"] = (len(cuts), len(cuts) + 1)
        cuts += [([50], [1.0], -INF, 0.0), ([51], [1.0], 0.71, INF)]
        return _snapshot(cuts, col_type, col_obj, col_lp), where
    return _cached("plants", make)


ROW_QUARTER_EPS = (2 ** 18 + 1, 1015279, 421, 38, 15)      # a_0 / |a| = 1/4 + 2^-20, |a| = 2^20
ROW_HALF_EPS = (2 ** 19 + 1, 908091, 1839, 158, 33)        # a_0 / |a| = 1/2 + 2^-20


def tie(kind, forced):
    """-> (CutSnapshot, forced rows or None, want = (order, n_kept) worked out by hand as in `selcases.tie_case`)."""
    def make():
        q0 = 0.75
        t = 0.9 * q0
        q3 = {"equal": t, "below": np.nextafter(t, 0.0), "f32up": F32_UP, "f32down": F32_DOWN}[kind]
        rows = [(1.0,) + (1.0,) * 15, ROW_QUARTER_EPS, ROW_QUARTER_EPS, (1.0,) * 4, ROW_HALF_EPS]
        quals = [0.1 * q0, t, q3, 0.95 * q0, 0.96 * q0]
        V, nxt = 64, 1
        cuts = [([40] if forced else [0], [1.0], -INF, -q0)]                  # all lp = 0: efficacy = -rhs / norm
        for row, q in zip(rows, quals):
            c = [0] + list(range(nxt, nxt + len(row) - 1))
            nxt += len(row) - 1
            norm = float(np.sqrt(sum(float(x) * float(x) for x in row)))
            assert norm in (4.0, 2.0, 2.0 ** 20)
            cuts.append((c, row, -INF, -q * norm))                               # a power-of-two norm scales q exactly
        assert nxt <= 40
        snap = _snapshot(cuts, np.full(V, 3), np.zeros(V), np.zeros(V))
        f = (np.array([[0], [0]], np.int32), np.array([1.0], np.float32), 1) if forced else None
        # ranking: 0, 5, 4, then 2 and 3 (2 first when q2 >= q3: ties in index order), 1.  Against the pivot: 5 goes (P > p_max_ub),
        # 4 stays (P == p_max_ub), 1 stays (low, but P == p_max), 2 stays (q == t is not low), 3 goes exactly when q3 < t
        want = {"equal": ([0, 4, 2, 3, 1, 5], 5), "f32up": ([0, 4, 3, 2, 1, 5], 5)}.get(kind, ([0, 4, 2, 1, 5, 3], 4))
        return snap, f, want
    return _cached(("tie", kind, forced), make)


# ---- seams ------------------------------------------------------------------------------------------------------------------------
CUT_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 40)


def with_cut_lengths(snap, lengths, seed):
    """`snap` with its cuts replaced by cuts of the given lengths, violated on their rhs (values as make_lp_snapshot draws them)."""
    rng = np.random.default_rng(seed)
    V = snap.col_type.shape[0]
    cols = [np.sort(rng.choice(V, n, replace=False)) for n in lengths]
    vals = [np.round(rng.standard_normal(n), 3) + 0.0005 for n in lengths]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    col, val = np.concatenate(cols).astype(np.int32), np.concatenate(vals)
    act = np.array([float(np.sum(v * snap.col_lp[c])) for c, v in zip(cols, vals)])
    out = lpstate.LPSnapshot(**{k: getattr(snap, k) for k in snap.__dataclass_fields__})
    out.cut_ptr, out.cut_col, out.cut_val = ptr, col, val
    out.cut_lhs, out.cut_rhs = np.full(len(lengths), -snap.infinity), act - rng.uniform(0.1, 1.0, len(lengths))
    return out


SEAMS = ("K255", "K256", "K257", "K513", "lengths", "V255", "V256", "V257", "V70000", "K4096")


def seam(name):
    def make():
        small = dict(problem="setcov", scale=0.2)                              # 100 rows, 200 columns
        if name.startswith("K"):
            return synthetic.make_lp_snapshot(sample_index=10, n_cuts=int(name[1:]), **small)
        if name == "lengths":
            return with_cut_lengths(synthetic.make_lp_snapshot(sample_index=11, **small), CUT_LENGTHS * 5, 11)
        return synthetic.make_lp_snapshot(sample_index=12, n_cuts=24, extra_cols=int(name[1:]) - 200, **small)
    return _cached(("seam", name), make)


def too_many():
    return _cached("K4097", lambda: synthetic.make_lp_snapshot("setcov", 13, scale=0.2, n_cuts=4097))


def no_cuts():
    def make():
        snap = synthetic.make_lp_snapshot("setcov", 14, scale=0.2, n_cuts=1)
        snap.cut_ptr, snap.cut_col, snap.cut_val = np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)
        snap.cut_lhs = snap.cut_rhs = np.zeros(0)
        return snap
    return _cached("K0", make)
