"""LP snapshots at the places where the state builder (csrc/k_lpstate.hpp) changes path: more than one 256-entry chunk of cuts, rows
or columns, more than 256 chunks of a kind (the second trip of the strided loops over the chunk tables), rows and cuts whose lengths
sit around the 16 lanes that share one, free and empty rows at chunk borders, and K just past the ranking / selection limit.
Built directly as `lpstate.LPSnapshot` from explicit numpy.random.default_rng seeds: `synthetic.make_lp_snapshot` is not touched.
The hand-made degenerate cases are `small_lp()` variants of tests/test_lpstate_restate.py (`hand_cases`).

`snapshot(name)` and `reference(name)` are computed once per process and shared: nobody writes into them."""
import functools

import numpy as np

import lpstate_restate as R
from gcnn_cut_selector_amd import lpstate

CHUNK = 256                                          # LP_NT: rows / columns / cuts per block
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 40)         # around LP_SUB = 16 lanes a row: one trip, one trip full, a second, a third
INF = 1e20

# name -> sizes, seed, and whether gcnn_lp_infer takes the snapshot (`single_call`; past 32,768 variables it does not).
# "short_rows": row lengths 0..2 instead of LENGTHS + (0,).
SEAM = {
    # cuts across chunks: the pre[] / tot[] terms of a cut's place, cut_part beyond chunk 0
    "cuts255": dict(seed=11, R=8, V=64, K=255),
    "cuts256": dict(seed=12, R=8, V=64, K=256),
    "cuts257": dict(seed=13, R=7, V=80, K=257),
    "cuts513": dict(seed=14, R=9, V=64, K=513),
    "cuts1100": dict(seed=15, R=8, V=300, K=1100),
    # rows across chunks, with free and empty rows at the first and last position of every chunk
    "rows1": dict(seed=21, R=1, V=64, K=12),
    "rows255": dict(seed=22, R=255, V=64, K=12),
    "rows256": dict(seed=23, R=256, V=64, K=11),
    "rows257": dict(seed=24, R=257, V=100, K=12),
    "rows600": dict(seed=25, R=600, V=64, K=13),
    # columns across chunks: the two norm partials (|col_obj|, |primal - lp|)
    "cols255": dict(seed=31, R=8, V=255, K=12),
    "cols256": dict(seed=32, R=8, V=256, K=12),
    "cols257": dict(seed=33, R=8, V=257, K=12),
    # more than 256 chunks of a kind: the strided loops over the chunk tables take a second trip
    "cols70000": dict(seed=41, R=6, V=70000, K=12, single_call=False),
    "rows66000": dict(seed=42, R=66000, V=64, K=12, short_rows=True),
    # just past the limit of the device ranking and of the selection
    "cuts4097": dict(seed=51, R=8, V=64, K=4097),
}
for _case in SEAM.values():
    _case.setdefault("single_call", True)
    _case.setdefault("short_rows", False)


def _columns(rng, lens, V):
    """Per row `lens[i]` distinct columns of [0, V), increasing: CSR (ptr, col)."""
    n = lens.shape[0]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    if n * V <= 1 << 23:
        order = np.argsort(rng.random((n, V)), axis=1)                       # a random permutation per row; its head is the draw
        picked = np.where(np.arange(V)[None, :] < lens[:, None], order, V)
        picked.sort(axis=1)
        col = picked[picked < V]
    else:
        col = np.concatenate([np.sort(rng.choice(V, size=int(m), replace=False)) for m in lens] + [np.zeros(0, np.int64)])
    return ptr, col.astype(np.int32)


def _chunk_ends(n):
    return [(b, min(b + CHUNK, n) - 1) for b in range(0, n, CHUNK)]


def _make(seed, R, V, K, short_rows, **_):
    rng = np.random.default_rng(seed)
    # ---- columns (as synthetic.make_lp_snapshot draws them, with every column type)
    col_type = rng.integers(0, 4, V).astype(np.int8)
    col_obj = rng.standard_normal(V)
    col_lb = np.where(rng.random(V) < 0.1, -INF, 0.0)
    col_ub = np.where(rng.random(V) < 0.2, INF, 1.0)
    col_basis = rng.integers(0, 4, V).astype(np.int8)
    col_lp = np.where(rng.random(V) < 0.5, rng.integers(0, 2, V).astype(np.float64), rng.random(V))
    col_redcost = rng.standard_normal(V) * (col_basis != 1)
    primal = np.where(col_type == 3, rng.random(V), rng.integers(0, 2, V).astype(np.float64))
    avg = 0.5 * (primal + rng.random(V))

    # ---- rows: 0 <=, 1 >=, 2 equality, 3 ranged, 4 free; lengths from LENGTHS and 0
    rlens = rng.integers(0, 3, R) if short_rows else rng.choice(LENGTHS + (0,), R)
    kind = rng.choice(5, R, p=[0.3, 0.2, 0.15, 0.2, 0.15])
    if R >= CHUNK - 1:
        # a free row and an empty row with both sides at the first and the last position of every chunk, alternating
        for i, (first, last) in enumerate(_chunk_ends(R)):
            if first == last:                                               # a chunk of one row: ranged, with entries, so that
                kind[first], rlens[first] = 3, 17                           # all four counts in front of it matter
                continue
            free, empty = (first, last) if i % 2 == 0 else (last, first)
            kind[empty], rlens[empty] = 3, 0
            kind[free], rlens[free] = 4, max(int(rlens[free]), 1)
            if first + 2 < last:                                            # and every chunk lists both sides with entries
                kind[first + 1], rlens[first + 1] = 1, max(int(rlens[first + 1]), 1)
                kind[first + 2], rlens[first + 2] = 0, max(int(rlens[first + 2]), 1)
    else:
        kind[0], rlens[0] = 3, 17
    row_ptr, row_col = _columns(rng, rlens, V)
    row_val = np.round(rng.uniform(0.5, 3.0, row_col.size), 3) * rng.choice([-1.0, 1.0], row_col.size)
    activity = np.bincount(np.repeat(np.arange(R), rlens), weights=row_val * col_lp[row_col], minlength=R)
    slack = rng.uniform(0.0, 2.0, R) * (rng.random(R) < 0.7)
    row_rhs = np.where((kind == 1) | (kind == 4), INF, activity + slack)
    row_lhs = np.where(kind == 2, row_rhs, activity - rng.uniform(0.0, 2.0, R))
    row_lhs = np.where(kind == 1, activity - slack, np.where((kind == 0) | (kind == 4), -INF, row_lhs))
    row_basis = np.where(slack == 0, np.where(kind == 1, 0, 2), 1).astype(np.int8)
    row_dual = rng.standard_normal(R) * (row_basis != 1)

    # ---- cuts: 0 rhs, 1 lhs, 2 ranged -> rhs, 3 ranged -> lhs, each clearly off its tie
    klens = rng.choice(LENGTHS, K)
    ckind = rng.integers(0, 4, K)
    for i, (first, last) in enumerate(_chunk_ends(K)):
        if first == last:
            ckind[first] = 3 if i % 2 else 2                                # a chunk of one cut: lhs in an odd chunk, rhs in an even one
        else:
            ckind[first], ckind[last] = (3, 0) if i % 2 == 0 else (2, 1)    # both sides in every chunk, at its borders
    cut_ptr, cut_col = _columns(rng, klens, V)
    cut_val = np.round(rng.standard_normal(cut_col.size), 3) + 0.0005        # (never exactly zero)
    kact = np.bincount(np.repeat(np.arange(K), klens), weights=cut_val * col_lp[cut_col], minlength=K)
    viol = rng.uniform(0.1, 1.0, K)
    cut_rhs = np.where(ckind == 0, kact - viol, np.where(ckind == 1, INF, np.where(ckind == 2, kact - viol, kact + 1.0 + viol)))
    cut_lhs = np.where(ckind == 0, -INF, np.where(ckind == 1, kact + viol, np.where(ckind == 2, kact - 1.0 - viol, kact + viol)))
    return lpstate.LPSnapshot(row_ptr=row_ptr, row_col=row_col, row_val=row_val, row_lhs=row_lhs, row_rhs=row_rhs, row_dual=row_dual,
                              row_basis=row_basis, col_type=col_type, col_obj=col_obj, col_lb=col_lb, col_ub=col_ub,
                              col_basis=col_basis, col_lp=col_lp, col_redcost=col_redcost, cut_ptr=cut_ptr, cut_col=cut_col,
                              cut_val=cut_val, cut_lhs=cut_lhs, cut_rhs=cut_rhs, col_primal=primal, col_primal_avg=avg)


@functools.lru_cache(maxsize=None)
def snapshot(name):
    return _make(**SEAM[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 restatement of a seam case: computed once, shared, never written to."""
    return R.restate(snapshot(name))


def assert_seams(name, snap, ref):
    """What makes a seam case one: without these a dropped pre[] or tot[] term of the placement stays invisible."""
    case = SEAM[name]
    side = ref["side_lhs"]
    for first, last in _chunk_ends(case["K"]):
        if last > first:
            assert side[first:last + 1].any() and not side[first:last + 1].all(), (name, "cut chunk", first // CHUNK)
    klens = np.diff(snap.cut_ptr)
    assert set(klens.tolist()) <= set(LENGTHS)
    if case["K"] >= CHUNK - 1:
        assert set(klens.tolist()) == set(LENGTHS)
    lens = np.diff(snap.row_ptr)
    has_l, has_r = lpstate.finite(snap.row_lhs, snap.infinity), lpstate.finite(snap.row_rhs, snap.infinity)
    if case["R"] >= CHUNK - 1:
        for first, last in _chunk_ends(case["R"]):
            if first == last:
                assert has_l[first] and has_r[first] and lens[first] > 0
                continue
            ends = [first, last]
            free = [r for r in ends if not has_l[r] and not has_r[r]]
            empty = [r for r in ends if lens[r] == 0 and has_l[r] and has_r[r]]
            assert len(free) == 1 and len(empty) == 1 and lens[free[0]] > 0, (name, "row chunk", first // CHUNK)
            if first + 2 < last:
                sl = slice(first, last + 1)
                assert (has_l[sl] & (lens[sl] > 0)).any() and (has_r[sl] & (lens[sl] > 0)).any()
        if not case["short_rows"]:
            assert set(lens.tolist()) == set(LENGTHS + (0,))
            kinds = {(bool(a), bool(b), bool(c)) for a, b, c in zip(has_l, has_r, snap.row_lhs == snap.row_rhs)}
            assert kinds == {(False, True, False), (True, False, False), (True, True, True), (True, True, False), (False, False, False)}
    if case["short_rows"]:
        assert set(lens.tolist()) == {0, 1, 2}
    chunks = lambda n: -(-n // CHUNK)  # noqa: E731
    if name == "cols70000":
        assert chunks(case["V"]) > CHUNK
    if name == "rows66000":
        assert chunks(case["R"]) > CHUNK and int(has_l.sum()) + int(has_r.sum()) == ref["inputs"][7]


def assert_sides_exact(snap):
    """The proof that a hand-made case's side choices do not depend on the summation order, so that a tie is a tie on every
    machine: for each cut with a finite lhs (the others take rhs whatever their activity), every coefficient, every LP value it meets
    and both sides are multiples of 2^-10 below 2^20 in magnitude, and the sum of |a_j x_j| stays below 2^32.  Every product is then a
    multiple of 2^-20, so is every partial sum in any order, fused or not, and all of them are below 2^33: 53 bits hold them exactly.
    The same goes for lhs - activity and activity - rhs (below 2^34).  The side is therefore defined by exact arithmetic."""
    inf = snap.scalars()[0]
    ptr = np.asarray(snap.cut_ptr)
    val, lp_at = np.asarray(snap.cut_val, np.float64), np.asarray(snap.col_lp, np.float64)[np.asarray(snap.cut_col)]
    lhs, rhs = np.asarray(snap.cut_lhs, np.float64), np.asarray(snap.cut_rhs, np.float64)

    def dyadic(x):
        x = np.atleast_1d(x)
        return bool(np.all(x * 1024.0 == np.round(x * 1024.0)) and np.all(np.abs(x) < 2.0 ** 20))

    checked = 0
    for k in range(lhs.shape[0]):
        if not lpstate.finite(lhs[k], inf):
            continue
        e = slice(ptr[k], ptr[k + 1])
        assert dyadic(val[e]) and dyadic(lp_at[e]) and dyadic(lhs[k]), k
        assert lpstate.finite(rhs[k], inf) and dyadic(rhs[k]), k
        assert float(np.sum(np.abs(val[e]) * np.abs(lp_at[e]))) < 2.0 ** 32, k
        checked += 1
    return checked


def hand_cases():
    """name -> (snapshot, the whole state worked out by hand): every `small_lp()` variant of tests/test_lpstate_restate.py."""
    from test_lpstate_restate import HAND, small_lp
    return {name: (small_lp(**over), want) for name, (over, want) in HAND.items()}
