"""Hand-worked cases that pin the NumPy restatement of the cut selection (tests/cutsel_restate.py) -- the yardstick the device
selection is compared with in test_gpu_select.py.  CPU only."""
import numpy as np

import cutsel_restate as R

S96 = float(np.sqrt(0.96))


def rows(*vecs):
    """Dense rows from short coefficient lists (a row is a list of (col, value))."""
    V = 1 + max((c for v in vecs for c, _ in v), default=0)
    a = np.zeros((len(vecs), max(V, 3)))
    for i, v in enumerate(vecs):
        for c, x in v:
            a[i, c] += np.float32(x)
    return a


def run(q, cuts, forced=None, **kw):
    order, n = R.select(np.array(q, np.float32), cuts, forced, **kw)
    return order.tolist(), n


def test_duplicate_of_the_best_cut_is_removed():
    assert run([0.5, 1.0, 0.2], rows([(0, 1)], [(1, 1)], [(1, 1)])) == ([1, 0, 2], 2)


def test_low_quality_is_indexed_by_position():
    # state order: D (0.85), A (1.0), B (0.95, a copy of A), C (0.92); P(C, D) = 0.3.  A removes B, so D moves from position 3
    # (low: 0.85 < 0.9) to position 2, whose Q = 0.92 is not low: C does not remove D.  Indexed by cut, D would go.
    cuts = rows([(1, 0.3), (2, float(np.sqrt(0.91)))], [(0, 1)], [(0, 1)], [(1, 1)])
    assert run([0.85, 1.0, 0.95, 0.92], cuts) == ([1, 3, 0, 2], 3)


def test_forced_rows_remove_cuts():
    cuts = rows([(0, 1)], [(1, 1)], [(2, 1)])
    # f0 is cut 2 itself (low: removed); f1 = 0.6 e1 + 0.8 e0 removes the best cut through p_max_ub and cut 0 as low
    f0 = rows([(2, 1)])
    assert run([0.3, 0.9, 0.5], cuts, f0) == ([1, 0, 2], 2)
    f01 = rows([(2, 1)], [(1, 0.6), (0, 0.8)])
    assert run([0.3, 0.9, 0.5], cuts, f01) == ([2, 1, 0], 0)


def test_negative_best_score_makes_every_position_low():
    cuts = rows([(0, 1)], [(0, 0.2), (1, S96)])          # P = 0.2: above p_max, below p_max_ub
    assert run([-1.0, -2.0], cuts) == ([0, 1], 1)       # t = -0.9: -2 < t and -1 < t
    assert run([1.0, 0.95], cuts) == ([0, 1], 2)        # t = 0.9: neither is low, nothing goes


def test_p_max_ub_removes_a_high_quality_cut():
    assert run([1.0, 0.99], rows([(0, 1)], [(0, 0.6), (1, 0.8)])) == ([0, 1], 1)
    assert run([1.0, 0.99], rows([(0, 1)], [(0, 0.4), (1, float(np.sqrt(0.84)))])) == ([0, 1], 2)


def test_two_removal_rounds_keep_the_tail_in_removal_order():
    # state order D B A E C; A removes its copy B, then C removes its copy D: B stays ahead of D in the tail
    cuts = rows([(1, 1)], [(0, 1)], [(0, 1)], [(2, 1)], [(1, 1)])
    assert run([0.4, 0.5, 1.0, 0.3, 0.8], cuts) == ([2, 4, 3, 1, 0], 3)


def test_nan_scores_rank_last_and_are_never_low():
    cuts = rows([(0, 0.3), (1, float(np.sqrt(0.91)))], [(0, 1)], [(2, 1)])
    # NaN ranks as -inf (position 2); its Q is NaN, NaN < t is False, and P = 0.3 < p_max_ub: the best cut keeps it
    assert run([np.nan, 1.0, 0.5], cuts) == ([1, 2, 0], 3)
    assert run([0.2, 1.0, 0.5], cuts) == ([1, 2, 0], 2)


def test_threshold_is_the_float64_product_rounded_to_float32():
    rng = np.random.default_rng(0)
    q0 = rng.uniform(0.1, 10, 20000).astype(np.float32)
    t64 = (0.9 * q0.astype(np.float64)).astype(np.float32)     # NumPy 1.22: float32 scalar * 0.9 -> float64
    t32 = np.float32(0.9) * q0                                   # NumPy >= 2: 0.9 rounded first, product in float32
    differ = np.nonzero(t64 != t32)[0]
    assert differ.size > 0
    for i in differ[:50]:
        assert R.threshold(q0[i]) == t64[i]


def test_record_and_margins():
    rec = {}
    R.select(np.array([1.0, 0.5], np.float32), rows([(0, 1)], [(0, 0.5), (1, float(np.sqrt(0.75)))]), record=rec)
    assert rec["P"].size == 1 and not R.margins_ok(rec, 0.1, 0.5)   # P = 0.5 sits on p_max_ub
    R.select(np.array([1.0, 0.5], np.float32), rows([(0, 1)], [(0, 0.3), (1, float(np.sqrt(0.91)))]), record=rec)
    assert R.margins_ok(rec, 0.1, 0.5)
