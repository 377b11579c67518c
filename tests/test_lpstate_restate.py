"""The LP-snapshot restatement (tests/lpstate_restate.py) against answers worked out by hand on a small LP, its invariants on the
synthetic generator, and the host checks of a snapshot.  No GPU."""
import dataclasses

import numpy as np
import pytest

import lpstate_restate as R
from gcnn_cut_selector_amd import lpstate, synthetic

INF = 1e20
S5 = np.sqrt(5.0)
f32 = np.float32


def small_lp(**over):
    """4 rows x 4 columns, 3 cuts; obj = (3, 0, 4, 0), norm 5; lp = (1, 0.5, 0.25, 2).
    rows: an equality row 3 x0 + 4 x1 = 10; a >= row 2 x1 >= 1; a free-lhs row x0 + 2 x3 <= 4; a zero-norm row 0 x2 <= 5.
    cuts: A = 4 x2 + 3 x3 in [5, 9], activity 7: (5 - 7) == (7 - 9), the tie goes to rhs; B = 3 x0 + 4 x1 in [7, 9], activity 5: the
    lhs is the violated side; C = 2 x0 <= 1, activity 2."""
    f = dict(row_ptr=[0, 2, 3, 5, 6], row_col=[0, 1, 1, 0, 3, 2], row_val=[3.0, 4.0, 2.0, 1.0, 2.0, 0.0],
             row_lhs=[10.0, 1.0, -INF, -INF], row_rhs=[10.0, INF, 4.0, 5.0], row_dual=[5.0, -2.0, 0.0, 1.0], row_basis=[2, 0, 1, 1],
             col_type=[0, 1, 3, 2], col_obj=[3.0, 0.0, 4.0, 0.0], col_lb=[0.0, 0.0, -INF, 0.0], col_ub=[1.0, INF, INF, 5.0],
             col_basis=[2, 1, 0, 3], col_lp=[1.0, 0.5, 0.25, 2.0], col_redcost=[-10.0, 0.0, 5.0, 0.0],
             cut_ptr=[0, 2, 4, 5], cut_col=[2, 3, 0, 1, 0], cut_val=[4.0, 3.0, 3.0, 4.0, 2.0],
             cut_lhs=[5.0, 7.0, -INF], cut_rhs=[9.0, 9.0, 1.0])
    f.update(over)
    return lpstate.LPSnapshot(**{k: (np.asarray(v) if isinstance(v, list) else v) for k, v in f.items()})


def test_small_lp_without_incumbent():
    ref = R.restate(small_lp())
    c, cei, cef, v, k, kei, kef, C, V, K = ref["inputs"]
    assert (C, V, K) == (5, 4, 3)
    assert ref["dims"]["n_state_rows"] == 5 and ref["dims"]["n_state_edges"] == 8        # the host's size computation
    # lhs copies of rows 0 and 1, negated; then rhs copies of rows 0, 2, 3; the zero-norm row divides by 1
    want = [[-2.0, 0, -9 / 25, -5 / 25], [-0.5, 1, 0.0, 2 / 10], [2.0, 1, 9 / 25, 5 / 25], [4 / S5, 0, 3 / (S5 * 5), 0.0], [5.0, 0, 0.0, 1 / 5]]
    np.testing.assert_array_equal(c, np.array(want, f32))
    assert c.dtype == f32 and cei.dtype == np.int32
    np.testing.assert_array_equal(cei, [[0, 0, 1, 2, 2, 3, 3, 4], [0, 1, 1, 0, 1, 0, 3, 2]])
    np.testing.assert_array_equal(cef[:, 0], np.array([-3 / 5, -4 / 5, -1.0, 3 / 5, 4 / 5, 1 / S5, 2 / S5, 0.0], f32))
    want_v = [[1, 0, 0, 0, 3 / 5, 1, 1, 0, 1, 0.0, -2.0, 1.0, 0, 0], [0, 1, 0, 0, 0.0, 1, 0, 0, 0, 0.5, 0.0, 0.5, 0, 0],
              [0, 0, 0, 1, 4 / 5, 0, 0, 1, 0, 0.0, 1.0, 0.25, 0, 0], [0, 0, 1, 0, 0.0, 1, 1, 0, 0, 0.0, 0.0, 2.0, 0, 0]]
    np.testing.assert_array_equal(v, np.array(want_v, f32))
    # B (lhs side) comes first, then A (the tie: rhs) and C in input order
    assert ref["cut_index"].tolist() == [1, 0, 2] and ref["side_lhs"].tolist() == [False, True, False]
    want_k = [[-7 / 5, 2 / 4, 1.0, 2 / 5, 0, 9 / 25], [9 / 5, 2 / 4, 0.5, -2 / 5, 0, 16 / 25], [1 / 2, 1 / 4, 1.0, 1 / 2, 0, 6 / 10]]
    np.testing.assert_array_equal(k, np.array(want_k, f32))
    np.testing.assert_array_equal(kei, [[0, 0, 1, 1, 2], [0, 1, 2, 3, 0]])
    np.testing.assert_array_equal(kef[:, 0], np.array([-3 / 5, -4 / 5, 4 / 5, 3 / 5, 1.0], f32))
    assert ref["margin"].tolist() == [0.0, 6.0, np.inf]
    assert not ref["margin"][0] > ref["margin_bound"][0] and ref["margin"][1] > ref["margin_bound"][1]


def test_small_lp_with_incumbent_and_near_zero_direction():
    # the incumbent differs from the LP solution in x0 only: direction (1, 0, 0, 0).  A has no x0: d = 0 -> sum_epsilon
    snap = small_lp(col_primal=[2.0, 0.5, 0.25, 2.0], col_primal_avg=[1.5, 0.5, 0.0, 1.0])
    ref = R.restate(snap)
    v, k = ref["inputs"][3], ref["inputs"][4]
    np.testing.assert_array_equal(v[:, 12:], np.array([[2.0, 1.5], [0.5, 0.5], [0.25, 0.0], [2.0, 1.0]], f32))
    np.testing.assert_array_equal(k[:, 4], np.array([2 / 3, -2 / 1e-6, 1 / 2], f32))
    # a direction almost orthogonal to A: |d| = 1e-9 <= sum_epsilon, whatever its sign
    for sign in (1.0, -1.0):
        snap = small_lp(col_primal=[2.0, 0.5, 0.25, 2.0 + sign * 1e-9 / 3], col_primal_avg=[0.0] * 4)
        assert R.restate(snap)["inputs"][4][1, 4] == f32(-2 / 1e-6)
    # a cutoff distance beyond infinity is capped; obj_norm <= 0 counts as 1
    snap = small_lp(cut_lhs=[-INF, 7.0, -INF], cut_rhs=[5.0, 9.0, 1.0], col_primal=[2.0, 0.5, 0.25, 2.0], col_primal_avg=[0.0] * 4,
                    infinity=1e5)
    # A is violated by 2 on its rhs now and d = 0 -> 2 / 1e-6 = 2e6, capped at infinity = 1e5
    assert R.restate(snap)["inputs"][4][1, 4] == f32(1e5)
    assert R.restate(small_lp(col_obj=[0.0] * 4))["inputs"][3][:, 4].tolist() == [0.0] * 4
    assert small_lp(col_obj=[0.0] * 4).scalars()[3] == 1.0 and small_lp(obj_norm=-2.0).scalars()[3] == 1.0


@pytest.mark.parametrize("problem", synthetic.PROBLEMS)
def test_invariants_on_the_generator(problem):
    for kw in (dict(), dict(incumbent=False, row_sides="ranged"), dict(row_sides="rhs_only", cut_sides="lhs", n_cuts=1)):
        snap = synthetic.make_lp_snapshot(problem, 0, scale=0.1, **kw)
        ref = R.restate(snap)
        c, cei, cef, v, k, kei, kef, C, V, K = ref["inputs"]
        d = ref["dims"]
        assert (d["n_state_rows"], d["n_state_edges"]) == (C, cei.shape[1]) and (c.shape[0], v.shape[0], k.shape[0]) == (C, V, K)
        assert kei.shape[1] == d["cut_nnz"] and lpstate.state_key(d) == (C, V, K, cei.shape[1], kei.shape[1])
        for ei, n_left in ((cei, C), (kei, K)):
            key = ei[0].astype(np.int64) * V + ei[1]
            assert np.all(np.diff(key) > 0) and (ei.size == 0 or (0 <= ei.min() and ei[0].max() < n_left and ei[1].max() < V))
        assert sorted(ref["cut_index"].tolist()) == list(range(K))
        n_lhs = int(ref["side_lhs"].sum())
        assert ref["side_lhs"][ref["cut_index"][:n_lhs]].all() and not ref["side_lhs"][ref["cut_index"][n_lhs:]].any()
        assert np.all(np.diff(ref["cut_index"][:n_lhs]) > 0) and np.all(np.diff(ref["cut_index"][n_lhs:]) > 0)
        assert np.all(ref["margin"] > ref["margin_bound"])                     # the generator keeps every side choice off its tie
        assert np.all(np.isfinite(k)) and np.all(np.isfinite(c)) and np.all(np.isfinite(v))
        if kw.get("row_sides") == "rhs_only":
            assert C == d["n_rows"] and K == 1 and n_lhs == 1
        if kw.get("row_sides") == "ranged":
            assert C == 2 * d["n_rows"] and np.all(v[:, 12:] == 0) and np.all(k[:, 4] == 0)


def test_check_snapshot_rejects_contract_violations():
    good = small_lp()
    lpstate.check_snapshot(good)
    bad = {
        "unsorted row": dict(row_col=[1, 0, 1, 0, 3, 2]),
        "duplicate column": dict(cut_col=[2, 2, 0, 1, 0]),
        "empty cut": dict(cut_ptr=[0, 2, 2, 5]),
        "column out of range": dict(cut_col=[2, 4, 0, 1, 0]),
        "negative column": dict(row_col=[0, 1, 1, 0, 3, -1]),
        "offsets": dict(row_ptr=[0, 3, 2, 5, 6]),
        "offsets end": dict(row_ptr=[0, 2, 3, 5, 7]),
        "lengths": dict(row_dual=[1.0, 2.0]),
        "codes": dict(col_basis=[0, 1, 2, 4]),
        "primal alone": dict(col_primal=[1.0] * 4),
        "index width": dict(cut_col=np.array([2, 3, 0, 1, 2 ** 32], np.int64)),
        "model vars": dict(n_model_vars=0),
    }
    for name, over in bad.items():
        with pytest.raises(ValueError):
            lpstate.check_snapshot(small_lp(**over))
    # the cheap check leaves the O(nnz) facts to the device, and nothing else
    lpstate.check_snapshot(small_lp(row_col=[1, 0, 1, 0, 3, 2]), deep=False)
    lpstate.check_snapshot(small_lp(cut_col=[2, 4, 0, 1, 0]), deep=False)
    for name in ("empty cut", "offsets", "lengths", "codes"):
        with pytest.raises(ValueError):
            lpstate.check_snapshot(small_lp(**bad[name]), deep=False)
    # dtypes are cast while packing, fields keep their order
    arrays, dims = lpstate.check_snapshot(dataclasses.replace(good, row_col=good.row_col.astype(np.int64)))
    assert [a.dtype for a in arrays] == [np.dtype(dt) for _, dt in lpstate.FIELDS] and len(arrays) == 21
