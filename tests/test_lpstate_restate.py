"""The LP-snapshot restatement (tests/lpstate_restate.py) against answers worked out by hand on a small LP, its invariants on the
synthetic generator and on the seam cases of tests/lpcases.py, and the host checks of a snapshot.  No GPU.  The hand-worked constants
live at module level: tests/test_gpu_lpstate_edges.py holds the device to them as well."""
import dataclasses

import numpy as np
import pytest

import lpcases
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


# ---- the answers worked out by hand on small_lp(), as exact rationals rounded to float32.  tests/test_gpu_lpstate_edges.py imports
# them (through lpcases.hand_cases) and holds the device to the same constants.
# lhs copies of rows 0 and 1, negated; then rhs copies of rows 0, 2, 3; the zero-norm row divides by 1
BASE_C = np.array([[-2.0, 0, -9 / 25, -5 / 25], [-0.5, 1, 0.0, 2 / 10], [2.0, 1, 9 / 25, 5 / 25], [4 / S5, 0, 3 / (S5 * 5), 0.0],
                   [5.0, 0, 0.0, 1 / 5]], f32)
BASE_CEI = np.array([[0, 0, 1, 2, 2, 3, 3, 4], [0, 1, 1, 0, 1, 0, 3, 2]], np.int32)
BASE_CEF = np.array([-3 / 5, -4 / 5, -1.0, 3 / 5, 4 / 5, 1 / S5, 2 / S5, 0.0], f32)
BASE_V = np.array([[1, 0, 0, 0, 3 / 5, 1, 1, 0, 1, 0.0, -2.0, 1.0, 0, 0], [0, 1, 0, 0, 0.0, 1, 0, 0, 0, 0.5, 0.0, 0.5, 0, 0],
                   [0, 0, 0, 1, 4 / 5, 0, 0, 1, 0, 0.0, 1.0, 0.25, 0, 0], [0, 0, 1, 0, 0.0, 1, 1, 0, 0, 0.0, 0.0, 2.0, 0, 0]], f32)
# B (lhs side) comes first, then A (the tie: rhs) and C in input order
BASE_INDEX, BASE_SIDE_LHS = [1, 0, 2], [False, True, False]
BASE_K = np.array([[-7 / 5, 2 / 4, 1.0, 2 / 5, 0, 9 / 25], [9 / 5, 2 / 4, 0.5, -2 / 5, 0, 16 / 25], [1 / 2, 1 / 4, 1.0, 1 / 2, 0, 6 / 10]], f32)
BASE_KEI = np.array([[0, 0, 1, 1, 2], [0, 1, 2, 3, 0]], np.int32)
BASE_KEF = np.array([-3 / 5, -4 / 5, 4 / 5, 3 / 5, 1.0], f32)
# the incumbent differs from the LP solution in x0 only: direction (1, 0, 0, 0).  A has no x0: d = 0 -> sum_epsilon
INCUMBENT = dict(col_primal=[2.0, 0.5, 0.25, 2.0], col_primal_avg=[1.5, 0.5, 0.0, 1.0])
INC_V12 = np.array([[2.0, 1.5], [0.5, 0.5], [0.25, 0.0], [2.0, 1.0]], f32)
INC_K4 = np.array([2 / 3, -2 / 1e-6, 1 / 2], f32)
NEAR_ZERO_K14 = f32(-2 / 1e-6)
# a cutoff distance beyond infinity is capped: A is violated by 2 on its rhs and d = 0 -> 2 / 1e-6 = 2e6, capped at infinity = 1e5
CAPPED = dict(cut_lhs=[-INF, 7.0, -INF], cut_rhs=[5.0, 9.0, 1.0], col_primal=[2.0, 0.5, 0.25, 2.0], col_primal_avg=[0.0] * 4, infinity=1e5)
CAPPED_K14 = f32(1e5)

# (a) the incumbent IS the LP solution: |primal - lp| = 0, every d counts as 0 and becomes sum_epsilon = 1e-6.
#     feasibility: B = min(9 - 5, 5 - 7) = -2, A = min(9 - 7, 7 - 5) = 2, C = min(1 - 2, 2 + 1e20) = -1
#     cutoff = -feasibility / 1e-6 (below infinity = 1e20), in state order B, A, C
SAME_POINT = dict(col_primal=[1.0, 0.5, 0.25, 2.0], col_primal_avg=[0.0] * 4)
SAME_POINT_V12 = np.array([[1.0, 0], [0.5, 0], [0.25, 0], [2.0, 0]], f32)
SAME_POINT_K4 = np.array([2 / 1e-6, -2 / 1e-6, 1 / 1e-6], f32)

# (b) a fourth cut D = 0 x1 in [1, 2] beside the incumbent of INCUMBENT: activity 0, (1 - 0) > (0 - 2): lhs side, so the state
#     order is B, D, A, C.  norm 0 -> 1: rhs feature -(1 / 1); support 1 / 4; x1 is an integer column: 1 / 1; feasibility =
#     min(2 - 0, 0 - 1) = -1: efficacy 1 = -feasibility; d = 0 -> 1e-6: cutoff 1 / 1e-6; parallelism: a norm is 0 -> 0.
#     Its one edge is -(0 / 1) at (1, x1).  B, A, C keep the rows of BASE_K with the cutoffs of INC_K4.
ZERO_CUT = dict(cut_ptr=[0, 2, 4, 5, 6], cut_col=[2, 3, 0, 1, 0, 1], cut_val=[4.0, 3.0, 3.0, 4.0, 2.0, 0.0],
                cut_lhs=[5.0, 7.0, -INF, 1.0], cut_rhs=[9.0, 9.0, 1.0, 2.0], **INCUMBENT)
ZERO_CUT_INDEX, ZERO_CUT_SIDE_LHS = [1, 3, 0, 2], [False, True, False, True]
ZERO_CUT_K = np.array([[-7 / 5, 2 / 4, 1.0, 2 / 5, 2 / 3, 9 / 25], [-1.0, 1 / 4, 1.0, 1.0, 1 / 1e-6, 0.0],
                       [9 / 5, 2 / 4, 0.5, -2 / 5, -2 / 1e-6, 16 / 25], [1 / 2, 1 / 4, 1.0, 1 / 2, 1 / 2, 6 / 10]], f32)
ZERO_CUT_KEI = np.array([[0, 0, 1, 2, 2, 3], [0, 1, 1, 2, 3, 0]], np.int32)
ZERO_CUT_KEF = np.array([-3 / 5, -4 / 5, -0.0, 4 / 5, 3 / 5, 1.0], f32)

# (c) infinity = 1e5 and sides AT it: row 1's rhs is exactly 1e5, row 2's lhs exactly -1e5, x1's upper bound 5e20, and C becomes
#     2 x0 in [-1e5, 3e5].  |x| >= infinity is not finite, so rows, columns and the sides of B and A are those of the base case
#     (a finite 1e5 or -1e5 would add a state row; a finite lhs would put C on its lhs side: (-1e5 - 2) > (2 - 3e5)).  C stays an
#     rhs cut with what the formulas give on the raw numbers: rhs feature 3e5 / 2, feasibility min(3e5 - 2, 2 + 1e5) = 100002,
#     efficacy -100002 / 2.
AT_INFINITY = dict(row_lhs=[10.0, 1.0, -1e5, -INF], row_rhs=[10.0, 1e5, 4.0, 5.0], col_ub=[1.0, 5e20, INF, 5.0],
                   cut_lhs=[5.0, 7.0, -1e5], cut_rhs=[9.0, 9.0, 3e5], infinity=1e5)
AT_INFINITY_K = np.array([[-7 / 5, 2 / 4, 1.0, 2 / 5, 0, 9 / 25], [9 / 5, 2 / 4, 0.5, -2 / 5, 0, 16 / 25],
                          [150000.0, 1 / 4, 1.0, -50001.0, 0, 6 / 10]], f32)

# col_obj = 0 (obj_norm -> 1): cosines and parallelisms 0, duals and reduced costs divided by the row norm alone
ZERO_OBJ_C = np.array([[-2.0, 0, -0.0, -5 / 5], [-0.5, 1, 0.0, 2 / 2], [2.0, 1, 0.0, 5 / 5], [4 / S5, 0, 0.0, 0.0], [5.0, 0, 0.0, 1.0]], f32)
# obj_norm = -2 counts as 1 as well, with the objective in place: cosines a.c / |a|, parallelisms unchanged (they use |col_obj| = 5)
NEG_NORM_C = np.array([[-2.0, 0, -9 / 5, -5 / 5], [-0.5, 1, 0.0, 2 / 2], [2.0, 1, 9 / 5, 5 / 5], [4 / S5, 0, 3 / S5, 0.0], [5.0, 0, 0.0, 1.0]], f32)


def _with(base, columns):
    out = base.copy()
    for c, v in columns.items():
        out[:, c] = v
    return out


def _want(c=BASE_C, v=BASE_V, k=BASE_K, kei=BASE_KEI, kef=BASE_KEF, index=BASE_INDEX):
    """The seven arrays and cut_index of a variant; rows and row edges are those of the base case unless given."""
    return dict(arrays=(c, BASE_CEI, BASE_CEF.reshape(-1, 1), v, k, kei, kef.reshape(-1, 1)), cut_index=np.array(index, np.int32))


_DIR = {s: dict(col_primal=[2.0, 0.5, 0.25, 2.0 + s * 1e-9 / 3], col_primal_avg=[0.0] * 4) for s in (1.0, -1.0)}
_DIR_V = _with(BASE_V, {12: [2.0, 0.5, 0.25, 2.0]})
# name -> (what small_lp() takes, the whole state by hand)
HAND = {
    "base": (dict(), _want()),
    "incumbent": (INCUMBENT, _want(v=_with(BASE_V, {12: INC_V12[:, 0], 13: INC_V12[:, 1]}), k=_with(BASE_K, {4: INC_K4}))),
    "direction+1e-9": (_DIR[1.0], _want(v=_DIR_V, k=_with(BASE_K, {4: INC_K4}))),
    "direction-1e-9": (_DIR[-1.0], _want(v=_DIR_V, k=_with(BASE_K, {4: INC_K4}))),
    # A on its rhs 5: rhs feature 5 / 5, feasibility -2, efficacy 2 / 5, the capped cutoff
    "capped": (CAPPED, _want(v=_DIR_V, k=np.array([[-7 / 5, 2 / 4, 1.0, 2 / 5, 2 / 3, 9 / 25], [5 / 5, 2 / 4, 0.5, 2 / 5, 1e5, 16 / 25],
                                                   [1 / 2, 1 / 4, 1.0, 1 / 2, 1 / 2, 6 / 10]], f32))),
    "zero_objective": (dict(col_obj=[0.0] * 4), _want(c=ZERO_OBJ_C, v=_with(BASE_V, {4: 0.0, 10: [-10.0, 0.0, 5.0, 0.0]}),
                                                      k=_with(BASE_K, {5: 0.0}))),
    "negative_obj_norm": (dict(obj_norm=-2.0), _want(c=NEG_NORM_C, v=_with(BASE_V, {4: [3.0, 0.0, 4.0, 0.0], 10: [-10.0, 0.0, 5.0, 0.0]}))),
    "same_point": (SAME_POINT, _want(v=_with(BASE_V, {12: SAME_POINT_V12[:, 0]}), k=_with(BASE_K, {4: SAME_POINT_K4}))),
    "zero_cut": (ZERO_CUT, _want(v=_with(BASE_V, {12: INC_V12[:, 0], 13: INC_V12[:, 1]}), k=ZERO_CUT_K, kei=ZERO_CUT_KEI,
                                 kef=ZERO_CUT_KEF, index=ZERO_CUT_INDEX)),
    "at_infinity": (AT_INFINITY, _want(k=AT_INFINITY_K)),
}


def test_small_lp_without_incumbent():
    ref = R.restate(small_lp())
    c, cei, cef, v, k, kei, kef, C, V, K = ref["inputs"]
    assert (C, V, K) == (5, 4, 3)
    assert ref["dims"]["n_state_rows"] == 5 and ref["dims"]["n_state_edges"] == 8        # the host's size computation
    np.testing.assert_array_equal(c, BASE_C)
    assert c.dtype == f32 and cei.dtype == np.int32
    np.testing.assert_array_equal(cei, BASE_CEI)
    np.testing.assert_array_equal(cef[:, 0], BASE_CEF)
    np.testing.assert_array_equal(v, BASE_V)
    assert ref["cut_index"].tolist() == BASE_INDEX and ref["side_lhs"].tolist() == BASE_SIDE_LHS
    np.testing.assert_array_equal(k, BASE_K)
    np.testing.assert_array_equal(kei, BASE_KEI)
    np.testing.assert_array_equal(kef[:, 0], BASE_KEF)
    assert ref["margin"].tolist() == [0.0, 6.0, np.inf]
    assert not ref["margin"][0] > ref["margin_bound"][0] and ref["margin"][1] > ref["margin_bound"][1]


def test_small_lp_with_incumbent_and_near_zero_direction():
    snap = small_lp(**INCUMBENT)
    ref = R.restate(snap)
    v, k = ref["inputs"][3], ref["inputs"][4]
    np.testing.assert_array_equal(v[:, 12:], INC_V12)
    np.testing.assert_array_equal(k[:, 4], INC_K4)
    # a direction almost orthogonal to A: |d| = 1e-9 <= sum_epsilon, whatever its sign
    for sign in (1.0, -1.0):
        snap = small_lp(col_primal=[2.0, 0.5, 0.25, 2.0 + sign * 1e-9 / 3], col_primal_avg=[0.0] * 4)
        assert R.restate(snap)["inputs"][4][1, 4] == NEAR_ZERO_K14
    # a cutoff distance beyond infinity is capped; obj_norm <= 0 counts as 1
    assert R.restate(small_lp(**CAPPED))["inputs"][4][1, 4] == CAPPED_K14
    assert R.restate(small_lp(col_obj=[0.0] * 4))["inputs"][3][:, 4].tolist() == [0.0] * 4
    assert small_lp(col_obj=[0.0] * 4).scalars()[3] == 1.0 and small_lp(obj_norm=-2.0).scalars()[3] == 1.0


def test_new_hand_cases():
    """(a) incumbent == LP solution, (b) a zero-norm cut, (c) sides and bounds at +-infinity exactly and beyond: derived above."""
    ref = R.restate(small_lp(**SAME_POINT))
    np.testing.assert_array_equal(ref["inputs"][3][:, 12:], SAME_POINT_V12)
    np.testing.assert_array_equal(ref["inputs"][4][:, 4], SAME_POINT_K4)
    assert ref["cut_index"].tolist() == BASE_INDEX
    ref = R.restate(small_lp(**ZERO_CUT))
    assert ref["cut_index"].tolist() == ZERO_CUT_INDEX and ref["side_lhs"].tolist() == ZERO_CUT_SIDE_LHS
    np.testing.assert_array_equal(ref["inputs"][4], ZERO_CUT_K)
    np.testing.assert_array_equal(ref["inputs"][5], ZERO_CUT_KEI)
    np.testing.assert_array_equal(ref["inputs"][6][:, 0], ZERO_CUT_KEF)
    assert ref["inputs"][4][1, 3] == 1.0 and ref["inputs"][4][1, 5] == 0.0          # efficacy = -feasibility, parallelism 0
    snap = small_lp(**AT_INFINITY)
    ref = R.restate(snap)
    assert (ref["dims"]["n_state_rows"], ref["dims"]["n_state_edges"]) == (5, 8) and ref["inputs"][7] == 5
    np.testing.assert_array_equal(ref["inputs"][0], BASE_C)
    np.testing.assert_array_equal(ref["inputs"][3], BASE_V)                          # x1's bound 5e20: not finite, as 1e20 was
    np.testing.assert_array_equal(ref["inputs"][4], AT_INFINITY_K)
    assert ref["cut_index"].tolist() == BASE_INDEX and ref["margin"][2] == np.inf
    assert not lpstate.finite(np.array([1e5, -1e5, 5e20]), 1e5).any() and lpstate.finite(np.array([99999.0, -99999.0]), 1e5).all()


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases_whole_state(name):
    """Every variant's WHOLE state against the constants (the GPU test holds the device to the same ones), and the proof that its
    side choices are defined by exact arithmetic."""
    over, want = HAND[name]
    snap = small_lp(**over)
    ref = R.restate(snap)
    for got, w in zip(ref["inputs"][:7], want["arrays"]):
        assert got.dtype == w.dtype
        np.testing.assert_array_equal(got, w)
    np.testing.assert_array_equal(ref["cut_index"], want["cut_index"])
    lpcases.assert_sides_exact(snap)


@pytest.mark.parametrize("name", list(lpcases.SEAM))
def test_invariants_on_the_seam_cases(name):
    case = lpcases.SEAM[name]
    snap, ref = lpcases.snapshot(name), lpcases.reference(name)
    c, cei, cef, v, k, kei, kef, C, V, K = ref["inputs"]
    d = ref["dims"]
    assert (d["n_rows"], V, K) == (case["R"], case["V"], case["K"])
    assert (d["n_state_rows"], d["n_state_edges"]) == (C, cei.shape[1]) and (c.shape[0], v.shape[0], k.shape[0]) == (C, V, K)
    assert kei.shape[1] == d["cut_nnz"] and lpstate.state_key(d) == (C, V, K, cei.shape[1], kei.shape[1])
    for ei, n_left in ((cei, C), (kei, K)):
        key = ei[0].astype(np.int64) * V + ei[1]
        assert np.all(np.diff(key) > 0) and (ei.size == 0 or (0 <= ei.min() and ei[0].max() < n_left and ei[1].max() < V))
    assert sorted(ref["cut_index"].tolist()) == list(range(K))
    n_lhs = int(ref["side_lhs"].sum())
    assert ref["side_lhs"][ref["cut_index"][:n_lhs]].all() and not ref["side_lhs"][ref["cut_index"][n_lhs:]].any()
    assert np.all(np.diff(ref["cut_index"][:n_lhs]) > 0) and np.all(np.diff(ref["cut_index"][n_lhs:]) > 0)
    assert np.all(ref["margin"] > ref["margin_bound"])                         # no random case puts a side choice on its tie
    assert np.all(np.isfinite(k)) and np.all(np.isfinite(c)) and np.all(np.isfinite(v))
    lpcases.assert_seams(name, snap, ref)
    # whether the single call takes these sizes is the library's own statement, made without a device
    assert bool(lpstate.lp_layout(d)[1].call_supported) == case["single_call"]


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
