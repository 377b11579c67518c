"""tests/edgecases.py proved on the host: every case is what its id says, the restated walk visits every edge exactly once, the
integer expected values agree with a plain fp64 restatement of the operation, the planted pairs of the float fill bite, and a
restatement with one of the named defects changes an exact expected output on a named case."""
from fractions import Fraction

import numpy as np
import pytest

import edgecases as X


def _lens(c, by_left=True):
    return np.diff(c["l_ptr"] if by_left else c["v_ptr"])


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", X.IDS)
def test_every_edge_is_visited_exactly_once(cid):
    c = X.case(cid)
    for recv_is_left in (True, False):
        p = X.plans(c, recv_is_left)
        rptr, sptr = X.csr(c, recv_is_left)[0], X.csr(c, not recv_is_left)[0]
        for ptr, plan, u in ((rptr, p["fwd"], X.EDGE_U), (rptr, p["infer"], X.EDGE_U), (sptr, p["send"], X.EDGE_UB)):
            assert (X.multiplicity(ptr, plan, u) == 1).all(), (cid, recv_is_left, plan["name"])
            if plan["kind"] == "main":       # every work item by exactly one wave of one block on one trip
                nwork = X.cdiv(plan["n_own"], 4 // plan["slots"])
                assert np.array_equal(np.sort(X.main_items(plan)), np.arange(nwork)), (cid, plan["name"])


def test_the_walk_by_hand():
    off, full = X.walk(21, 1, 4)                 # G = 16, F = 4: four full steps, a chunk boundary, a full step, a masked step of one
    assert off.tolist() == list(range(21)) and full.tolist() == [True] * 20 + [False]
    off, full = X.walk(7, 2, 2)                  # B = 4: a full step and a masked step of three
    assert off.tolist() == list(range(7)) and full.tolist() == [True] * 4 + [False] * 3
    assert X.walk(5, 1, 4, "masked_drop_last")[0].tolist() == [0, 1, 2, 3] and X.walk(5, 1, 4, "slot_past_end")[0].tolist() == [0, 1, 2, 3, 4, 0]
    assert X.shares(33, 16)[:2] == [(0, 3), (3, 6)] and X.shares(33, 16)[10:12] == [(30, 33), (33, 33)]
    assert X.shares(33, 16, "share_overlap")[11] == (32, 33)
    assert [int(X.xcd_remap(b, 19)) for b in (0, 1, 8, 3, 11)] == [0, 3, 1, 9, 10]      # the remainder branch: 19 = 2 * 8 + 3


@pytest.mark.parametrize("cid", ("seams/S1", "long/S2", "block"))
@pytest.mark.parametrize("s1", X.S1)
def test_integer_expected_values_are_the_plain_operation(cid, s1):
    c, f = X.case(cid), X.grid_fill(cid)
    cc = (f["coef"].astype(np.float64) + X.E_SHIFT) * X.E_SCALE
    J = f["PL"].astype(np.float64)[c["el"]] + cc[:, None] * f["w"].astype(np.float64)[None, :] + f["PR"].astype(np.float64)[c["ev"]]
    act = s1 * J > 0
    for recv_is_left in (True, False):
        recv, send = (c["el"], c["ev"]) if recv_is_left else (c["ev"], c["el"])
        n_recv, n_send = (c["n_left"], c["n_var"]) if recv_is_left else (c["n_var"], c["n_left"])
        dS = (f["dS_l"] if recv_is_left else f["dS_v"]).astype(np.float64)
        S, N, T = np.zeros((n_recv, 64)), np.zeros((n_recv, 64)), np.zeros((n_send, 64))
        np.add.at(S, recv, np.maximum(s1 * J, 0))
        np.add.at(N, recv, act)
        np.add.at(T, send, s1 * act * dS[recv])
        got = X.expected(cid, s1, recv_is_left)
        assert np.array_equal(got["S"], S) and np.array_equal(got["N"], N) and np.array_equal(got["d_recv"], s1 * dS * N)
        assert np.array_equal(got["d_send"], T) and np.array_equal(got["d_w"], (s1 * act * dS[recv] * cc[:, None]).sum(0))
        assert np.array_equal(got["dw_main"] + got["dw_tail"], got["d_w"])


# ---- each case is what its id says --------------------------------------------------------------------------------------------------
def _kinds(c, unroll):
    """{("full" | "masked", "main" | "long" | "block")} over the forced ties of the pass that walks the left rows."""
    return {X.classify(c, int(e), unroll) for e in c["ties"]}


@pytest.mark.parametrize("cid", X.IDS)
def test_forced_and_natural_ties(cid):
    c, f = X.case(cid), X.grid_fill(cid)
    t = c["ties"]
    J8 = f["c2"][t, None] * f["w4"][None, :] + 8 * (f["PL"][c["el"][t]] + f["PR"][c["ev"][t]])
    assert t.size >= 8 and (J8 == 0).all()
    zeros = np.concatenate([f["PL"][c["el"][t]], f["PR"][c["ev"][t]]])
    assert (np.signbit(zeros) & (zeros == 0)).any() and (~np.signbit(zeros) & (zeros == 0)).any()      # zeros of both signs
    both = np.signbit(f["PL"][c["el"][t], 5]) & np.signbit(f["PR"][c["ev"][t], 5])
    assert both.any(), "no tie with p_own = p_oth = -0"
    has_long = bool((X.row_paths(_lens(c), X.left_plan(c, X.EDGE_U))[0] == X.LONG).any())
    for unroll in (X.EDGE_U, X.EDGE_UB):
        kinds = _kinds(c, unroll)
        assert {k for k, _ in kinds} == {"full", "masked"}, (cid, unroll, kinds)
        assert not has_long or any(p == "long" for _, p in kinds), (cid, unroll, kinds)
    assert has_long == (cid.split("/")[0] == "finder2" or "long" in cid)
    if cid.startswith("seams"):            # ties by themselves, on the edges that are not forced: a few per cent of the elements
        e = np.setdiff1d(np.arange(min(c["el"].size, 1 << 16)), t)
        J = f["c2"][e, None] * f["w4"][None, :] + 8 * (f["PL"][c["el"][e]] + f["PR"][c["ev"][e]])
        assert 0.01 < (J == 0).mean() < 0.06


@pytest.mark.parametrize("S", (1, 2, 4))
@pytest.mark.parametrize("asc", (False, True))
def test_seam_cases(S, asc):
    c = X.case(f"seams/S{S}" + ("/asc" if asc else ""))
    lens, G, F, B, T = _lens(c), 16 * S, 4 * S, 2 * S, 32 * S
    craft = lens[c["rows"] == "craft"]
    assert set(range(0, 2 * G + 1)) <= set(craft.tolist())
    fwd, send = X.left_plan(c, X.EDGE_U), X.left_plan(c, X.EDGE_UB)
    assert (fwd["name"], send["name"]) == ("k_edge_fwd<count>", "k_edge_bwd_send") and fwd["slots"] == send["slots"] == S
    assert fwd["grid"] % 8 != 0 and fwd["grid"] == send["grid"] < X.EDGE_MAX_GRID
    if S < 4:
        assert lens.max() == T and {T - 1, T} <= set(craft.tolist()) and c["n_left"] % (4 // S) != 0
    else:
        assert c["n_left"] > X.BLOCK_MAX_OWN and fwd["kind"] == "main" and {2 * G + 1, 256, 257, 493, 1000, 2049} <= set(craft.tolist())
    for step in (F, B):                     # a full step alone, a masked step alone, both, and a chunk boundary with both behind it
        assert {step - 1, step, step + 1, G, G + 1, G + step + 1} <= set(craft.tolist())
    if asc:
        assert (np.diff(lens) >= 0).all()
    elif S < 4:                             # the lane groups of one wave hold different lengths
        rpw = 4 // S
        items = lens[: lens.size // rpw * rpw].reshape(-1, rpw)
        assert (items.max(1) != items.min(1)).mean() > 0.5


@pytest.mark.parametrize("S", (1, 2))
def test_long_cases(S):
    c = X.case(f"long/S{S}")
    lens, T = _lens(c), 32 * S
    assert set(X.seam_lengths(S)) <= set(lens.tolist()) and set(X.long_lengths(S)) <= set(lens.tolist())
    assert X.long_lengths(S)[:3] == [T + 1, T + 2, 2 * T]
    fwd, send = X.left_plan(c, X.EDGE_U), X.left_plan(c, X.EDGE_UB)
    assert (fwd["name"], send["name"]) == ("k_edge_fwd<count> + long segments", "k_edge_bwd_send + long segments")
    assert fwd["slots"] == send["slots"] == S and fwd["lb"] == send["lb"] == X.long_grid(c["n_left"]) and fwd["lb"] % 8 == 0
    rows = np.flatnonzero(lens > T)
    assert rows.size == 9 and rows[0] == 0 and rows[-1] == c["n_left"] - 1 and (np.diff(rows[1:-1]) == 1).all()
    assert 0 < rows[1] and rows[-2] < c["n_left"] - 1
    path, _ = X.row_paths(lens, fwd)
    assert (path[rows] == X.LONG).all() and (np.delete(path, rows) == X.MAIN).all()
    if S == 1:       # T + 1 edges over 16 lane groups: a share of 3 and five empty trailing groups
        sh = X.shares(T + 1, 256 // (16 * S))
        assert sh[0] == (0, 3) and [e - b for b, e in sh][11:] == [0] * 5


@pytest.mark.parametrize("S", (1, 2))
@pytest.mark.parametrize("base", ("seams", "long"))
def test_unknown_cases_are_the_known_graphs(S, base):
    c, k = X.case(f"unknown/{base}/S{S}"), X.case(f"{base}/S{S}")
    for name in ("el", "ev", "l_ptr", "v_ptr", "pv", "ties", "pair_l", "pair_v"):
        assert np.array_equal(c[name], k[name]), name
    for name in ("coef", "w", "PL", "PR", "dS_l", "dS_v"):
        assert np.array_equal(X.grid_fill(c["id"])[name], X.grid_fill(k["id"])[name]), name
    assert X.max_degs(c) == (0, 0) and not c["known"] and k["known"]
    for recv_is_left in (True, False):
        p = X.plans(c, recv_is_left)
        assert p["fwd"]["lb"] > 0 and p["send"]["lb"] > 0 and p["fwd"]["name"].endswith("+ long segments") and p["send"]["name"].endswith("+ long segments")
        assert np.array_equal(X.expected(c["id"], 0.5, recv_is_left)["d_w"], X.expected(k["id"], 0.5, recv_is_left)["d_w"])


def test_block_case():
    c = X.case("block")
    lens = _lens(c)
    assert c["n_left"] <= X.BLOCK_MAX_OWN and c["el"].size >= X.BLOCK_DEG * c["n_left"]
    assert {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097} <= set(lens[c["rows"] == "craft"].tolist())
    p = X.plans(c, True)
    assert (p["fwd"]["kind"], p["fwd"]["name"], p["infer"]["name"]) == ("block", "k_edge_fwd_block<count>", "k_edge_fwd_block")
    assert [e - b for b, e in X.shares(4097, 4)] == [1025, 1025, 1025, 1022] and [e - b for b, e in X.shares(1, 4)] == [1, 0, 0, 0]


@pytest.mark.parametrize("S,n", ((1, 131072 + 37), (2, 65536 + 37), (4, 32768 + 37)))
def test_trip_cases(S, n):
    c = X.case(f"trip/S{S}")
    lens, G, F = _lens(c), 16 * S, 4 * S
    assert c["n_left"] == n and c["n_var"] <= 512
    fill = lens[c["rows"] == "fill"]
    assert set(fill.tolist()) == {X.TRIP_FILL[S], X.TRIP_FILL[S] + 1}       # the bottom of the class
    for unroll in (X.EDGE_U, X.EDGE_UB):
        plan = X.left_plan(c, unroll)
        assert plan["slots"] == S and plan["grid"] == X.EDGE_MAX_GRID and plan["lb"] == 0 and "long" not in plan["name"]
        path, trip = X.row_paths(lens, plan)
        assert (path == X.MAIN).all() and trip.max() == 1 and (trip == 1).sum() == 37
        assert {0, 1, F - 1, F, F + 1, G - 1, G, G + 1, 2 * G} <= set(lens[(trip == 1) & (c["rows"] == "craft")].tolist())
        assert X.main_items(plan, "one_trip").size == 4 * X.EDGE_MAX_GRID < X.main_items(plan).size
    assert S == 4 or n % (4 // S) == 1       # a partial last item


def test_finder2_case():
    c = X.case("finder2/S1")
    lens = _lens(c)
    n = X.LONG_NT * X.MAX_GRID + 512
    assert c["n_left"] == n == 524288 + 512
    assert (lens[5], lens[524288 + 7], lens[n - 1]) == (33, 100, 493) and (lens > 32).sum() == 3 and (np.delete(lens, [5, 11, 524288 + 7, 524288 + 30, n - 1]) == 1).all()
    for unroll in (X.EDGE_U, X.EDGE_UB):
        plan = X.left_plan(c, unroll)
        assert plan["slots"] == 1 and plan["lb"] == X.MAX_GRID and plan["name"].endswith("+ long segments")
        path, rnd = X.row_paths(lens, plan)
        assert np.flatnonzero(path == X.LONG).tolist() == [5, 524288 + 7, n - 1] and rnd[[5, 524288 + 7, n - 1]].tolist() == [0, 1, 1]
    assert [e - b for b, e in X.shares(33, 16)][10:] == [3] + [0] * 5


def test_scatter_cases():
    lens, idx, msg, _ = X.scatter_case("lens")
    assert set(X.SCATTER_LENS) == set(lens.tolist()) and 64 == X.SEG_U * X.SEG_SLOTS and X.seg_trips(lens.size) == 1
    lens, idx, msg, _ = X.scatter_case("trip")
    assert lens.size == 32768 + 5 and X.seg_trips(lens.size) == 2 and lens[-5:].tolist() == [0, 1, 5, 65, 129]
    assert np.abs(msg).max() * lens.max() < 1 << 24 and np.array_equal(msg, np.round(msg))
    want = np.zeros((lens.size, 64))
    np.add.at(want, idx, msg.astype(np.float64))
    assert np.array_equal(X.scatter_expected("trip"), want)


# ---- the planted pairs --------------------------------------------------------------------------------------------------------------
def test_round_f32_rounds_once_to_nearest_even():
    one, ulp = Fraction(1), Fraction(1, 1 << 23)
    assert X.round_f32(one + ulp / 2) == 1.0 and X.round_f32(one + 3 * ulp / 2) == float(one + 2 * ulp)      # ties to even
    assert X.round_f32(one + ulp / 2 + Fraction(1, 1 << 80)) == float(one + ulp)       # where fp64 first, then fp32, would give 1.0
    assert X.round_f32(-(one + ulp / 2 + Fraction(1, 1 << 80))) == -float(one + ulp)
    assert X.round_f32(Fraction(1, 1 << 149) * Fraction(3, 2)) == float(Fraction(1, 1 << 148)) and X.round_f32(Fraction(0)) == 0.0
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(500).astype(np.float32), rng.standard_normal(500).astype(np.float32)
    assert np.array_equal(X.fma_f32(a, b, np.float32(0)), a * b) and np.array_equal(X.fma_f32(a, np.float32(1), b), a + b)


@pytest.mark.parametrize("recv_is_left", (True, False))
def test_planted_pairs_bite(recv_is_left):
    """On the 256 x 64 planted elements the kernels' expression fma(c, w, P_send) + P_recv is exactly 0.  Restated with an unfused
    multiply, then add, a share of them is not, and its sign makes the element active for one sign of s1 in the forward and not in
    the backward pass (or the other way round).  Measured over the 16,384 elements of seams/S1 (recv_is_left True / False): the
    unfused defect leaves 0.135 / 0.133 of them active for s1 > 0 (0.264 / 0.261 non-zero); regrouped as fma(c, w, P_send + P_recv)
    0.493 / 0.496 are active.  The floor asserted for the unfused defect is 0.05, under half of what was measured."""
    c, f = X.case("seams/S1"), X.float_fill("seams/S1", recv_is_left)
    pl, pv = c["pair_l"], c["pair_v"]
    assert pl.size == 256 and (np.diff(c["l_ptr"])[pl] == 1).all() and (np.diff(c["v_ptr"])[pv] == 1).all()
    assert np.array_equal(c["ev"][c["l_ptr"][pl]], pv)
    cw = X.prenorm_c(f["coef"][c["l_ptr"][pl]])[:, None]
    p_recv, p_send = (f["PL"][pl], f["PR"][pv]) if recv_is_left else (f["PR"][pv], f["PL"][pl])
    w = f["w"][None, :]
    assert (X.fma_f32(cw, w, p_send) + p_recv == 0).all()
    unfused = (cw * w + p_send) + p_recv                       # numpy fp32: two roundings
    regrouped = X.fma_f32(cw, w, p_send + p_recv)
    shares = [float((j > 0).mean()) for j in (unfused, regrouped)]
    print(f"\nplanted pairs, recv_is_left={recv_is_left}: active for s1 > 0 unfused {shares[0]:.3f} (non-zero {float((unfused != 0).mean()):.3f}), regrouped {shares[1]:.3f}")
    assert shares[0] >= 0.05


# ---- named defects -------------------------------------------------------------------------------------------------------------------
# defect: (case, s1, recv_is_left, outputs that must change, outputs that must not)
NAMED = {
    "masked_drop_last": [("seams/S1", 0.5, True, ("S", "N"), ()), ("seams/S2", 0.5, False, ("d_send", "d_w"), ()), ("block", 0.5, True, ("S", "N"), ())],
    "slot_past_end": [("seams/S2", 0.5, True, ("S", "N"), ()), ("seams/S4", -0.5, False, ("d_send", "d_w"), ())],
    "thresh_lt": [("seams/S1", 0.5, True, ("S", "N"), ()), ("seams/S2", -0.5, False, ("d_send", "d_w"), ())],
    "tie_active": [("seams/S1", 0.5, True, ("N", "d_recv", "d_send", "d_w"), ("S",)), ("seams/S1", -0.5, False, ("N", "d_send"), ("S",))],
    "neg_max": [("seams/S1", -0.5, True, ("S", "N", "d_send", "d_w"), ())],
    "share_overlap": [("long/S1", 0.5, True, ("S", "N"), ()), ("long/S1", 0.5, False, ("d_send", "d_w"), ())],
    "one_trip": [("trip/S1", 0.5, True, ("S", "N"), ()), ("trip/S1", 0.5, False, ("d_send", "d_w"), ())],
    "one_round": [("finder2/S1", 0.5, True, ("S", "N"), ()), ("finder2/S1", -0.5, False, ("d_send", "d_w"), ())],
    "long_dw_left_out": [("long/S1", 0.5, False, ("d_w",), ("S", "N", "d_send")), ("unknown/long/S2", -0.5, False, ("d_w",), ("d_send",))],
}


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_named_defect_changes_an_exact_expected_output(defect):
    assert set(NAMED) == set(X.DEFECTS)
    for cid, s1, recv_is_left, changed, same in NAMED[defect]:
        good, bad = X.expected(cid, s1, recv_is_left), X.expected(cid, s1, recv_is_left, defect)
        for k in changed:
            assert not np.array_equal(good[k], bad[k]), (defect, cid, k)
        for k in same:
            assert np.array_equal(good[k], bad[k]), (defect, cid, k)


def test_defects_hit_the_rows_they_are_named_for():
    c = X.case("seams/S1")
    lens = _lens(c)
    good, bad = X.expected("seams/S1", 0.5, True), X.expected("seams/S1", 0.5, True, "thresh_lt")
    rows = np.flatnonzero((good["N"] != bad["N"]).any(1))
    assert rows.size and (lens[rows] == 32).all()               # only T-rows, skipped by both sides
    bad = X.expected("seams/S1", 0.5, True, "masked_drop_last")
    rows = np.flatnonzero((good["N"] != bad["N"]).any(1))
    assert rows.size and (lens[rows] % 4 != 0).all()            # only rows that end in a masked step
    c = X.case("trip/S1")
    good, bad = X.expected("trip/S1", 0.5, True), X.expected("trip/S1", 0.5, True, "one_trip")
    rows = np.flatnonzero((good["N"] != bad["N"]).any(1))
    assert rows.size and rows.min() >= 131072 and (bad["N"][131072:] == 0).all()
