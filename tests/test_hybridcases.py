"""Host proofs for the cases of tests/hybridcases.py: before the device sees a case, it is shown here that the case discriminates --
that its integers are decided far from every tie (random, seams), or that each way of getting the semantics wrong that
tests/hybrid_restate.py restates as a variant changes a planted bit (exact cases): a fused last step, the other association of
the integer-support term, float32 keys, ties in the LP path's state order."""
import numpy as np
import pytest

import hybrid_restate as H
import hybridcases as X
from gcnn_cut_selector_amd import lpstate

# A consulted parallelism must stay this far from a threshold.  The issue's 1e-9 covers a float64 sum taken in another order; a row
# entry whose float32 rounding falls the other way on the device (its norm may differ in the last bit) moves P by up to 2^-24, so
# the cases are held to 1e-6, which they clear by more than an order of magnitude.
P_MARGIN = 1e-6


def _margins(key, snap):
    ref = X.reference(key, snap)
    order, n_kept, record = X.expected(key, snap)
    return ref, order, n_kept, H.margins(ref, record, 0.1, 0.5)


@pytest.mark.parametrize("problem,i", X.RANDOM)
def test_random_cases_are_decided_far_from_every_tie(problem, i):
    snap = X.random_case(problem, i)
    ref, order, n_kept, (gap, thr, par) = _margins(("random", problem, i), snap)
    K = ref["dims"]["n_cuts"]
    assert gap > 1e-9 and thr > 1e-9 and par > P_MARGIN, (gap, thr, par)
    assert ref["quality_bound"].max() < 1e-12
    assert 0 < n_kept < K                                      # the filter removes cuts: a ranking alone would not pass
    assert sorted(order.tolist()) == list(range(K))


@pytest.mark.parametrize("name", X.SEAMS)
def test_seam_cases_have_their_sizes_and_margins(name):
    snap = X.seam(name)
    ref, order, n_kept, (gap, thr, par) = _margins(("seam", name), snap)
    K, V = ref["dims"]["n_cuts"], ref["dims"]["n_cols"]
    if name.startswith("K"):
        assert K == int(name[1:])
    elif name.startswith("V"):
        assert V == int(name[1:]) and (V <= 257 or -(-V // 256) > 256)
    else:
        assert tuple(np.diff(snap.cut_ptr)[:8]) == X.CUT_LENGTHS
    assert gap > 0 and thr > 0 and par > P_MARGIN, (gap, thr, par)
    assert 0 < n_kept <= K and (n_kept < K or name == "V70000")     # (24 cuts over 70,000 columns hardly meet)


def test_limits_cases():
    assert lpstate.check_cut_snapshot(X.too_many())[1]["n_cuts"] == 4097
    assert lpstate.check_cut_snapshot(X.no_cuts())[1]["n_cuts"] == 0
    ref = H.restate(X.no_cuts())
    assert ref["quality"].shape == (0,) and H.select(ref["quality"], ref["rows"])[1] == 0


def test_an_lp_snapshot_and_its_cut_snapshot_restate_alike():
    snap = X.random_case("setcov", 0)
    arrays, dims = lpstate.check_cut_snapshot(snap)
    full, full_dims = lpstate.check_snapshot(snap)
    assert all(np.array_equal(a, full[i]) for a, i in zip(arrays, (16, 17, 18, 19, 20, 7, 8, 12)))
    assert (dims["n_cols"], dims["n_cuts"], dims["cut_nnz"]) == (full_dims["n_cols"], full_dims["n_cuts"], full_dims["cut_nnz"])
    cut = lpstate.CutSnapshot(*arrays, infinity=snap.infinity)
    assert np.array_equal(H.restate(cut)["quality"], H.restate(snap)["quality"])
    for field, bad, text, deep in (("cut_col", lambda a: np.where(np.arange(a.size) == 3, dims["n_cols"], a), "outside", True),
                                   ("cut_ptr", lambda a: np.concatenate([a[:1], a[:1], a[2:]]), "at least one entry", False),
                                   ("col_type", lambda a: a + 4, "codes", False), ("col_lp", lambda a: a[:-1], "vector", False)):
        broken = lpstate.CutSnapshot(*arrays, infinity=snap.infinity)
        setattr(broken, field, bad(getattr(broken, field)))
        with pytest.raises(ValueError, match=text):
            lpstate.check_cut_snapshot(broken, deep)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def test_plants_are_exact_and_every_variant_fails_one():
    snap, where = X.plants()
    ref = X.reference(("plants",), snap)
    eff, par, q = ref["features"][:, 0], ref["features"][:, 2], ref["quality"]
    # the sums are exact: integers and k/64, perfect-square norms
    assert np.array_equal(ref["norm"], np.round(ref["norm"])) and set(ref["norm"]) == {1.0, 3.0, 4.0, 5.0}
    # fused last step: efficacy i/64, parallelism 7/8 -- eight planted cuts, each differs in its last bit
    fused = H.quality_fused(eff, ref["nint"], ref["nnz"], par)
    for i, k in zip(X.FUSED_I, where["fused"]):
        assert eff[k] == i / 64 and par[k] == 0.875 and ref["nint"][k] == 0
        assert q[k] == i / 64 + 0.1 * 0.875 and fused[k] != q[k], (i, q[k], fused[k])
    # the other association of the integer-support term
    other = H.quality_other_assoc(eff, ref["nint"], ref["nnz"], par)
    for j, ((nint, nnz), k) in enumerate(where["int"].items()):
        assert (ref["nint"][k], ref["nnz"][k], par[k], eff[k]) == (nint, nnz, 0.0, (j + 2) / 1024)
        assert (0.1 * nint) / nnz != 0.1 * (nint / nnz) and other[k] != q[k], (nint, nnz)
    # single-entry cuts: the quality is col_lp itself
    lo, hi = where["neighbours"]
    assert q[lo] == snap.col_lp[48] and q[hi] == np.nextafter(q[lo], 1.0) and lo < hi
    a, b = where["sides"]
    assert q[a] == q[b] == 0.71 and a < b and ref["state_rank"][b] < ref["state_rank"][a]
    order, n_kept, _ = X.expected(("plants",), snap)
    rank = order.tolist()
    assert rank.index(hi) < rank.index(lo) and rank.index(a) < rank.index(b) and 0 < n_kept < q.size
    # float32 keys: the neighbours tie and swap; state-order ties: the lhs-sided cut comes first
    o32, _, _ = X.expected(("plants",), snap, key=np.float32)
    assert np.float32(q[lo]) == np.float32(q[hi]) and o32.tolist().index(lo) < o32.tolist().index(hi) and not np.array_equal(o32, order)
    ost, _, _ = X.expected(("plants",), snap, tie_rank=ref["state_rank"])
    assert ost.tolist().index(b) < ost.tolist().index(a) and not np.array_equal(ost, order)
    # and a wrong quality changes what is compared: the planted bits are among the outputs
    assert not np.array_equal(fused, q) and not np.array_equal(other, q)


@pytest.mark.parametrize("forced", (False, True))
@pytest.mark.parametrize("kind", X.TIE_KINDS)
def test_tie_cases_sit_exactly_on_the_thresholds(kind, forced):
    snap, f, want = X.tie(kind, forced)
    key = ("tie", kind, forced)
    ref = X.reference(key, snap)
    q0, t = 0.75, 0.9 * 0.75
    q3 = {"equal": t, "below": np.nextafter(t, 0.0), "f32up": X.F32_UP, "f32down": X.F32_DOWN}[kind]
    assert ref["quality"].tolist() == [q0, 0.1 * q0, t, q3, 0.95 * q0, 0.96 * q0]
    assert np.float32(X.F32_UP) == np.float32(0.675) and np.nextafter(np.float32(0.675), np.float32(0)) == np.float32(X.F32_DOWN)
    assert X.F32_DOWN < t < X.F32_UP
    col0 = ref["rows"][1:, 0]
    assert col0.tolist() == [0.25, 0.25 + 2.0 ** -20, 0.25 + 2.0 ** -20, 0.5, 0.5 + 2.0 ** -20]
    order, n_kept, record = X.expected(key, snap, f, *X.T_THR)
    assert (order.tolist(), n_kept) == want
    for p in (0.25, 0.25 + 2.0 ** -20, 0.5, 0.5 + 2.0 ** -20):
        assert (record["P"] == p).any(), p
    # float32 keys: one ulp below the float64 threshold is the float32 threshold itself -- partner 3 would stay
    o32, n32, _ = X.expected(key, snap, f, *X.T_THR, key=np.float32)
    if kind == "below":
        assert n32 == 5 and n_kept == 4
