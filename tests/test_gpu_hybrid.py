"""The hybrid selection from cut rows on the device (GPU): `HybridSelector` (gcnn_hybrid_select) against tests/hybrid_restate.py
on the cases of tests/hybridcases.py, which tests/test_hybridcases.py has shown on the host to discriminate.

  random   features and quality within each element's summation bound of the restatement; order and n_kept with `==` (the host
           proof puts every decision far from its tie), and n_kept < K in all sixteen, so a ranking alone does not pass.
  LP path  float32(features) equals `state_from_lp`'s cut_feats[:, (3, 2, 5)] bit for bit and the fp32 rows equal its
           cut_edge_feats up to sign: both paths run the same device functions on the same `make_lp_snapshot`.
  exact    quality, order and n_kept with `==`: every sum of these cases is exact in any order.
  batch    every member of a union has the bits of its solo call; a flagged member keeps to itself; a session can be reused.
  server   torch-free workers get the in-process call's bits: the quality does not depend on grouping, so no tolerance applies."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hybrid_restate as H  # noqa: E402
import hybridcases as X  # noqa: E402
import serve_worker_hybrid as W  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate, serve  # noqa: E402
from gcnn_cut_selector_amd.hybrid import HybridSelector  # noqa: E402

from gpucommon import PATTERN, dev, make_model  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sel(dev):  # noqa: F811
    return HybridSelector(dev)


@pytest.fixture(scope="module")
def model(dev):  # noqa: F811
    return make_model(94, dev)[0]


def _same(a, b):
    """Every output of two `SelectResult`s, bit for bit."""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) and np.asarray(x).dtype == np.asarray(y).dtype
               for x, y in ((a.scores, b.scores), (a.features, b.features), (a.order, b.order), (a.cut_index, b.cut_index))) \
        and (a.n_kept, a.n_selected) == (b.n_kept, b.n_selected)


def _check_against_restatement(res, case, snap):
    ref = X.reference(case, snap)
    K = ref["dims"]["n_cuts"]
    assert res.scores.dtype == np.float64 and res.features.shape == (K, 3) and np.array_equal(res.cut_index, np.arange(K))
    err_f = np.abs(res.features - ref["features"])
    err_q = np.abs(np.asarray(res.scores) - ref["quality"])
    print(case, "features: worst error / bound", float((err_f / np.maximum(ref["bounds"], 1e-300)).max()) if K else 0.0,
          "quality:", float((err_q / ref["quality_bound"]).max()) if K else 0.0)
    assert (err_f <= ref["bounds"]).all(), np.argwhere(err_f > ref["bounds"])[:5]
    assert (err_q <= ref["quality_bound"]).all(), np.argwhere(err_q > ref["quality_bound"])[:5]
    order, n_kept, _ = X.expected(case, snap)
    assert np.array_equal(res.order, order) and res.n_kept == n_kept
    return K, n_kept


@pytest.mark.parametrize("problem,i", X.RANDOM)
def test_random_cases_against_the_restatement(sel, problem, i):
    snap = X.random_case(problem, i)
    res = sel.select_cuts(snap)
    K, n_kept = _check_against_restatement(res, ("random", problem, i), snap)
    assert 0 < n_kept < K
    q = sel.quality(snap)
    assert np.array_equal(q, res.scores) and np.array_equal(q.features, res.features)


def _tie_to_lp_path(sel, model, snap):
    res = sel.select_cuts(snap)
    ptr, col, val = sel._sess().last_rows()
    state, cut_index = model.state_from_lp(snap)
    feats, kei, kef = state[4], state[5], state[6].reshape(-1)
    assert np.array_equal(res.features.astype(np.float32)[cut_index], feats[:, (3, 2, 5)])
    assert np.array_equal(ptr, snap.cut_ptr)
    seg = [np.arange(ptr[k], ptr[k + 1]) for k in cut_index]          # the LP path's edges: state order, input column order
    at = np.concatenate(seg) if seg else np.zeros(0, np.int64)
    assert np.array_equal(col[at], kei[1]) and np.array_equal(np.abs(val[at]), np.abs(kef))
    assert np.array_equal(kei[0], np.repeat(np.arange(len(seg)), [s.size for s in seg]))


@pytest.mark.parametrize("problem,i", X.RANDOM)
def test_random_cases_tie_to_the_lp_path(sel, model, problem, i):
    _tie_to_lp_path(sel, model, X.random_case(problem, i))


@pytest.mark.parametrize("name", X.SEAMS)
def test_seam_cases(sel, model, name):
    snap = X.seam(name)
    _check_against_restatement(sel.select_cuts(snap), ("seam", name), snap)
    _tie_to_lp_path(sel, model, snap)


def test_limits(sel):
    many = sel.select_cuts_many([X.no_cuts(), X.too_many(), X.seam("V255")], return_exceptions=True)
    assert many[0].n_kept == 0 and many[0].order.shape == (0,) and many[0].scores.shape == (0,) and many[0].features.shape == (0, 3)
    assert isinstance(many[1], _lib.GcnnError) and "4097 cuts" in str(many[1])
    assert _same(many[2], sel.select_cuts(X.seam("V255")))
    with pytest.raises(_lib.GcnnError):
        sel.select_cuts(X.too_many())
    q = sel.quality(X.too_many())                       # the quality alone has no limit
    ref = H.restate(X.too_many())
    assert (np.abs(q - ref["quality"]) <= ref["quality_bound"]).all()
    with pytest.raises(ValueError):
        sel.select_cuts(X.seam("V255"), p_max=float("nan"))


def test_exact_plants(sel):
    snap, where = X.plants()
    ref = X.reference(("plants",), snap)
    res = sel.select_cuts(snap)
    order, n_kept, _ = X.expected(("plants",), snap)
    assert np.array_equal(res.scores, ref["quality"]), np.flatnonzero(np.asarray(res.scores) != ref["quality"])
    assert np.array_equal(res.features, ref["features"])
    assert np.array_equal(res.order, order) and res.n_kept == n_kept


@pytest.mark.parametrize("forced", (False, True))
@pytest.mark.parametrize("kind", X.TIE_KINDS)
def test_exact_ties(sel, kind, forced):
    snap, f, want = X.tie(kind, forced)
    ref = X.reference(("tie", kind, forced), snap)
    res = sel.select_cuts(snap, f, p_max=X.T_THR[0], p_max_ub=X.T_THR[1])
    assert np.array_equal(res.scores, ref["quality"])
    assert (res.order.tolist(), res.n_kept) == want


def test_quality_and_rank_modes(sel):
    """The two shorter modes of the call: two launches for the quality, three for the ranking (no pair bits, n_kept = K)."""
    snaps = [X.random_case("setcov", 1), X.seam("K513"), X.plants()[0]]
    checked = [lpstate.check_cut_snapshot(s, deep=False) for s in snaps]
    sess = sel._sess()
    full = sess.run(checked, None, _lib.HYBRID_SELECT, 0.1, 0.5)
    for mode, names in ((_lib.HYBRID_QUALITY, ["k_hyb_stats", "k_hyb_emit"]), (_lib.HYBRID_RANK, ["k_hyb_stats", "k_hyb_emit", "k_hyb_filter"])):
        with _lib.launch_profile() as prof:
            got = sess.run(checked, None, mode)
        assert [n for n, _ in prof.launches] == names
        for g, f in zip(got, full):
            assert g[0] == "ok" and np.array_equal(g[1], f[1]) and np.array_equal(g[2], f[2])
            if mode == _lib.HYBRID_QUALITY:
                assert g[3] is None and g[4] is None
            else:
                assert np.array_equal(g[3], H.ranking(g[1])) and g[4] == g[1].size
    lo, hi = X.plants()[1]["neighbours"]
    rank = got[2][3].tolist()
    assert rank.index(hi) < rank.index(lo)              # neighbouring doubles: an fp64 key tells them apart


# ---- batch ------------------------------------------------------------------------------------------------------------------------
def _union():
    """The four shapes, a member without cuts, multi-chunk members that are not first, cut lengths around the lanes."""
    snaps = [X.random_case(p, 0) for p in X.PROBLEMS] + [X.no_cuts(), X.seam("K513"), X.seam("K257"), X.seam("lengths"), X.seam("V257")]
    rng = np.random.default_rng(5)
    forced = []
    for j, s in enumerate(snaps):
        V = s.col_type.shape[0]
        cols = np.sort(rng.choice(V, size=6, replace=False))
        forced.append(None if j % 3 == 0 else (np.stack([np.repeat([0, 1], 3), cols]).astype(np.int32),
                                               rng.standard_normal(6).astype(np.float32) * 0.5, 2))
    return snaps, forced


_solo = {}


def _solo_results(sel):
    """Every member of the union alone: computed once, shared, never written to."""
    if not _solo:
        snaps, forced = _union()
        _solo["r"] = [sel.select_cuts(s, f, max_selected=5) for s, f in zip(snaps, forced)]
    return _solo["r"]


def test_union_members_have_their_solo_bits(sel):
    snaps, forced = _union()
    solo = _solo_results(sel)
    calls = sel._sess().calls
    got = sel.select_cuts_many(snaps, forced, max_selected=5)
    assert sel._sess().calls == calls + 1
    assert all(_same(a, b) for a, b in zip(got, solo))
    back = sel.select_cuts_many(snaps[::-1], forced[::-1], max_selected=5)      # nor on its position
    assert all(_same(a, b) for a, b in zip(back[::-1], solo))
    with _lib.launch_profile() as prof:
        sel.select_cuts_many(snaps, forced, max_selected=5)
    assert [n for n, _ in prof.launches] == ["k_hyb_stats", "k_hyb_emit", "k_hyb_pairs", "k_hyb_filter"]


def test_a_flagged_member_moves_nobody_elses_bits(sel):
    snaps, forced = _union()
    solo = _solo_results(sel)
    bad = lpstate.CutSnapshot(**{n: getattr(snaps[1], n) for n, _ in lpstate.CUT_FIELDS}, infinity=snaps[1].infinity)
    bad.cut_col = bad.cut_col.copy()
    bad.cut_col[7] = bad.col_type.shape[0]                  # passes the cheap host check; the device flags it
    got = sel.select_cuts_many(snaps[:1] + [bad] + snaps[2:], forced, max_selected=5, return_exceptions=True)
    assert isinstance(got[1], ValueError) and "outside" in str(got[1])
    assert all(_same(a, b) for j, (a, b) in enumerate(zip(got, solo)) if j != 1)
    with pytest.raises(ValueError, match="outside"):
        sel.select_cuts(bad)


def test_a_session_is_reusable(dev):  # noqa: F811
    snaps, forced = _union()
    used, fresh = HybridSelector(dev), HybridSelector(dev)
    used.select_cuts_many(snaps, forced)
    small = [2, 6]
    a = used.select_cuts_many([snaps[j] for j in small], [forced[j] for j in small])
    b = fresh.select_cuts_many([snaps[j] for j in small], [forced[j] for j in small])
    assert all(_same(x, y) for x, y in zip(a, b))


def test_more_than_64_snapshots_take_several_calls(sel):
    snap = X.tie("below", False)[0]
    calls = sel._sess().calls
    got = sel.select_cuts_many([snap] * 70, p_max=X.T_THR[0], p_max_ub=X.T_THR[1])
    assert sel._sess().calls == calls + 2 and all(_same(g, got[0]) for g in got) and got[0].n_kept == 4


def test_the_call_stays_inside_its_arena(sel, dev):  # noqa: F811
    snaps, forced = _union()
    pick = [5, 0, 7]
    checked = [lpstate.check_cut_snapshot(snaps[j], deep=False) for j in pick]
    from gcnn_cut_selector_amd.infer import normalize_forced
    packed = [normalize_forced(forced[j], snaps[j].col_type.shape[0]) for j in pick]
    sess = sel._sess()
    want = sess.run(checked, packed, _lib.HYBRID_SELECT, 0.1, 0.5)
    need, guard = int(sess.last.arena_bytes), 4096
    block = torch.empty((need + 2 * guard + 256) // 4 + 1, dtype=torch.int32, device=dev)
    block.fill_(PATTERN)
    raw = block.view(torch.uint8)
    lead = (-raw.data_ptr()) % 256 + guard                  # (the guard is a multiple of 256: the arena stays aligned)
    arena = raw[lead:lead + need]
    assert need % 256 == 0 and arena.data_ptr() % 256 == 0
    got = sess.run(checked, packed, _lib.HYBRID_SELECT, 0.1, 0.5, arena=arena)
    for a, b in zip(got, want):
        assert a[0] == b[0] == "ok" and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4])) and a[4] == b[4]
    words = block.cpu().numpy()
    assert (words[:lead // 4] == PATTERN).all() and (words[(lead + need) // 4:] == PATTERN).all()
    assert (words[lead // 4:(lead + need) // 4] != PATTERN).any()
    with pytest.raises(_lib.GcnnError):
        sess.run(checked, packed, _lib.HYBRID_SELECT, 0.1, 0.5, arena=arena[:need - 256])


# ---- server -----------------------------------------------------------------------------------------------------------------------
N_WORKERS = 2


def test_server_with_hybrid_workers(sel, model, tmp_path):
    """Torch-free workers that open no GPU send hybrid requests with and without forced rows, and one bad snapshot each."""
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer({"m": model}, address).start()
    worker = os.path.join(ROOT, "tests", "serve_worker_hybrid.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), str(tmp_path / f"w{w}.npz")])
             for w in range(N_WORKERS)]
    try:
        codes = [p.wait(timeout=150) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * N_WORKERS
    assert server.stats["errors"] == N_WORKERS and server.stats["requests"] == N_WORKERS * (W.N_REQUESTS + 1)
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        for j in range(W.N_REQUESTS):
            snap, forced, (p_max, p_max_ub) = W.hybrid_request(w, j)
            direct = sel.select_cuts(snap, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=4)
            assert got[f"q{j}"].dtype == np.float64 and np.array_equal(got[f"q{j}"], direct.scores)
            assert np.array_equal(got[f"f{j}"], direct.features) and np.array_equal(got[f"o{j}"], direct.order)
            assert int(got[f"n{j}"]) == direct.n_kept and np.array_equal(got[f"i{j}"], direct.cut_index)
