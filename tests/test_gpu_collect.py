"""The data collector's expert round on the device (GPU): `Collector.collect_lp` (gcnn_lp_collect) on the cases of
tests/collectcases.py, which tests/test_collectcases.py has shown on the host to discriminate.  Everything is compared bit for bit:

  state, cut_index              `state_from_lp` of the same snapshot (gcnn_lp_state alone)
  hybrid_quality, features      `HybridSelector.quality` (gcnn_hybrid_select alone)
  improvements                  quality[cut_index]
  order, n_kept, n_selected     the restatement of tests/collectcases.py -- sound because the host proof holds every consulted
                                parallelism 1e-6 away from its thresholds, and the float64 keys and threshold are inputs, not results;
                                with quality := the hybrid quality, `HybridSelector.select_cuts` itself"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import collectcases as CC  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate  # noqa: E402
from gcnn_cut_selector_amd.collect import Collector  # noqa: E402
from gcnn_cut_selector_amd.hybrid import HybridSelector  # noqa: E402

from gpucommon import PATTERN, dev, make_model  # noqa: E402,F401

LAUNCHES = ["k_lp_stats", "k_lp_emit", "k_collect_stats", "k_collect_emit", "k_collect_pairs", "k_collect_filter"]


@pytest.fixture(scope="module")
def col(dev):  # noqa: F811
    return Collector(dev)


@pytest.fixture(scope="module")
def hyb(dev):  # noqa: F811
    return HybridSelector(dev)


_state = {}


def _state_of(col, K):
    """`state_from_lp` of a case's snapshot: computed once, shared, never written to."""
    if K not in _state:
        _state[K] = col.state_from_lp(CC.snapshot(K))
    return _state[K]


def _same_state(a, b):
    return len(a) == len(b) == 10 and a[7:] == b[7:] and all(
        x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:7], b[:7]))


def _check_fixed_part(res, col, hyb, K, q):
    """What does not depend on the quality's values: the state, cut_index, the labels' alignment, the hybrid outputs."""
    state, cut_index = _state_of(col, K)
    assert _same_state(res.state, state)
    assert res.cut_index.dtype == np.int32 and np.array_equal(res.cut_index, cut_index)
    assert res.improvements.dtype == np.float64 and np.array_equal(res.improvements, np.asarray(q, np.float64)[cut_index])
    hq = hyb.quality(CC.snapshot(K))
    assert res.hybrid_quality.dtype == np.float64 and np.array_equal(res.hybrid_quality, np.asarray(hq), equal_nan=True)
    assert res.features.shape == (K, 3) and np.array_equal(res.features, hq.features, equal_nan=True)
    assert res.order.dtype == np.int32 and sorted(res.order.tolist()) == list(range(K))


@pytest.mark.parametrize("case", CC.GPU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_cases_against_the_restatement(col, hyb, case):
    K, name, n_forced, p_max, p_max_ub = case
    q, forced = CC.quality(K, name), CC.forced_rows(K, n_forced)
    want = CC.restate(K, q, forced, p_max, p_max_ub, max_selected=7)
    res = col.collect_lp(CC.snapshot(K), q, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=7)
    print(case, "n_kept", res.n_kept, "of", K)
    _check_fixed_part(res, col, hyb, K, q)
    assert np.array_equal(res.cut_index, want["cut_index"])
    assert np.array_equal(res.order, want["order"]) and (res.n_kept, res.n_selected) == (want["n_kept"], want["n_selected"])
    assert res.n_selected == min(res.n_kept, 7)
    if name == "negative" and K >= 63:
        assert res.n_kept < K                      # every position is low: whatever is parallel to a kept cut goes


@pytest.mark.parametrize("K", CC.SIZES)
@pytest.mark.parametrize("n_forced", (0, 3))
def test_the_hybrid_quality_gives_the_hybrid_selection(col, hyb, K, n_forced):
    """The oracle the contract states: quality := HybridSelector.quality(snapshot) -> HybridSelector.select_cuts, bit for bit."""
    snap, forced = CC.snapshot(K), CC.forced_rows(K, n_forced)
    q = hyb.quality(snap)
    want = hyb.select_cuts(snap, forced, max_selected=5)
    res = col.collect_lp(snap, np.asarray(q), forced, max_selected=5)
    _check_fixed_part(res, col, hyb, K, q)
    assert np.array_equal(res.order, want.order) and (res.n_kept, res.n_selected) == (want.n_kept, want.n_selected)
    assert np.array_equal(res.hybrid_quality, want.scores) and np.array_equal(res.features, want.features)
    if K >= 63:
        assert res.n_kept < K


def test_max_selected(col):
    q = CC.quality(65, "spread")
    full = col.collect_lp(CC.snapshot(65), q)
    assert full.n_selected == full.n_kept > 3
    for m, want in ((3, 3), (0, 0), (1000, full.n_kept)):
        res = col.collect_lp(CC.snapshot(65), q, max_selected=m)
        assert res.n_selected == want and res.n_kept == full.n_kept and np.array_equal(res.order, full.order)


def test_the_model_without_a_model_builds_the_models_state(col, dev):  # noqa: F811
    """`Collector.state_from_lp` is `GCNN.state_from_lp`, and `GCNN.collect_lp` is `Collector.collect_lp`: no parameter is read."""
    model = make_model(94, dev)[0]
    for K in (65, 257):
        state, cut_index = model.state_from_lp(CC.snapshot(K))
        mine = _state_of(col, K)
        assert _same_state(mine[0], state) and np.array_equal(mine[1], cut_index)
    q = CC.quality(65, "ties")
    a, b = model.collect_lp(CC.snapshot(65), q, CC.forced_rows(65, 1), max_selected=4), col.collect_lp(CC.snapshot(65), q, CC.forced_rows(65, 1), max_selected=4)
    assert _same_state(a.state, b.state) and np.array_equal(a.order, b.order) and (a.n_kept, a.n_selected) == (b.n_kept, b.n_selected)
    assert np.array_equal(a.improvements, b.improvements) and np.array_equal(a.hybrid_quality, b.hybrid_quality)


def test_no_cuts(col):
    import hybridcases as X
    snap = X.no_cuts()
    res = col.collect_lp(snap, np.zeros(0))
    state, cut_index = col.state_from_lp(snap)
    assert _same_state(res.state, state) and res.cut_index.shape == (0,) and res.improvements.shape == (0,)
    assert res.order.shape == (0,) and (res.n_kept, res.n_selected) == (0, 0) and res.features.shape == (0, 3)


def test_too_many_cuts_are_refused_and_the_next_call_is_exact(col):
    q = CC.quality(64, "ties")
    before = col.collect_lp(CC.snapshot(64), q)
    calls = col._sess().calls
    with pytest.raises(_lib.GcnnError, match="4097 cuts"):
        col.collect_lp(CC.too_many(), np.zeros(4097))
    assert col._sess().calls == calls                                  # refused before anything was enqueued
    arrays, dims = lpstate.check_snapshot(CC.too_many(), deep=False)
    d, L = _lib.LpDims(**dims), _lib.LpCollectLayout()
    assert _lib.lib().gcnn_lp_collect_layout_for(C.byref(d), 0, 0, C.byref(L)) == -4
    after = col.collect_lp(CC.snapshot(64), q)
    assert _same_state(before.state, after.state) and np.array_equal(before.order, after.order) and before.n_kept == after.n_kept


def test_a_flagged_snapshot_raises_and_the_next_call_is_exact(col):
    snap, q = CC.snapshot(65), CC.quality(65, "spread")
    before = col.collect_lp(snap, q, CC.forced_rows(65, 1))
    for field, at, value, text in (("cut_col", 7, snap.col_type.shape[0], "outside"), ("row_col", 3, 10 ** 6, "outside"),
                                   ("cut_col", 1, int(snap.cut_col[0]), "increasing")):
        bad = lpstate.LPSnapshot(**{k: getattr(snap, k) for k in snap.__dataclass_fields__})
        a = getattr(bad, field).copy()
        a[at] = value                                                  # passes the cheap host check; the device flags it
        setattr(bad, field, a)
        with pytest.raises(ValueError, match=text):
            col.collect_lp(bad, q, CC.forced_rows(65, 1))
    after = col.collect_lp(snap, q, CC.forced_rows(65, 1))
    assert _same_state(before.state, after.state) and np.array_equal(before.order, after.order) and before.n_kept == after.n_kept
    assert np.array_equal(before.hybrid_quality, after.hybrid_quality) and np.array_equal(before.improvements, after.improvements)


def test_one_upload_six_launches_one_download(col):
    from gcnn_cut_selector_amd.infer import al16
    for K, n_forced in ((65, 3), (257, 0), (1, 1)):
        snap, q, forced = CC.snapshot(K), CC.quality(K, "ties"), CC.forced_rows(K, n_forced)
        timings = {}
        with _lib.launch_profile() as prof:
            col.collect_lp(snap, q, forced, timings=timings)
        names = [n for n, _ in prof.launches]
        assert len(names) <= 6 and names == LAUNCHES
        sess = col._sess()
        arrays, dims = lpstate.check_snapshot(snap, deep=False)
        nf, nfe = (0, 0) if forced is None else (forced[2], forced[1].size)
        _, lp = lpstate.lp_layout(dims, nf, nfe)
        L = sess.last
        assert sess.upload_bytes == lp.in_bytes + al16(8 * K) + L.table_bytes == timings["upload_bytes"]
        assert sess.download_bytes == L.out_bytes == timings["download_bytes"]
        assert set(timings) >= {"pack", "enqueue", "wait"} and all(timings[k] >= 0 for k in ("pack", "enqueue", "wait"))
        # the table the call wrote into the upload: one entry whose eight positions are the LP snapshot's own arrays
        table = sess.last_table().view(np.int32)
        head_words = 4 + 4 * _lib.IBATCH_TABLE_STRIDE
        assert table[0] == 1 and table.size * 4 == L.table_bytes
        pos = table[head_words:][:2 * 18].view(np.int64)
        assert pos[:8].tolist() == list(L.entry_snap) == [L.snap_off[i] for i in (17, 18, 19, 20, 21, 8, 9, 13)]
        assert (pos[8:12] >= L.hyb_scratch_off).all() and (pos[8:12] < L.arena_bytes).all()
        assert pos[12:14].tolist() == [L.out_dev_off + L.out_off[9], L.out_dev_off + L.out_off[10]]
        assert pos[14:17].tolist() == list(L.rows_off) and pos[17] == L.out_dev_off + L.out_off[13]


def test_the_call_stays_inside_its_arena(col, dev):  # noqa: F811
    from gcnn_cut_selector_amd.infer import normalize_forced
    K = 257
    snap, q = CC.snapshot(K), CC.quality(K, "spread")
    arrays, dims = lpstate.check_snapshot(snap, deep=False)
    packed = normalize_forced(CC.forced_rows(K, 3), dims["n_cols"])
    sess = col._sess()
    want = sess.run(arrays, dims, q, packed, 0.1, 0.5)
    need, guard = int(sess.last.arena_bytes), 4096
    block = torch.empty((need + 2 * guard + 256) // 4 + 1, dtype=torch.int32, device=dev)
    block.fill_(PATTERN)
    raw = block.view(torch.uint8)
    lead = (-raw.data_ptr()) % 256 + guard                  # (the guard is a multiple of 256: the arena stays aligned)
    arena = raw[lead:lead + need]
    assert need % 256 == 0 and arena.data_ptr() % 256 == 0
    got = sess.run(arrays, dims, q, packed, 0.1, 0.5, arena=arena)
    assert _same_state(got[0], want[0]) and all(np.array_equal(x, y) for x, y in zip(got[1:5], want[1:5])) and got[5] == want[5]
    words = block.cpu().numpy()
    assert (words[:lead // 4] == PATTERN).all() and (words[(lead + need) // 4:] == PATTERN).all()
    assert (words[lead // 4:(lead + need) // 4] != PATTERN).any()
    with pytest.raises(_lib.GcnnError):
        sess.run(arrays, dims, q, packed, 0.1, 0.5, arena=arena[:need - 256])
