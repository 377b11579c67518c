"""The state builder (csrc/k_lpstate.hpp: k_lp_stats, k_lp_emit) at chunk seams and degenerate values (GPU): every case of
tests/lpcases.py through `GCNN.state_from_lp`, `score_lp` and `select_cuts_lp` against the float64 restatement
tests/lpstate_restate.py, under the rule of tests/test_gpu_lpstate.py -- integers, flags and `cut_index` equal, continuous values
within one float32 ulp plus the element's derived fp64 summation bound; no tolerance of this file's own.

Seam cases (random, seeded): more than one 256-entry chunk of cuts, rows and columns with both sides in every chunk, more than 256
chunks of columns and of rows, lengths around the 16 lanes of a row, free and empty rows at chunk borders, K = 4,097.  Each asserts
that every side choice is further from its tie than the activity's summation bound.
Hand-made cases (`small_lp()` variants): the side tie, a zero-norm row and a zero-norm cut, d = 0 and |d| = 1e-9 of both signs, an
incumbent equal to the LP solution, the capped cutoff, a zero objective, sides and bounds at +-infinity exactly and beyond.  Their
tie is a tie: the test asserts that the side is defined by exact arithmetic (lpcases.assert_sides_exact) in place of the margin, and
holds the device to the constants worked out by hand in tests/test_lpstate_restate.py as well.  No case is skipped or filtered."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lpcases  # noqa: E402
import lpstate_restate as R  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate  # noqa: E402
from gcnn_cut_selector_amd.infer import _UseGeneralPath  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401
from test_gpu_lpstate import _GuardedSession, _same  # noqa: E402

HAND = lpcases.hand_cases()
NAMES = [f"hand-{n}" for n in HAND] + list(lpcases.SEAM)
LIMIT_RANK = LIMIT_SELECT = 4096                    # cuts the LP entry points rank / select on the device


@pytest.fixture(scope="module")
def model(dev):  # noqa: F811
    return make_model(91, dev)[0]


def _case(name):
    """(snapshot, restatement, hand constants | None, does gcnn_lp_infer take it)"""
    if name.startswith("hand-"):
        snap, want = HAND[name[5:]]
        return snap, R.restate(snap), want, True
    return lpcases.snapshot(name), lpcases.reference(name), None, lpcases.SEAM[name]["single_call"]


def _forced(V):
    """Two forced rows over distinct columns (three each where V allows)."""
    rng = np.random.default_rng(5)
    per = min(3, V // 2)
    cols = np.sort(rng.choice(V, size=2 * per, replace=False))
    return np.stack([np.repeat([0, 1], per), cols]).astype(np.int32), rng.standard_normal(2 * per).astype(np.float32), 2


def _outcome(call):
    try:
        return call()
    except Exception as exc:  # noqa: BLE001 -- the type is what is compared
        return exc


@pytest.mark.parametrize("name", NAMES)
def test_state_scores_and_selection_match(dev, model, name):  # noqa: F811
    snap, ref, hand, single_call = _case(name)
    if hand is None:
        assert np.all(ref["margin"] > ref["margin_bound"]), "a side choice sits on its tie: fix the case, not the test"
        lpcases.assert_seams(name, snap, ref)
    else:
        lpcases.assert_sides_exact(snap)            # the tie cases: the side is defined by exact arithmetic instead
    state, cut_index = model.state_from_lp(snap)
    worst = R.compare(state, cut_index, ref)
    print(f"{name}: dims {lpstate.state_key(ref['dims'])}, largest |difference| / tolerance = {worst:.3f}")
    if hand is not None:
        assert np.array_equal(cut_index, hand["cut_index"])
        for got, want in zip(state[:7], hand["arrays"]):
            assert got.dtype == want.dtype and got.shape == want.shape
            if want.dtype == np.int32:
                assert np.array_equal(got, want)
            else:
                gap = np.abs(got.astype(np.float64) - want.astype(np.float64))
                assert np.all(gap <= np.spacing(np.abs(want)).astype(np.float64)), (got, want)
    # two runs: the same bits
    again, index_again = model.state_from_lp(snap)
    assert _same(state, again) and np.array_equal(cut_index, index_again)

    V, K = state[8], state[9]
    sess = model._lp()
    if not single_call:
        with pytest.raises(_UseGeneralPath):
            sess.run(snap, False)
    if K > LIMIT_RANK:
        with pytest.raises(_UseGeneralPath):
            sess.run(snap, True)
    q = model.score_lp(snap, rank=True)
    q0 = model.score_state(state, rank=True)
    assert np.array_equal(q.numpy(), q0.numpy(), equal_nan=True) and np.array_equal(q.rankings, q0.rankings)
    assert np.array_equal(q.cut_index, ref["cut_index"]) and sorted(q.rankings.tolist()) == list(range(K))
    if single_call:
        model.score_lp(snap)                                          # (unranked: the single call at every K)
        assert _same(sess.last_state(), state[:7])                    # the state the single call built in its arena
    if single_call and K <= LIMIT_RANK:
        qd = model.score_lp(snap, rank="device")
        assert np.array_equal(qd.rankings, q0.rankings)
    for f in (None, _forced(V)):
        s = _outcome(lambda: model.select_cuts_lp(snap, f, p_max=0.1, p_max_ub=0.5, max_selected=5))
        s0 = _outcome(lambda: model.select_cuts(state, f, p_max=0.1, p_max_ub=0.5, max_selected=5))
        if K > LIMIT_SELECT:
            assert type(s) is type(s0) and isinstance(s, _lib.GcnnError)
            continue
        assert not isinstance(s, Exception) and not isinstance(s0, Exception), (s, s0)
        assert np.array_equal(s.order, s0.order) and (s.n_kept, s.n_selected) == (s0.n_kept, s0.n_selected)
        assert np.array_equal(s.scores, s0.scores, equal_nan=True) and np.array_equal(s.cut_index, ref["cut_index"])
        assert sorted(s.order.tolist()) == list(range(K))


@pytest.mark.parametrize("name", ["cuts513", "rows257"])
def test_nothing_is_written_outside_the_state(dev, model, name):  # noqa: F811
    """Several chunks of cuts / of rows in an arena exactly as large as the layout asks: the guard bytes around it and the padding
    between the state arrays inside it keep their fill, and the scores are those of the plain session."""
    snap, ref = lpcases.snapshot(name), lpcases.reference(name)
    good = model.score_lp(snap)
    plain, sess = model._lp_session, _GuardedSession(model)
    model._lp_session = sess
    try:
        q = model.score_lp(snap)
        s = model.select_cuts_lp(snap, _forced(ref["inputs"][8]))
        torch.cuda.synchronize()
        assert sess.guards_intact() and sess.interior_untouched()
        assert np.array_equal(q.numpy(), good.numpy(), equal_nan=True) and np.array_equal(s.cut_index, ref["cut_index"])
    finally:
        model._lp_session = plain
