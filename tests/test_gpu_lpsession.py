"""The resident LP (`GCNN.open_lp`, csrc/k_lpres.hpp) on the GPU: every round of every session case of tests/lpsessioncases.py
against `state_from_lp` / `score_lp` / `select_cuts_lp` of the assembled snapshot, with `np.array_equal` -- a round's result is
those calls' result by definition, bit for bit.  No tolerance anywhere; the hand-worked cases are also held to the restatement
under the rule of tests/test_gpu_lpstate.py."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lpcases  # noqa: E402
import lpsessioncases as S  # noqa: E402
import lpstate_restate as R  # noqa: E402
import selcases  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate  # noqa: E402
from gcnn_cut_selector_amd.infer import LPSession  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401


@pytest.fixture(scope="module")
def model(dev):  # noqa: F811
    return make_model(93, dev)[0]


class GuardedSession(LPSession):
    GUARD = 256


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _check_round(model, sess, rnd, snap, states=True):
    """One round against the assembled snapshot: the state, the scores with both rankings' source, and a selection."""
    if states:
        want, want_index = model.state_from_lp(snap)
        got, got_index = sess.state(rnd)
        assert _same(got, want) and np.array_equal(got_index, want_index)
    q, q0 = sess.score(rnd, rank=True), model.score_lp(snap, rank=True)
    assert q.shape == q0.shape and np.array_equal(q.numpy(), q0.numpy(), equal_nan=True)
    assert np.array_equal(q.rankings, q0.rankings) and np.array_equal(q.cut_index, q0.cut_index)
    if q.shape[0] <= 4096:
        s, s0 = sess.select_cuts(rnd, max_selected=7), model.select_cuts_lp(snap, max_selected=7)
        assert np.array_equal(s.order, s0.order) and (s.n_kept, s.n_selected) == (s0.n_kept, s0.n_selected)
        assert np.array_equal(s.scores, s0.scores, equal_nan=True) and np.array_equal(s.cut_index, s0.cut_index)
    return q


def _play(model, steps, cls=LPSession, **kw):
    sess = None
    for step in steps:
        if step[0] == "open":
            sess = cls(model, step[1])
        elif step[0] == "append":
            before = sess.n_rows
            sess.append_rows(*step[1])
            assert sess.n_rows == before + np.asarray(step[1][3]).shape[0]
        else:
            _check_round(model, sess, step[1], step[2], **kw)
    return sess


@pytest.mark.parametrize("name", S.ROW_CASES)
def test_rows_of_every_kind_across_chunks(model, name):
    """Case 1: ranged, lhs-only, rhs-only, free and empty rows mixed, R at 255 / 256 / 257 / 600."""
    sess = _play(model, S.case(name))
    assert sess.n_rows == lpcases.SEAM[name]["R"] and sess.n_cols == lpcases.SEAM[name]["V"]
    sess.close()


def test_rounds_in_sequence_through_one_session(model):
    """Case 2: K = 600 -> 5 -> 0 -> 513 -> 1,100; K = 0 answers empty and leaves the session usable."""
    steps = S.case("k_sequence")
    sess = _play(model, steps, GuardedSession)
    assert sess.guards_intact()
    empty = steps[3]
    q = sess.score(empty[1], rank=True)
    assert q.shape == (0,) and q.rankings.shape == (0,) and q.cut_index.shape == (0,)
    s = sess.select_cuts(empty[1])
    assert (s.n_kept, s.n_selected) == (0, 0) and s.order.shape == (0,)
    _check_round(model, sess, steps[1][1], steps[1][2], states=False)


def test_appends(model):
    """Case 3: 3 rhs-only rows; 2 ranged and 1 lhs-only; none; R 255 -> 257 -- the next round equals the assembled snapshot."""
    sess = _play(model, S.case("appends"), GuardedSession)
    assert sess.n_rows == 257 and sess.guards_intact()


def test_none_keeps_the_last_value(model):
    """Case 4: col_ub flips has_ub, is left out, comes again; the incumbent arrays likewise; has_incumbent False -> True -> False."""
    _play(model, S.case("none_rules"))


@pytest.mark.parametrize("name", S.hand_names())
def test_hand_worked_cases(model, name):
    """Case 5: the `small_lp()` variants, against the assembled snapshot and against the restatement itself."""
    steps = S.case(name)
    sess = _play(model, steps)
    snap = steps[1][2]
    ref = R.restate(snap)
    got, index = sess.state(steps[1][1])
    R.compare(got, index, ref)


def test_more_columns_than_the_single_call_takes(model):
    """Case 6: V = 33,000 -- the session serves what gcnn_lp_infer declines; against state_from_lp + the general path."""
    steps = S.case("big_v")
    snap = steps[1][2]
    sess = LPSession(model, steps[0][1])
    want, want_index = model.state_from_lp(snap)
    got, index = sess.state(steps[1][1])
    assert _same(got, want) and np.array_equal(index, want_index)
    with torch.no_grad():
        general = model.call(want, False).numpy()
    q = sess.score(steps[1][1], rank=True)
    assert np.array_equal(q.numpy(), general) and np.array_equal(q.numpy(), model.score_state(want).numpy())
    s, s0 = sess.select_cuts(steps[1][1]), model.select_cuts_lp(snap)
    assert np.array_equal(s.order, s0.order) and s.n_kept == s0.n_kept and np.array_equal(s.scores, s0.scores)


def test_rejection_and_isolation(model):
    """Case 7: a cut column out of range (found by the device, deep=False), 4,097 cuts to select_cuts, then a good round that
    equals a fresh session's answer; guard bytes around the arena and the resident buffers stay intact."""
    base = lpcases.snapshot("rows257")
    rows, rnd = S.split(base)
    sess = GuardedSession(model, rows, deep=False)
    first = _check_round(model, sess, rnd, base)
    V = sess.n_cols
    ub_bad = np.where(np.arange(V) % 2 == 0, lpcases.INF, 3.0)
    bad = dataclasses.replace(rnd, cut_col=np.where(np.arange(rnd.cut_col.size) == 7, V + 5, rnd.cut_col), col_ub=ub_bad,
                              col_primal=np.asarray(rnd.col_primal) + 1.0)
    with pytest.raises(ValueError, match="outside"):
        sess.score(bad)
    many = lpcases.snapshot("cuts4097")
    wide = dataclasses.replace(rnd, **{n: getattr(many, n) for n in ("cut_ptr", "cut_col", "cut_val", "cut_lhs", "cut_rhs")})
    with pytest.raises(_lib.GcnnError, match="4097 cuts"):
        sess.select_cuts(wide)
    # the next round leaves col_ub and the incumbent to the session: it must see the accepted values, not the rejected round's
    kept = dataclasses.replace(rnd, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    again = sess.score(kept, rank=True)
    fresh = LPSession(model, rows, deep=False).score(rnd, rank=True)
    assert np.array_equal(again.numpy(), fresh.numpy()) and np.array_equal(again.numpy(), first.numpy())
    assert np.array_equal(again.rankings, fresh.rankings)
    got, index = sess.state(kept)
    want, want_index = model.state_from_lp(base)
    assert _same(got, want) and np.array_equal(index, want_index)
    assert sess.guards_intact()
    # host-side rejections enqueue nothing
    with pytest.raises(ValueError, match="row_dual"):
        sess.score(dataclasses.replace(rnd, row_dual=np.zeros(3)))
    _check_round(model, sess, rnd, base, states=False)
    sess.close()
    with pytest.raises(_lib.GcnnError, match="closed"):
        sess.score(rnd)


def test_parameters_are_read_per_round(model):
    """Case 8: score, perturb the flat parameters, score again: the second result is score_lp's under the new parameters."""
    base = lpcases.snapshot("cuts257")
    rows, rnd = S.split(base)
    sess = LPSession(model, rows)
    before = sess.score(rnd).numpy().copy()
    saved = model._flat.detach().clone()
    try:
        with torch.no_grad():
            model._flat.mul_(1.01)
        after = sess.score(rnd).numpy()
        assert np.array_equal(after, model.score_lp(base).numpy()) and not np.array_equal(after, before)
    finally:
        with torch.no_grad():
            model._flat.copy_(saved)
    assert np.array_equal(sess.score(rnd).numpy(), before)


@pytest.mark.parametrize("p_max,p_max_ub", [(0.1, 0.5), selcases.C_THR])
def test_selection_with_forced_rows(model, p_max, p_max_ub):
    """Case 9: forced rows, thresholds at the defaults and at selcases' tie thresholds, on the K = 513 round of case 2."""
    steps = S.case("k_sequence")
    rnd, snap = steps[4][1], steps[4][2]
    assert np.asarray(rnd.cut_lhs).shape[0] == 513
    sess = LPSession(model, steps[0][1])
    rng = np.random.default_rng(5)
    V = sess.n_cols
    cols = np.concatenate([np.sort(rng.choice(V, size=5, replace=False)) for _ in range(3)])
    forced = (np.stack([np.repeat([0, 1, 2], 5), cols]).astype(np.int32), rng.standard_normal(15).astype(np.float32), 3)
    for f in (None, forced):
        for cap in (None, 9):
            s = sess.select_cuts(rnd, f, p_max=p_max, p_max_ub=p_max_ub, max_selected=cap)
            s0 = model.select_cuts_lp(snap, f, p_max=p_max, p_max_ub=p_max_ub, max_selected=cap)
            assert np.array_equal(s.order, s0.order) and (s.n_kept, s.n_selected) == (s0.n_kept, s0.n_selected)
            assert np.array_equal(s.scores, s0.scores) and np.array_equal(s.cut_index, s0.cut_index)
            assert sorted(s.order.tolist()) == list(range(513))


def test_upload_and_launches_of_a_round(model):
    """A round uploads the snapshot minus the resident arrays and records its own two state launches in front of the forward's."""
    base = lpcases.snapshot("rows600")
    rows, rnd = S.split(base)
    sess = LPSession(model, rows)
    arrays, dims = lpstate.check_snapshot(base)
    _, full = lpstate.lp_layout(dims)
    resident = sum(arrays[i].nbytes for i in (0, 1, 2, 3, 4, 7, 8))
    assert sess.upload_bytes(rnd) <= full.in_bytes - resident + 256
    sess.score(rnd)
    with _lib.launch_profile() as prof:
        sess.score(rnd)
    names = [n for n, _ in prof.launches]
    batch = model.prepare(model.state_from_lp(base)[0])
    with torch.no_grad(), _lib.launch_profile() as general:
        model.call(batch, False)
    assert names[:2] == ["k_lpr_stats", "k_lpr_emit"] and names[2:] == [n for n, _ in general.launches], names
    assert len(names) == 9 and not [n for n in names if "iplan" in n or n.startswith("k_lp_")], names
