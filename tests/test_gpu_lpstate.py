"""The state built on the device from a raw LP snapshot (GPU): `GCNN.state_from_lp`, `score_lp` and `select_cuts_lp` against the
float64 restatement tests/lpstate_restate.py.  Integer and flag outputs must be equal; continuous outputs must lie within one float32
ulp of the restatement's float32 value plus the element's summation bound (one final rounding plus fp64 reassociation: derived in
the restatement, not measured).  Every case asserts that each cut's side choice is further from its tie than the activity's
summation bound; no case is left out.

These ten cases come from `synthetic.make_lp_snapshot`: at most one chunk of cuts, no degenerate value, no free or empty row.
tests/test_gpu_lpstate_edges.py covers, under the same rule, several chunks of cuts / rows / columns with both sides in each, more
than 256 chunks of a kind, lengths around the 16 lanes of a row, free and empty rows, K = 4,097, and the hand-made degenerate cases
(side tie, zero norms, d = 0, incumbent = LP solution, capped cutoff, zero objective, sides at +-infinity).  Neither file checks the
three interpreted cut features against SCIP: both compare with this project's own restatement."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lpstate_restate as R  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.infer import _LPSession, _UseGeneralPath  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402
from test_lpstate_build import LP_NAMES  # noqa: E402

CASES = [(p, dict()) for p in synthetic.PROBLEMS] + [
    ("setcov", dict(scale=0.3, row_sides="rhs_only")),                       # no row with a finite lhs
    ("capfac", dict(scale=0.3, row_sides="ranged")),                         # every row twice
    ("indset", dict(scale=0.3, n_cuts=1)),                                   # K = 1
    ("combauc", dict(cut_sides="lhs")),                                      # every cut on its lhs side
    ("setcov", dict(scale=0.3, incumbent=False)),                            # no incumbent
    ("indset", dict(scale=0.3, extra_cols=33000)),                           # past gcnn_infer's variable limit: the fallback
]


@pytest.fixture(scope="module")
def model(dev):
    return make_model(91, dev)[0]


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("problem,kw", CASES, ids=[f"{p}-{'-'.join(f'{k}={v}' for k, v in kw.items()) or 'full'}" for p, kw in CASES])
def test_state_scores_and_selection_match(dev, model, problem, kw):
    snap = synthetic.make_lp_snapshot(problem, 3, **kw)
    ref = R.restate(snap)
    assert np.all(ref["margin"] > ref["margin_bound"]), "a side choice sits on its tie: fix the generator, not the test"
    state, cut_index = model.state_from_lp(snap)
    worst = R.compare(state, cut_index, ref)
    print(f"{problem} {kw}: dims {lpstate.state_key(ref['dims'])}, largest |difference| / tolerance = {worst:.3f}")
    if kw.get("row_sides") == "rhs_only":
        assert state[7] == ref["dims"]["n_rows"]
    if kw.get("row_sides") == "ranged":
        assert state[7] == 2 * ref["dims"]["n_rows"]
    if kw.get("cut_sides") == "lhs":
        assert ref["side_lhs"].all()
    # two runs: the same bits
    again, index_again = model.state_from_lp(snap)
    assert _same(state, again) and np.array_equal(cut_index, index_again)
    # the single call against score_state / select_cuts on that state: same arrays, same kernels, same bits
    sess = model._lp()
    past_limit = ref["dims"]["n_cols"] > 32768
    if past_limit:
        with pytest.raises(_UseGeneralPath):
            sess.run(snap, False)
    q = model.score_lp(snap, rank=True)
    q0 = model.score_state(state, rank=True)
    assert np.array_equal(q.numpy(), q0.numpy(), equal_nan=True) and np.array_equal(q.rankings, q0.rankings)
    assert np.array_equal(q.cut_index, ref["cut_index"])
    if not past_limit:
        assert _same(sess.last_state(), state[:7])                # the state the single call built in its arena
        qd = model.score_lp(snap, rank="device")
        assert np.array_equal(qd.rankings, q0.rankings)
    K, V = state[9], state[8]
    rng = np.random.default_rng(5)
    cols = np.sort(rng.choice(V, size=6, replace=False))
    forced = (np.stack([np.repeat([0, 1], 3), cols]).astype(np.int32), rng.standard_normal(6).astype(np.float32), 2)
    for f in (None, forced):
        s = model.select_cuts_lp(snap, f, p_max=0.1, p_max_ub=0.5, max_selected=5)
        s0 = model.select_cuts(state, f, p_max=0.1, p_max_ub=0.5, max_selected=5)
        assert np.array_equal(s.order, s0.order) and (s.n_kept, s.n_selected) == (s0.n_kept, s0.n_selected)
        assert np.array_equal(s.scores, s0.scores, equal_nan=True) and np.array_equal(s.cut_index, ref["cut_index"])
        assert sorted(s.order.tolist()) == list(range(K))


def test_fallback_state_equals_the_single_calls(dev, model):
    """gcnn_lp_state (what the fallback feeds to prepare + forward) and the single call build the same bits; and a snapshot
    the single call accepts scores the same through the fallback."""
    snap = synthetic.make_lp_snapshot("setcov", 5, scale=0.5)
    sess = model._lp()
    q = model.score_lp(snap)
    fast = sess.last_state()
    state, index = sess.build_state(snap)
    assert _same(fast, tuple(t.cpu().numpy() for t in state[:7]))
    with torch.no_grad():
        general = model.call(state, False).numpy()
    np.testing.assert_allclose(general, q.numpy(), rtol=1e-5, atol=1e-6)
    assert np.array_equal(index.cpu().numpy(), q.cut_index)


def test_launches_are_recorded_under_their_own_names(dev, model):
    snap = synthetic.make_lp_snapshot("combauc", 1)
    state, _ = model.state_from_lp(snap)
    model.score_lp(snap), model.score_state(state)
    with _lib.launch_profile() as lp:
        model.score_lp(snap)
    with _lib.launch_profile() as plain:
        model.score_state(state)
    names = [n for n, _ in lp.launches]
    assert names[:2] == ["k_lp_stats", "k_lp_emit"] and names[2:] == [n for n, _ in plain.launches]
    assert set(names[:2]) == LP_NAMES


class _GuardedSession(_LPSession):
    """The product session with an arena exactly as large as the layout asks and guard bytes on either side of it."""
    GUARD, BYTE = 256, 0xA5

    def _buffers(self, L):
        super()._buffers(L)                                   # staging buffers; the arena is replaced below
        raw = torch.full((L.arena_bytes + 2 * self.GUARD,), self.BYTE, dtype=torch.uint8, device=self.model.device)
        self._raw, self.arena = raw, raw[self.GUARD:self.GUARD + L.arena_bytes]

    def guards_intact(self):
        return bool((self._raw[:self.GUARD] == self.BYTE).all() and (self._raw[-self.GUARD:] == self.BYTE).all())

    def interior_untouched(self):
        """The arena's own layout: the seven state arrays sit between the plan's zero block and its by-variable arrays.  The words
        behind the last state array up to the next carved block must still hold the fill byte wherever padding exists."""
        L, (c, v, k, e1, e2) = self.last
        off, sizes = list(L.state.in_off), (16 * c, 8 * e1, 4 * e1, 56 * v, 24 * k, 8 * e2, 4 * e2)
        ends = [off[i + 1] + n for i, n in enumerate(sizes)]
        nexts = off[2:] + [L.state.in_bytes]
        return all(bool((self.arena[e:n] == self.BYTE).all()) for e, n in zip(ends, nexts))


def _poisoned(monkeypatch, field, where, value):
    """Corrupt the packed upload behind the host check."""
    index = [n for n, _ in lpstate.FIELDS].index(field) + 1
    pack = lpstate.pack_snapshot

    def wrapper(buf, snap_off, arrays):
        pack(buf, snap_off, arrays)
        buf[snap_off[index]:].view(np.int32)[where] = value
    monkeypatch.setattr(lpstate, "pack_snapshot", wrapper)


@pytest.mark.parametrize("field,where,value,text", [
    ("row_col", 1, 0, "strictly increasing"),          # the second entry of row 0 repeats / precedes the first
    ("cut_col", 0, 10 ** 6, "outside"),                # a column far out of range
    ("row_col", 5, -7, "outside"),
    ("cut_ptr", 1, 10 ** 7, "monotone"),               # an offset beyond the entries
    ("row_ptr", 2, -3, "monotone"),
])
def test_bad_input_behind_the_host_check_is_flagged(dev, model, monkeypatch, field, where, value, text):
    """The upload is corrupted after the host check (which, in its cheap form, leaves these facts to the device anyway): the call
    raises ValueError afterwards, the guard bytes around the arena and the padding between the state arrays inside it are
    untouched, and the session works again at once."""
    snap = synthetic.make_lp_snapshot("setcov", 2, scale=0.3)
    good = model.score_lp(snap)
    plain, sess = model._lp_session, _GuardedSession(model)
    model._lp_session = sess
    try:
        with monkeypatch.context() as mp:
            _poisoned(mp, field, where, value)
            for call in (lambda: model.score_lp(snap), lambda: model.select_cuts_lp(snap)):
                with pytest.raises(ValueError, match=text):
                    call()
                torch.cuda.synchronize()
                assert sess.guards_intact() and sess.interior_untouched()
            with pytest.raises(ValueError, match=text):
                model.state_from_lp(snap)                      # gcnn_lp_state flags the same violation
        assert np.array_equal(model.score_lp(snap).numpy(), good.numpy()) and sess.guards_intact() and sess.interior_untouched()
    finally:
        model._lp_session = plain


def test_host_check_runs_before_anything_is_launched(dev, model):
    snap = synthetic.make_lp_snapshot("indset", 0, scale=0.2)
    snap.cut_ptr = snap.cut_ptr.copy()
    snap.cut_ptr[3] = snap.cut_ptr[2]                  # an empty cut
    with _lib.launch_profile() as prof:
        for call in (model.score_lp, model.select_cuts_lp, model.state_from_lp):
            with pytest.raises(ValueError):
                call(snap)
    assert prof.launches == []
    ok = synthetic.make_lp_snapshot("indset", 0, scale=0.2)
    model._lp().deep_check = True                      # with the deep check the host finds the O(nnz) facts too
    try:
        ok.row_col = ok.row_col.copy()
        ok.row_col[0] = 10 ** 6
        with _lib.launch_profile() as prof:
            with pytest.raises(ValueError):
                model.score_lp(ok)
        assert prof.launches == []
    finally:
        model._lp().deep_check = False
