"""Many host states in one call (GPU): `GCNN.score_states` / `GCNN.select_cuts_many` through gcnn_infer_batch -- the same bits as the
general path on the same disjoint union, every state against the fp64 oracle, proof that the new path ran, per-state isolation of
bad states, and forced rows per state.

No claim is made, and none tested, that a state's bits inside a union equal its bits alone: the row programs tile the union."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
from gcnn_cut_selector_amd import _lib, ops, synthetic, utils  # noqa: E402
from gcnn_cut_selector_amd.graph import BipartiteGraph  # noqa: E402
from gcnn_cut_selector_amd.model import SelectResult  # noqa: E402

from gpucommon import dev, general_batch as _general_batch, make_model, oracle_scores as _oracle  # noqa: E402

PROBLEMS = ("setcov", "combauc", "capfac", "indset")
SCALES = (0.2, 1.0, 0.5)
f32, i32 = np.float32, np.int32


def _mixed(S, first=0):
    """S states of all four problems at scales 0.2 - 1.0; from three states on, one without constraint edges and one with one cut."""
    out = []
    for i in range(S):
        state, _ = synthetic.make_sample(PROBLEMS[i % 4], first + i, scale=SCALES[(i + i // 4) % 3])
        out.append(utils.state_to_inputs(state))
    if S >= 3:
        c, cei, cef, v, k, kei, kef, nc, nv, nk = out[1]
        out[1] = (c, np.zeros((2, 0), i32), np.zeros((0, 1), f32), v, k, kei, kef, nc, nv, nk)
        c, cei, cef, v, k, kei, kef, nc, nv, nk = out[2]
        keep = kei[0] == 0
        out[2] = (c, cei, cef, v, k[:1], kei[:, keep], kef[keep], nc, nv, 1)
    return out


class _Spy:
    """Counts the C calls of the batch session, keeps its per-state answers and forbids the solo entry points."""

    def __init__(self, m, allow_solo=False):
        self.m, self.answers, self.solo = m, [], []
        if m._batch_session is None:
            m.score_states([])                                             # creates the session
        self.sess = m._batch_session
        self.run = self.sess.run
        self.sess.run = self._run
        self.saved = (m.score_state, m.select_cuts)
        if not allow_solo:
            def refuse(*a, **k):
                raise AssertionError("a state of a clean batch fell back to the solo path")
            m.score_state = m.select_cuts = refuse
        else:
            m.score_state = lambda *a, **k: self.solo.append("score") or self.saved[0](*a, **k)
            m.select_cuts = lambda *a, **k: self.solo.append("select") or self.saved[1](*a, **k)

    def _run(self, *a, **k):
        got = self.run(*a, **k)
        self.answers.append(got)
        return got

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sess.run = self.run
        del self.m.score_state, self.m.select_cuts
        return False


def _dense(inp):
    return R.dense_rows(inp[5][0], inp[5][1], inp[6].reshape(-1), inp[9], inp[8])


@pytest.mark.parametrize("S", [1, 2, 3, 8, 17, 64])
def test_same_bits_as_the_general_path_and_fp64(dev, S):
    m, params = make_model(90 + S, dev)
    inputs = _mixed(S, first=S)
    with _Spy(m) as spy:
        scored = m.score_states(inputs, rank=True)
        selected = m.select_cuts_many(inputs)
    # it took the new path, in one call per entry point, and no state fell back: every per-state answer is "ok" (all flags clear)
    assert len(spy.answers) == 2 and all(len(a) == S and all(r[0] == "ok" for r in a) for a in spy.answers)
    batch, k_off = _general_batch(m, inputs)
    with torch.no_grad():
        general_dev = m(batch, False).as_subclass(torch.Tensor)
        order_dev, kept_dev = ops.select_cuts(general_dev, batch.cut_graph, torch.from_numpy(k_off).to(dev),
                                              max_cuts=max(inp[9] for inp in inputs))
    general, order_g, kept_g = general_dev.cpu().numpy(), order_dev.cpu().numpy(), kept_dev.cpu().numpy()
    for s, inp in enumerate(inputs):
        q, sel = scored[s], selected[s]
        lo, hi = k_off[s], k_off[s + 1]
        assert q.dtype == f32 and q.shape == (inp[9],) and isinstance(sel, SelectResult)
        # 1. same plan, same kernels, same union: same bits
        assert np.array_equal(q.numpy(), general[lo:hi]), s
        assert np.array_equal(sel.scores.numpy(), general[lo:hi]), s
        assert list(q.rankings) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), s
        assert np.array_equal(sel.order, order_g[lo:hi]) and sel.n_kept == kept_g[s] == sel.n_selected, s
        rec = {}
        order, n = R.select(sel.scores, _dense(inp), None, 0.1, 0.5, record=rec)
        assert R.margins_ok(rec, 0.1, 0.5), s
        assert np.array_equal(sel.order, order) and sel.n_kept == n, s
        # 2. against fp64, on the state alone
        np.testing.assert_allclose(q.numpy(), _oracle(params, inp), rtol=1e-4, atol=1e-4)


def test_it_really_took_the_new_path(dev):
    m, _ = make_model(95, dev)
    inputs = _mixed(5, first=40)
    m.score_states(inputs)                                                 # buffers and layouts exist
    for call, extra in ((lambda: m.score_states(inputs), set()), (lambda: m.score_states(inputs, rank=True), {"k_ib_rank"}),
                        (lambda: m.select_cuts_many(inputs), {"k_sel_pairs", "k_sel_filter"})):
        with _Spy(m), _lib.launch_profile() as prof:
            call()
        names = [n for n, _ in prof.launches]
        assert names[0] == "k_ib_unpack" and names[1] == "k_ib_by_variable" and names.count("k_ib_unpack") == 1, names
        assert extra <= set(names) and ("k_ib_rank" in names) == ("k_ib_rank" in extra), names
        assert "k_check_edges" not in names and not [n for n in names if n.startswith("k_infer_s")], names
        assert "k_rank_scores" not in names, names


def _bad_states(rng):
    """(out-of-range variable id, row-unsorted cut edges, 4,097 cuts, a hub variable of degree 3,000) -- each otherwise well formed."""
    a = list(utils.state_to_inputs(synthetic.make_sample("setcov", 70, scale=0.2)[0]))
    a[1] = a[1].copy(); a[1][1, 5] = a[8] + 3
    b = list(utils.state_to_inputs(synthetic.make_sample("capfac", 71, scale=0.2)[0]))
    p = rng.permutation(b[5].shape[1])
    b[5], b[6] = b[5][:, p], b[6][p]
    c = list(utils.state_to_inputs(synthetic.make_sample("indset", 72, scale=0.2)[0]))
    K, V = 4097, c[8]
    rows = np.repeat(np.arange(K), 3)
    c[4] = rng.standard_normal((K, 6)).astype(f32)
    c[5] = np.stack([rows, rng.integers(0, V, 3 * K)]).astype(i32)
    c[6] = rng.standard_normal((3 * K, 1)).astype(f32)
    c[9] = K
    Ch, Vh = 3000, 50
    hub_rows = np.repeat(np.arange(Ch), 2)
    hub_cols = np.stack([np.zeros(Ch, np.int64), 1 + np.arange(Ch) % (Vh - 1)], 1).reshape(-1)
    kr = np.sort(rng.integers(0, 12, 60))
    d = [rng.standard_normal((Ch, 4)).astype(f32), np.stack([hub_rows, hub_cols]).astype(i32), (0.1 * rng.standard_normal((2 * Ch, 1))).astype(f32),
         rng.standard_normal((Vh, 14)).astype(f32), rng.standard_normal((12, 6)).astype(f32),
         np.stack([kr, rng.integers(0, Vh, 60)]).astype(i32), rng.standard_normal((60, 1)).astype(f32), Ch, Vh, 12]
    return tuple(a), tuple(b), tuple(c), tuple(d)


def test_isolation(dev):
    m, params = make_model(96, dev)
    rng = np.random.default_rng(7)
    bad_index, unsorted, huge, hub = _bad_states(rng)
    clean = _mixed(3, first=50)
    inputs = [clean[0], bad_index, clean[1], unsorted, huge, clean[2], hub]
    stayed = (0, 2, 3, 5, 6)       # the unsorted list is sorted while it is packed, and this plan has no by-variable degree limit
    solo_scores = m.score_state(huge, rank=True)
    with _Spy(m, allow_solo=True) as spy:
        scored = m.score_states(inputs, rank=True, return_exceptions=True)
        assert spy.solo == ["score"]                                      # only the 4,097-cut state went through score_state
        selected = m.select_cuts_many(inputs, return_exceptions=True)
        assert spy.solo == ["score", "select"]
    assert [r[0] for r in spy.answers[0]] == ["ok", "bad_index", "ok", "ok", "ok", "ok"]   # (the huge state never entered the union)
    assert isinstance(scored[1], ValueError) and isinstance(selected[1], ValueError)
    assert isinstance(selected[4], _lib.GcnnError) and "4097" in str(selected[4])
    assert np.array_equal(scored[4].numpy(), solo_scores.numpy()) and np.array_equal(scored[4].rankings, solo_scores.rankings)
    for s in stayed:
        inp, q, sel = inputs[s], scored[s], selected[s]
        np.testing.assert_allclose(q.numpy(), _oracle(params, inp), rtol=1e-4, atol=1e-4)
        assert list(q.rankings) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), s
        assert np.array_equal(sel.scores.numpy(), q.numpy()), s           # the same union of the same six states
        rec = {}
        order, n = R.select(sel.scores, _dense(inp), None, 0.1, 0.5, record=rec)
        assert R.margins_ok(rec, 0.1, 0.5), s
        assert np.array_equal(sel.order, order) and sel.n_kept == n, s
    # without return_exceptions the error is raised, after the others were served
    calls = m._batch_session.calls
    with pytest.raises(ValueError, match="out of range"):
        m.score_states(inputs[:3])
    assert m._batch_session.calls == calls + 1
    # S = 1 simply works, and so does an empty list
    one = m.score_states([clean[0]])[0]
    np.testing.assert_allclose(one.numpy(), _oracle(params, clean[0]), rtol=1e-4, atol=1e-4)
    assert m.score_states([]) == [] and m.select_cuts_many([]) == []
    # a state without cuts comes back in place (through score_state)
    empty = clean[1][:4] + (np.zeros((0, 6), f32), np.zeros((2, 0), i32), np.zeros((0, 1), f32)) + clean[1][7:9] + (0,)
    got = m.score_states([clean[0], empty, clean[2]], rank=True)
    assert got[1].shape == (0,) and np.array_equal(got[0].numpy(), m.score_states([clean[0], clean[2]])[0].numpy())


def _forced_like_cuts(rng, inp, F):
    """F forced rows, each on the support of one of the state's cuts (so that the filter has something to remove)."""
    rows, cols, vals = [], [], []
    for r in range(F):
        sup = inp[5][1][inp[5][0] == (r * 7) % inp[9]]
        x = rng.standard_normal(len(sup))
        rows += [r] * len(sup); cols += list(sup); vals += list(x / np.linalg.norm(x))
    return np.array([rows, cols], i32).reshape(2, -1), np.array(vals, f32), F


@pytest.mark.parametrize("p_max,p_max_ub", [(0.1, 0.5), (0.0, 0.0), (2.0, 2.0)])
def test_forced_rows_per_state(dev, p_max, p_max_ub):
    m, _ = make_model(97, dev)
    rng = np.random.default_rng(11)
    inputs = _mixed(6, first=60)
    counts = (0, 1, 40, 0, 3, 40)
    forced = [None if F == 0 and s == 0 else _forced_like_cuts(rng, inp, F) for s, (inp, F) in enumerate(zip(inputs, counts))]
    with _Spy(m) as spy:
        got = m.select_cuts_many(inputs, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=5)
    assert all(r[0] == "ok" for r in spy.answers[0])
    removed = 0
    for s, (inp, f, res) in enumerate(zip(inputs, forced, got)):
        K, V = inp[9], inp[8]
        graph = BipartiteGraph(torch.from_numpy(inp[5]).to(dev), torch.from_numpy(inp[6]).to(dev), K, V)
        fi, fv, F = f if f is not None else (np.zeros((2, 0), i32), np.zeros(0, f32), 0)
        packed = tuple(torch.from_numpy(a).to(dev) for a in ops.pack_rows(fi, fv, F, V))
        order, n_kept = ops.select_cuts(torch.from_numpy(np.asarray(res.scores)).to(dev), graph, None, packed, p_max=p_max,
                                        p_max_ub=p_max_ub, max_cuts=K)
        assert np.array_equal(res.order, order.cpu().numpy()) and res.n_kept == int(n_kept.cpu()[0]), s
        assert res.n_selected == min(res.n_kept, 5) and sorted(res.order.tolist()) == list(range(K)), s
        removed += K - res.n_kept
    assert removed == 0 if p_max == 2.0 else (removed > 0 or p_max > 0.0)   # nothing is that parallel; at 0.0 everything that touches is
