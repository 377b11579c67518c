"""Whole-model parity (GPU): the HIP GCNN against the CPU oracle on identical inputs and weights.
Tolerance (BASELINE.json north star): scores within 1e-4 absolute of the fp32/fp64 restatement; gradients within
1e-4 of the largest entry of each tensor -- or, where the reference's own fp32 arithmetic sits farther than that from fp64
(ReLU branches decided by rounding), within twice that distance (see _grad_check)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gcnn_cut_selector_amd import synthetic  # noqa: E402
from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
from gpucommon import dev, make_model  # noqa: E402


def _check_scores(m, params, state, atol=1e-4):
    got = m(state, False).numpy()
    want64 = O.scores({k: v.astype(np.float64) for k, v in params.items()}, state, torch.float64)
    assert got.shape == want64.shape and got.dtype == np.float32
    np.testing.assert_allclose(got, want64, rtol=1e-4, atol=atol)
    return got


def test_variable_spec_matches_oracle():
    from gcnn_cut_selector_amd.model import VARIABLE_SPEC
    assert [(n, tuple(s), t) for n, s, t in VARIABLE_SPEC] == [(n, tuple(s), t) for n, s, t in O.PARAM_SPEC]


@pytest.mark.parametrize("problem,batch,scale", [("setcov", 2, 0.1), ("setcov", 4, 1.0), ("combauc", 8, 1.0),
                                                 ("capfac", 2, 0.2), ("indset", 4, 1.0)])
def test_forward_parity(dev, problem, batch, scale):
    m, params = make_model(1, dev)
    state, _, _ = synthetic.make_batch(problem, batch, scale=scale)
    _check_scores(m, params, state)


def test_forward_known_answer_single_edge(dev):
    """Same hand-computed case as tests/test_oracle.py::test_known_answer_single_edge: answer 16.25."""
    from gcnn_cut_selector_amd.model import GCNN, VARIABLE_SPEC
    arrays = []
    for name, shape, _ in VARIABLE_SPEC:
        if name.endswith("/kernel"):
            w = np.zeros(shape, np.float32)
            if shape == (128, 64):
                w[:64] = np.eye(64); w[64:] = np.eye(64)
            elif shape[0] == shape[1]:
                w = np.eye(64, dtype=np.float32)
            elif shape[1] == 1:
                w[:] = 1.0
            else:
                w[0, 0] = 1.0
            arrays.append(w)
        elif name.endswith("/scale"):
            arrays.append(np.ones(shape, np.float32))
        else:
            arrays.append(np.zeros(shape, np.float32))
    m = GCNN(device=dev)
    m.set_weights(arrays)
    st = (np.array([[2.0, 0, 0, 0]]), np.array([[0], [0]]), np.array([[0.5]]), np.array([[3.0] + [0] * 13]),
          np.array([[1.0, 0, 0, 0, 0, 0]]), np.array([[0], [0]]), np.array([[0.25]]), 1, 1, 1)
    np.testing.assert_allclose(m(st, False).numpy(), [16.25], rtol=1e-6)


def test_isolated_nodes_and_unsorted_edges(dev):
    m, params = make_model(2, dev)
    rng = np.random.default_rng(0)
    C, V, K = 37, 45, 9
    cei = np.stack([rng.integers(0, C - 5, 300), rng.integers(0, V - 7, 300)])   # last rows/cols isolated
    kei = np.stack([rng.integers(0, K - 1, 80), rng.integers(0, V, 80)])         # last cut has no edge
    state = (rng.standard_normal((C, 4)), cei, rng.standard_normal((300, 1)), rng.standard_normal((V, 14)),
             rng.standard_normal((K, 6)), kei, rng.standard_normal((80, 1)), C, V, K)
    _check_scores(m, params, state)


def test_empty_cases(dev):
    m, params = make_model(3, dev)
    rng = np.random.default_rng(1)
    z2 = np.zeros((2, 0), np.int32)
    # no cuts at all -> empty score vector
    st = (rng.standard_normal((4, 4)), np.array([[0, 1], [1, 0]]), rng.standard_normal((2, 1)),
          rng.standard_normal((3, 14)), np.zeros((0, 6)), z2, np.zeros((0, 1)), 4, 3, 0)
    assert m(st, False).numpy().shape == (0,)
    # cuts but no cut edges and no constraint edges
    st = (rng.standard_normal((4, 4)), z2, np.zeros((0, 1)), rng.standard_normal((3, 14)),
          rng.standard_normal((5, 6)), z2, np.zeros((0, 1)), 4, 3, 5)
    _check_scores(m, params, st)


def test_input_validation(dev):
    m, _ = make_model(3, dev)
    state, _, _ = synthetic.make_batch("setcov", 1, scale=0.1)
    bad = list(state); bad[0] = bad[0][:, :3]
    with pytest.raises(ValueError):
        m(tuple(bad), False)
    bad = list(state); bad[7] = state[7] + 1
    with pytest.raises(ValueError):
        m(tuple(bad), False)
    bad = list(state); bad[1] = state[1].copy(); bad[1][1, 0] = state[8]
    with pytest.raises(ValueError):
        m(tuple(bad), False)


def test_batching_invariance(dev):
    """SURVEY section 4 invariant 1 on the HIP path."""
    m, _ = make_model(4, dev)
    samples = [synthetic.make_sample("setcov", i, scale=0.2) for i in range(3)]
    full = synthetic.stack_samples(samples)
    batched = m(full[:7] + (int(full[7].sum()), int(full[8].sum()), int(full[9].sum())), False).numpy()
    singles = []
    for s in samples:
        b = synthetic.stack_samples([s])
        singles.append(m(b[:7] + (int(b[7][0]), int(b[8][0]), int(b[9][0])), False).numpy())
    np.testing.assert_allclose(batched, np.concatenate(singles), rtol=1e-5, atol=1e-6)


def test_edge_order_invariance(dev):
    m, _ = make_model(5, dev)
    state, _, _ = synthetic.make_batch("combauc", 2)
    rng = np.random.default_rng(0)
    p1, p2 = rng.permutation(state[1].shape[1]), rng.permutation(state[5].shape[1])
    shuffled = (state[0], state[1][:, p1], state[2][p1], state[3], state[4], state[5][:, p2], state[6][p2]) + state[7:]
    np.testing.assert_allclose(m(state, False).numpy(), m(shuffled, False).numpy(), rtol=1e-5, atol=1e-6)


def test_forward_is_deterministic_and_training_flag_inert(dev):
    m, _ = make_model(6, dev)
    state, _, _ = synthetic.make_batch("indset", 2)
    a, b = m(state, False).numpy(), m(state, True).numpy()
    assert np.array_equal(a, b)


def _grad_check(m, params, state, y, rtol=1e-4):
    # Tolerance: fp32 kernels vs the fp64 oracle, relative to the largest entry of each tensor: 1e-4 (measured on these cases:
    # 2e-7 .. 5e-6, as close as or closer than torch's own fp32 evaluation of the restatement).  The exception is inherent to
    # fp32: a ReLU pre-activation that lands within rounding of 0 can take the other branch than in fp64, and one such edge
    # moves a gradient entry by that edge's whole share (capfac at scale 0.2: 0.05 % of the largest entry -- for the fp32
    # restatement exactly as for the kernels).  So where the reference's arithmetic itself (fp32, restated) is farther than
    # 1e-4 from fp64, the bound is twice ITS distance.
    pred = m(state, True)
    loss = ((pred - torch.as_tensor(y, device=pred.device)) ** 2).mean()
    m.flat_parameters.grad = None
    loss.backward()
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    _, want_loss, want = O.loss_and_grads(p64, state, y, torch.float64)
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    # the reference's own arithmetic is fp32: its restatement in fp32 shows how far ANY fp32 evaluation sits from fp64
    _, _, want32 = O.loss_and_grads(params, state, y, torch.float32)
    names = [n for n, _, t in O.PARAM_SPEC if t]
    bad = []
    for name, g in zip(names, m.gradients()):
        g = g.cpu().numpy().astype(np.float64)
        w = want[name]
        err = np.abs(g - w).max()
        ref = max(np.abs(w).max(), 1e-6)
        fp32_gap = np.abs(want32[name].astype(np.float64) - w).max()
        if not err <= max(rtol * ref, 2 * fp32_gap) + 1e-7:
            bad.append((name, err, ref, fp32_gap))
    assert not bad, bad


@pytest.mark.parametrize("problem,batch,scale", [("setcov", 2, 0.1), ("setcov", 3, 1.0), ("combauc", 4, 1.0),
                                                 ("capfac", 2, 0.2), ("indset", 3, 1.0)])
def test_backward_parity(dev, problem, batch, scale):
    m, params = make_model(7, dev)
    state, y, _ = synthetic.make_batch(problem, batch, scale=scale)
    _grad_check(m, params, state, y)


def test_backward_isolated_and_unsorted(dev):
    m, params = make_model(8, dev)
    rng = np.random.default_rng(3)
    C, V, K = 37, 45, 9
    cei = np.stack([rng.integers(0, C - 5, 300), rng.integers(0, V - 7, 300)])
    kei = np.stack([rng.integers(0, K - 1, 80), rng.integers(0, V, 80)])
    state = (rng.standard_normal((C, 4)), cei, rng.standard_normal((300, 1)), rng.standard_normal((V, 14)),
             rng.standard_normal((K, 6)), kei, rng.standard_normal((80, 1)), C, V, K)
    _grad_check(m, params, state, rng.uniform(0, 0.1, K))


def test_two_layer_form_for_prenorm_fitting_agrees_with_the_folded_form(dev):
    """`gcnn_forward(save_for_backward=2)` runs feature_module_final and output_module's first layer as two products and stores the
    tensor between them (PreNorm fitting needs its statistics, model.py:503, 570); the default folds them into one matrix.
    Same function: scores agree to rounding, and A equals S Wf + deg bf of the oracle."""
    import ctypes as C
    from gcnn_cut_selector_amd import _lib
    m, params = make_model(13, dev)
    state, _, _ = synthetic.make_batch("combauc", 3)
    batch = m.prepare(state)
    flat = m.flat_parameters.detach()
    ws = m._take_workspace(batch)
    folded = m._forward_into(flat, batch, ws, save=1).cpu().numpy()
    two_layer = m._forward_into(flat, batch, ws, save=2).cpu().numpy()
    np.testing.assert_allclose(two_layer, folded, rtol=2e-5, atol=2e-6)
    want = O.scores({k: v.astype(np.float64) for k, v in params.items()}, state, torch.float64)
    np.testing.assert_allclose(two_layer, want, rtol=1e-4, atol=1e-4)
    m._give_workspace(ws)


def test_save_restore_roundtrip(dev, tmp_path):
    from gcnn_cut_selector_amd.model import GCNN
    m, _ = make_model(9, dev)
    path = str(tmp_path / "best_params.pkl")
    m.save_state(path)
    m2 = GCNN(device=dev)
    m2.restore_state(path)
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    import pickle
    with open(path, "rb") as f:  # the reference's format: 62 bare pickled ndarrays (model.py:53-56)
        arrs = [pickle.load(f) for _ in range(62)]
    assert [a.shape for a in arrs] == [tuple(s) for _, s, _ in O.PARAM_SPEC]
