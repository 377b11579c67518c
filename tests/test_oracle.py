"""Oracle self-checks (CPU): the torch restatement vs an independent NumPy forward, the oracle-free invariants of
SURVEY.md section 4, hand-computed known answers, and an fp64 finite-difference gradcheck."""
import numpy as np
import pytest
import torch

from gcnn_cut_selector_amd import synthetic
from oracle import gcnn_oracle as O


def _params(seed=0, dtype=np.float64):
    return O.randomize_params(O.init_params(seed, dtype), seed + 1)


def _tiny_state(seed=0):
    rng = np.random.default_rng(seed)
    C, V, K = 5, 7, 3
    cei = np.array([[0, 0, 1, 2, 2, 2, 4], [1, 3, 0, 2, 5, 6, 3]])  # constraint 3 and variable 4 are isolated
    kei = np.array([[0, 1, 1, 2], [6, 0, 2, 5]])
    return (rng.standard_normal((C, 4)), cei, rng.standard_normal((cei.shape[1], 1)), rng.standard_normal((V, 14)),
            rng.standard_normal((K, 6)), kei, rng.standard_normal((kei.shape[1], 1)), C, V, K)


def test_param_spec_matches_survey():
    assert len(O.PARAM_SPEC) == 62
    shapes = [s for _, s, _ in O.PARAM_SPEC]
    assert shapes[:6] == [(4,), (4,), (4, 64), (64,), (64, 64), (64,)]
    assert shapes[6:8] == [(1,), (1,)]
    assert shapes[22:34] == [(64, 64), (64,), (1, 64), (64, 64), (1,), (64, 64), (64,), (1,), (128, 64), (64,),
                             (64, 64), (64,)]
    assert shapes[-4:] == [(64, 64), (64,), (64, 1), (1,)]


def test_orthogonal_init():
    p = O.init_params(3, np.float64)
    w = p["cons_conv_out_1/kernel"]
    np.testing.assert_allclose(w.T @ w, np.eye(64), atol=1e-12)
    w = p["var_emb_1/kernel"]  # (14, 64): orthonormal rows
    np.testing.assert_allclose(w @ w.T, np.eye(14), atol=1e-12)


def test_torch_vs_numpy_forward():
    p, st = _params(), _tiny_state()
    a = O.scores(p, st, torch.float64)
    b = O.numpy_forward(p, st, np.float64, loop_scatter=True)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    state, _, _ = synthetic.make_batch("setcov", 2, scale=0.1)
    np.testing.assert_allclose(O.scores(p, state, torch.float64), O.numpy_forward(p, state), rtol=1e-10, atol=1e-12)


def test_fp32_close_to_fp64():
    p = _params()
    state, _, _ = synthetic.make_batch("combauc", 2)
    a = O.scores(p, state, torch.float64)
    b = O.scores({k: v.astype(np.float32) for k, v in p.items()}, state, torch.float32)
    np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-4)


def test_batching_invariance():
    """Invariant 1: scores of a stacked batch == concatenation of per-sample scores."""
    p = _params()
    samples = [synthetic.make_sample("setcov", i, scale=0.08) for i in range(3)]
    full = synthetic.stack_samples(samples)
    state = full[:7] + (int(full[7].sum()), int(full[8].sum()), int(full[9].sum()))
    batched = O.scores(p, state, torch.float64)
    single = []
    for s in samples:
        b = synthetic.stack_samples([s])
        single.append(O.scores(p, b[:7] + (int(b[7][0]), int(b[8][0]), int(b[9][0])), torch.float64))
    np.testing.assert_allclose(batched, np.concatenate(single), rtol=1e-11, atol=1e-12)


def test_edge_order_invariance():
    """Invariant 2: permuting the COO edge list leaves outputs unchanged (scatter_nd sums duplicates)."""
    p, st = _params(), _tiny_state(1)
    rng = np.random.default_rng(0)
    p1, p2 = rng.permutation(st[1].shape[1]), rng.permutation(st[5].shape[1])
    st2 = (st[0], st[1][:, p1], st[2][p1], st[3], st[4], st[5][:, p2], st[6][p2]) + st[7:]
    np.testing.assert_allclose(O.scores(p, st, torch.float64), O.scores(p, st2, torch.float64), rtol=1e-12)


def test_isolated_receiver_gets_zero_row_without_final_bias():
    """Invariant 3: a receiver with no edge gets conv row 0 -> out = MLP([0 | x_recv]); b_final NOT added."""
    p = O.to_torch(_params(), torch.float64)
    rng = np.random.default_rng(2)
    left, var = torch.tensor(rng.standard_normal((3, 64))), torch.tensor(rng.standard_normal((4, 64)))
    ei = torch.tensor([[0, 0, 2], [1, 3, 3]])
    ef = torch.tensor(rng.standard_normal((3, 1)))
    out = O.conv(p, "cons_conv", left, ei, ef, var, 3, True)
    h = torch.relu(torch.cat([torch.zeros(1, 64, dtype=torch.float64), left[1:2]], 1) @ p["cons_conv_out_1/kernel"]
                   + p["cons_conv_out_1/bias"])
    want = torch.relu(h @ p["cons_conv_out_2/kernel"] + p["cons_conv_out_2/bias"])
    np.testing.assert_allclose(out[1:2].numpy(), want.numpy(), rtol=1e-12)


def test_hoisting_identity():
    """Invariant 4: sum_e (H_e W + b) == (sum_e H_e) W + deg * b -- the identity the HIP path relies on."""
    rng = np.random.default_rng(3)
    H, W, b = rng.random((50, 64)), rng.standard_normal((64, 64)), rng.standard_normal(64)
    idx = rng.integers(0, 7, 50)
    lhs = np.zeros((7, 64)); np.add.at(lhs, idx, H @ W + b)
    S = np.zeros((7, 64)); np.add.at(S, idx, H)
    np.testing.assert_allclose(lhs, S @ W + np.bincount(idx, minlength=7)[:, None] * b, rtol=1e-12, atol=1e-12)


def test_known_answer_single_edge():
    """Invariant 8: one constraint, one variable, one cut, one edge each; weights chosen so the answer is by hand."""
    p = O.init_params(0, np.float64)
    for name, shape, _ in O.PARAM_SPEC:
        if name.endswith("/kernel"):
            w = np.zeros(shape)
            if shape == (128, 64):
                w[:64] = np.eye(64); w[64:] = np.eye(64)
            elif shape[0] == shape[1]:
                w = np.eye(64)
            elif shape[1] == 1:
                w[:] = 1.0  # readout: sum of the 64 channels
            else:
                w[0, 0] = 1.0  # first feature -> channel 0 (also the (1,64) edge kernels)
            p[name] = w
    st = (np.array([[2.0, 0, 0, 0]]), np.array([[0], [0]]), np.array([[0.5]]), np.array([[3.0] + [0] * 13]),
          np.array([[1.0, 0, 0, 0, 0, 0]]), np.array([[0], [0]]), np.array([[0.25]]), 1, 1, 1)
    # channel 0 only: c=2, v=3, k=1.  conv1: J=2+.5+3=5.5 -> A=5.5 -> c'=5.5+2=7.5
    # conv2: J=7.5+.5+3=11 -> v'=11+3=14 ; conv3: J=1+.25+14=15.25 -> k'=15.25+1=16.25 ; readout = 16.25
    np.testing.assert_allclose(O.scores(p, st, torch.float64), [16.25], rtol=1e-13)
    np.testing.assert_allclose(O.numpy_forward(p, st), [16.25], rtol=1e-13)


def test_training_flag_is_inert_and_output_flat():
    p, st = _params(), _tiny_state(4)
    out = O.scores(p, st, torch.float64)
    assert out.shape == (3,)


def test_gradcheck_fp64():
    """Invariant 7: fp64 finite differences of the loss vs autograd, on every trainable tensor (sampled entries)."""
    p, st = _params(5), _tiny_state(5)
    y = np.random.default_rng(5).uniform(0, 0.1, 3)
    _, loss, grads = O.loss_and_grads(p, st, y, torch.float64)
    rng = np.random.default_rng(6)
    eps = 1e-6
    for name, g in grads.items():
        flat = p[name].reshape(-1)
        for idx in rng.choice(flat.size, size=min(3, flat.size), replace=False):
            old = flat[idx]
            flat[idx] = old + eps; lp = O.loss_and_grads(p, st, y, torch.float64)[1]
            flat[idx] = old - eps; lm = O.loss_and_grads(p, st, y, torch.float64)[1]
            flat[idx] = old
            fd = (lp - lm) / (2 * eps)
            assert abs(fd - g.reshape(-1)[idx]) <= 1e-6 * max(1.0, abs(fd)) + 1e-8, (name, idx, fd, g.reshape(-1)[idx])


def test_chan_merge_equals_two_pass():
    """Invariant 6: streaming (count, mean, M2) == two-pass population mean/variance of the concatenation."""
    rng = np.random.default_rng(7)
    chunks = [rng.standard_normal((n, 4)) * 3 + 1 for n in (5, 17, 1, 40)]
    fit = O.PreNormFit(4, torch.float64)
    for c in chunks:
        fit.update(torch.tensor(c))
    shift, scale = fit.finish()
    allx = np.concatenate(chunks)
    np.testing.assert_allclose(shift.numpy(), -allx.mean(0), rtol=1e-12)
    np.testing.assert_allclose(scale.numpy(), 1 / np.sqrt(allx.var(0)), rtol=1e-12)
    fit = O.PreNormFit(1, torch.float64)  # constant input: var == 0 -> scale 1 (model.py:432)
    fit.update(torch.full((6, 1), 2.0, dtype=torch.float64))
    shift, scale = fit.finish()
    assert float(shift) == -2.0 and float(scale) == 1.0


def test_pretrain_fits_eleven_layers_in_call_order():
    p = O.init_params(8, np.float64)
    batches = [synthetic.make_batch("setcov", 2, first_sample=2 * i, scale=0.08)[0] for i in range(3)]
    fitted, n = O.pretrain(p, batches, torch.float64)
    assert n == 11
    # layer 1 (constraint features) sees the raw inputs of every batch
    allc = np.concatenate([b[0] for b in batches]).astype(np.float64)
    np.testing.assert_allclose(fitted["cons_prenorm/shift"], -allc.mean(0), rtol=1e-10, atol=1e-12)
    # is_tight is 0/1 -> finite scale; after fitting, every fitted activation is ~unit variance
    assert np.all(np.isfinite(fitted["cons_prenorm/scale"]))
    for _, scale, _ in O.PRENORM_LAYERS:
        assert np.all(fitted[scale] > 0)
    # a second pretraining pass over the already-normalised first layer gives the same numbers (idempotent inputs)
    again, _ = O.pretrain(O.init_params(8, np.float64), batches, torch.float64)
    for k in fitted:
        np.testing.assert_array_equal(fitted[k], again[k])


def test_keras_adam_step_known_answer():
    theta, g = np.array([1.0, -2.0]), np.array([0.5, -0.25])
    th, m, v = O.keras_adam_step(theta, g, np.zeros(2), np.zeros(2), 1, lr=0.1)
    # step 1: m_hat = g, v_hat = g^2 -> update ~ lr * sign(g) (eps outside the sqrt)
    lr_t = 0.1 * np.sqrt(1 - 0.999) / (1 - 0.9)
    np.testing.assert_allclose(th, theta - lr_t * (0.1 * g) / (np.sqrt(0.001 * g * g) + 1e-7), rtol=1e-14)
    np.testing.assert_allclose(th, theta - 0.1 * np.sign(g), atol=1e-5)


def test_ranking_fraction():
    assert O.ranking_fraction(np.array([3., 2, 1]), np.array([9., 5, 1])) == 1.0
    assert O.ranking_fraction(np.array([3., 1, 2]), np.array([9., 5, 1])) == pytest.approx(1 / 3)
    assert O.ranking_fraction(np.array([1., 2, 3]), np.array([9., 5, 1])) == 0.0


def test_relu_hook_records_and_forces_one_unit():
    """ReluHook: an empty hook changes nothing; the recorded pre-activations and magnitudes are those of the layer; forcing one
    unit of the head's hidden layer changes the loss and the head's gradients exactly as the hand-computed flip predicts."""
    p, st = _params(4), _tiny_state(2)
    y = np.array([0.1, -0.2, 0.05])
    pred0, loss0, g0 = O.loss_and_grads(p, st, y, torch.float64)
    rec = O.ReluHook()
    pred1, loss1, g1 = O.loss_and_grads(p, st, y, torch.float64, relu_hook=rec)
    assert np.array_equal(pred0, pred1) and loss0 == loss1
    assert all(np.array_equal(g0[n], g1[n]) for n in g0)
    sites = {f"{e}_emb_{i}" for e in ("cons", "var", "cut") for i in (1, 2)}
    sites |= {f"{c}_{s}" for c in ("cons_conv", "var_conv", "cut_conv") for s in ("joint", "out_1", "out_2")} | {"out_1"}
    assert set(rec.sites) == sites
    assert rec.sites["cons_conv_joint"][0].shape == (st[1].shape[1], 64)
    for z, m in rec.sites.values():
        assert bool((m >= z.abs() * (1 - 1e-12)).all())
    # the head by hand from the recorded tensors: k = relu(z of cut_conv_out_2), z1 = k W1 + b1
    k = torch.relu(rec.sites["cut_conv_out_2"][0]).numpy()
    z1 = rec.sites["out_1"][0].numpy()
    np.testing.assert_allclose(z1, k @ p["out_1/kernel"] + p["out_1/bias"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(rec.sites["out_1"][1].numpy(), np.abs(k) @ np.abs(p["out_1/kernel"]) + np.abs(p["out_1/bias"]),
                               rtol=1e-12)
    w2, b2 = p["out_2/kernel"], p["out_2/bias"]

    def head(mask):
        h = z1 * mask
        pred = (h @ w2 + b2).reshape(-1)
        d = 2 * (pred - y) / len(y)                       # d loss / d pred
        dz = (d[:, None] * w2[:, 0][None, :]) * mask     # d loss / d z1
        return pred, np.mean((pred - y) ** 2), {"out_2/kernel": h.T @ d[:, None], "out_2/bias": d.sum(keepdims=True),
                                                 "out_1/bias": dz.sum(0), "out_1/kernel": k.T @ dz}
    mask = (z1 > 0).astype(np.float64)
    r, c = np.unravel_index(np.argmin(np.abs(z1)), z1.shape)   # the unit nearest its kink: the one rounding could flip
    flipped = mask.copy()
    flipped[r, c] = 1 - flipped[r, c]
    for msk, (pr, ls, gs) in ((mask, (pred0, loss0, g0)), (flipped, O.loss_and_grads(
            p, st, y, torch.float64, relu_hook=O.ReluHook(force=[("out_1", r, c)], record=False)))):
        want_pred, want_loss, want = head(msk)
        np.testing.assert_allclose(pr, want_pred, rtol=1e-12, atol=1e-13)
        assert abs(ls - want_loss) <= 1e-12 * max(1.0, want_loss)
        for name, w in want.items():
            np.testing.assert_allclose(gs[name], w, rtol=1e-11, atol=1e-13, err_msg=name)
    # the flip moves out_1/kernel in column c only, by the unit's own share k[r] * dz[r, c]
    _, _, gf = O.loss_and_grads(p, st, y, torch.float64, relu_hook=O.ReluHook(force=[("out_1", r, c)], record=False))
    moved = np.abs(gf["out_1/kernel"] - g0["out_1/kernel"]).max(0) > 0
    if abs(z1[r, c]) > 0:
        assert moved[c]
    # forcing a unit elsewhere (a joint unit of the first convolution: edge 3, constraint 2 -> variable 2, which reaches the cuts)
    # reaches the gradients before it
    _, _, gj = O.loss_and_grads(p, st, y, torch.float64, relu_hook=O.ReluHook(force=[("cons_conv_joint", 3, 0)], record=False))
    assert not np.array_equal(gj["cons_conv_feat_final/kernel"], g0["cons_conv_feat_final/kernel"])


def test_flip_proof_accepts_a_proven_flip_and_rejects_a_defect():
    """tests/gradparity.py on the CPU: gradients of the fp64 oracle with one ambiguous unit forced (what an fp32 evaluation that
    rounds that unit the other way computes) pass only through that proof; the same gradients with one column of a weight
    gradient moved by 2e-4 of its largest entry -- the size of a flip, but not a flip -- fail."""
    import gradparity
    from test_gpu_stress import CASES, _state
    params = O.randomize_params(O.init_params(11, np.float32), 12)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    rng = np.random.default_rng(1005)
    state = _state(CASES[5], rng)
    y = rng.uniform(0, 0.2, state[9])
    units = gradparity.ambiguous_units(p64, state, y)
    assert 1 <= len(units) <= gradparity.MAX_AMBIGUOUS, units
    unit = units[0][:3]
    _, _, flipped = O.loss_and_grads(p64, state, y, torch.float64, relu_hook=O.ReluHook(force=[unit], record=False))
    got = {n: g.astype(np.float32) for n, g in flipped.items()}
    rule = lambda ref, gap: max(1e-4 * ref, 3 * gap) + 1e-7 * ref
    _, _, plain = O.loss_and_grads(p64, state, y, torch.float64)
    assert any(np.abs(flipped[n] - plain[n]).max() > 1e-4 * np.abs(plain[n]).max() for n in plain)   # the flip is visible
    assert gradparity.check(got, params, state, y, rule) == [unit]
    bad = {n: g.astype(np.float32) for n, g in plain.items()}
    w = bad["var_conv_out_1/kernel"]
    w[:, 7] += 2e-4 * np.abs(plain["var_conv_out_1/kernel"]).max()
    with pytest.raises(AssertionError):
        gradparity.check(bad, params, state, y, rule)
