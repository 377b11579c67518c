"""The loss head, every form of the Adam update, the readout gradient and the ranking metric on the device against fp64 (GPU):
k_mse, k_adam, k_adam_tick / k_adam_dev, the Adam tails of k_reduce (reduce_body, fold_block's emit), k_score_bwd and the fused
head at the 64-cut seam, k_ranking.

Cases, restatements and bounds are in tests/headcases.py; tests/test_headcases.py proves on the host that float32 emulations of these
kernels stay inside every bound used here and that a planted defect leaves it by a factor of 10 or changes an exact result.
  MSE       every size x scale: the loss within mse_bound(n) of fp64, d_scores bit for bit, either output absent, the words behind
            d_scores untouched
  Adam      raw flat buffers of 1 .. 524,289 floats (past the cap of 1,024 blocks: second and third trips) through Adam.apply_flat
            and Adam.apply_flat_dev, three steps from zero moments and from iterations 999 / 99,999, the gradient scale absent, a
            factor, a divisor, and the divisor 0 (no step); m, v and the parameter change per slot within adam_bounds after every
            step, each form with its own lr_t; the device's step counter and lr_t; PATTERN words behind every buffer
  fused     train_step with the optimizer riding in the backward (k_reduce / fold_block, and k_adam behind the backward on the
            degenerate batches): the restatement applied to the gradient the launch stored and to the state before the step
  readout   63 .. 129 cuts through the autograd path (k_score_bwd) and the fused head, by the rule of test_gpu_model._grad_check
  ranking   the ragged batch of headcases.rank_batch, exact; the device path of _EpochTotals.add against its host path
Every bound is derived in tests/headcases.py, none is measured.  For the record, on an MI355X: the MSE loss sits 2e-9 .. 1.4e-7
from fp64 (bounds 7.7e-7 .. 1.7e-6); m and v reach about half of their bounds, the parameter change up to 0.998 of its bound,
whose largest term is the half ulp of the parameter itself (the float32 emulation gives the same figures); the readout gradients
are 4e-9 .. 4e-8 from the oracle at entries of 0.1 .. 0.3.  Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
import gradparity  # noqa: E402
import headcases as H  # noqa: E402
from gpucommon import PATTERN, dev, make_model, make_state, run_autograd, run_step  # noqa: E402,F401

PAD = 64
f32, f64 = np.float32, np.float64


def padded(host, device):
    """(the whole buffer, its first len(host) elements): `host` on the device with PAD words of PATTERN behind it."""
    buf = torch.empty(len(host) + PAD, dtype=torch.float32, device=device)
    buf.view(torch.int32).fill_(PATTERN)
    buf[:len(host)] = torch.from_numpy(np.ascontiguousarray(host, f32))
    return buf, buf[:len(host)]


def pad_intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == PATTERN).all())


# ---- MSE head --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", H.MSE_SIZES)
def test_mse_head(dev, n):
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.graph import _ptr, _stream
    from gcnn_cut_selector_amd.trainer import mse_loss
    s, t = H.mse_case(n)
    sd, td = torch.from_numpy(s.copy()).to(dev), torch.from_numpy(t.copy()).to(dev)
    for kind in H.MSE_SCALES:
        scale = H.mse_scale(kind, n)
        want, _ = H.mse(s, t, scale)
        want_d = H.mse_d32(s, t, scale)
        loss, d = mse_loss(sd, td, scale)
        got = float(loss.cpu()[0])
        print(f"mse n={n} {kind}: loss {got!r} fp64 {want!r} rel {abs(got - want) / want if want else 0.0:.3e} bound {H.mse_bound(n):.3e}")
        assert abs(got - want) <= H.mse_bound(n) * want, (kind, got, want)
        assert d.cpu().numpy().tobytes() == want_d.tobytes(), kind
        only_loss, none = mse_loss(sd, td, scale, want_grad=False)            # d_scores absent
        assert none is None and float(only_loss.cpu()[0]) == got
        buf, dd = padded(np.zeros(n, f32), dev)                                # loss_out absent
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gcnn_mse_loss(_ptr(sd), _ptr(td), n, scale, None, _ptr(dd), _stream(dev)), "gcnn_mse_loss")
        if n:
            assert dd.cpu().numpy().tobytes() == want_d.tobytes(), kind
        assert pad_intact(buf, n)
    default, _ = mse_loss(sd, td)                                              # the scale mse_loss chooses itself: 1/n, 0 when empty
    assert float(default.cpu()[0]) == float(mse_loss(sd, td, H.mse_scale("mean", n))[0].cpu()[0])


# ---- Adam on raw flat buffers ------------------------------------------------------------------------------------------------------------
class FlatOnly:
    """What Adam.apply_flat / apply_flat_dev read of a model: its flat parameter buffer."""

    def __init__(self, flat):
        self.flat_parameters = flat


def check_step(before, after, g, lr_t, gscale, recip, what):
    """One step's m, v and parameter change against the restatement; returns the largest error / bound."""
    p0, m0, v0 = before
    p1, m1, v1 = after
    args = (p0, g, m0, v0, lr_t, H.B1, H.B2, H.EPS, gscale, recip)
    p64, m64, v64 = H.adam64(*args)
    worst = 0.0
    for name, got, want, bound in zip(("m", "v", "dp"), (m1, v1, p1.astype(f64) - p0), (m64, v64, p64 - p0), H.adam_bounds(*args)):
        ratio, bad = H.adam_compare(got, want, bound)
        worst = max(worst, ratio)
        assert bad.size == 0, (what, name, ratio, bad[:8], got[bad[:8]], want[bad[:8]], bound[bad[:8]])
    return worst


def adam_run(dev, form, n, start, kind, steps=3):
    from gcnn_cut_selector_amd.trainer import Adam
    gscale, recip = (0.0, True) if kind == "zero" else H.adam_scale(kind)
    p, m, v = H.adam_start(n, start)
    bufs = [padded(a, dev) for a in (p, m, v)]
    opt = Adam(H.LR)
    opt.iterations = start
    opt.m, opt.v = bufs[1][1], bufs[2][1]
    model = FlatOnly(bufs[0][1])
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=dev)
    state = H.opt_state(start)
    before = (p, m, v)
    worst = 0.0
    for k in range(steps):
        g = H.adam_grad(n, k)
        gbuf, gd = padded(g, dev)
        if form == "host":
            opt.apply_flat(model, gd, gs, divide=recip)
            lr_t = f32(H.tick_host(start + k + 1))
        else:
            opt.apply_flat_dev(model, gd, gs, divide=recip)
            got_state = opt._dev.cpu().numpy()
            want_state = H.tick_emul(state, gscale, recip)
            assert got_state[:5].tobytes() == want_state[:5].tobytes(), (k, got_state, want_state)      # t advanced (or not: no step)
            assert abs(float(got_state[5]) - float(want_state[5])) <= np.spacing(want_state[5]), (k, got_state, want_state)
            state, lr_t = got_state, got_state[5]
        after = tuple(b[1].cpu().numpy() for b in bufs)
        assert all(pad_intact(b[0], n) for b in bufs) and pad_intact(gbuf, n) and gd.cpu().numpy().tobytes() == g.tobytes()
        if kind == "zero":
            assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before)), "a count of 0 is no step"
        else:
            worst = max(worst, check_step(before, after, g, lr_t, gscale, recip, (form, n, start, kind, k)))
        before = after
    return worst


@pytest.mark.parametrize("n", H.ADAM_SIZES)
@pytest.mark.parametrize("form", ["host", "dev"])
def test_adam_on_flat_buffers(dev, form, n):
    for kind in H.ADAM_SCALES:
        worst = adam_run(dev, form, n, 0, kind)
        print(f"adam {form} n={n} from zero, scale {kind}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("n", [257, H.ADAM_CAP + 1])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_adam_continues_and_a_zero_count_is_no_step(dev, form, n):
    for start in H.ADAM_STARTS[1:]:
        for kind in H.ADAM_SCALES if n == 257 else ("divisor",):
            worst = adam_run(dev, form, n, start, kind)
            print(f"adam {form} n={n} from {start}, scale {kind}: largest error / bound {worst:.3f}")
    adam_run(dev, form, n, 999, "zero", steps=2)


# ---- the fused forms ---------------------------------------------------------------------------------------------------------------------
def degenerate_states():
    """The "no constraints" and "no cuts" states of tests/test_gpu_train.py::test_train_step_on_degenerate_batches."""
    rng = np.random.default_rng(5)
    z2 = np.zeros((2, 0), np.int32)
    ei = lambda n_left, n_var, n: np.stack([np.sort(rng.integers(0, n_left, n)), rng.integers(0, n_var, n)]).astype(np.int32)
    r = lambda *s: rng.standard_normal(s).astype(f32)
    no_cuts = (r(4, 4), ei(4, 3, 6), r(6, 1), r(3, 14), np.zeros((0, 6), f32), z2, np.zeros((0, 1), f32), 4, 3, 0)
    no_cons = (np.zeros((0, 4), f32), z2, np.zeros((0, 1), f32), r(3, 14), r(5, 6), ei(5, 3, 7), r(7, 1), 0, 3, 5)
    return {"no cuts": (no_cuts, np.zeros(0, f32)), "no constraints": (no_cons, rng.uniform(0, 0.1, 5).astype(f32))}


@pytest.mark.parametrize("name", ["small", "no constraints", "no cuts"])
def test_fused_adam_reproduces_the_restatement_on_the_stored_gradient(dev, name):
    from gcnn_cut_selector_amd.trainer import Adam, TrainState, train_step
    m, _ = make_model(21, dev)
    if name == "small":
        state, y = make_state(37, 45, 70, 3)
    else:
        state, y = degenerate_states()[name]
    batch = m.prepare(state)
    yd = torch.as_tensor(np.asarray(y, f32)).to(dev)
    opt, ts = Adam(H.LR), TrainState(m)
    flat = m.flat_parameters.detach()
    mask = m._trainable_mask.cpu().numpy()
    n = flat.numel()
    names = [nm for nm, _, _ in O.PARAM_SPEC]
    slots = {nm: slice(off, off + rows * cols) for nm, (off, rows, cols, _) in zip(names, m._layout)}
    if name == "no cuts":    # every gradient is 0: with moments behind them they decay and the parameters still move
        _, m0, v0 = H.adam_start(n, 999)
        opt.m, opt.v = (torch.from_numpy(np.where(mask, a, 0).astype(f32)).to(dev) for a in (m0, v0))
    for k in range(3):
        before = (flat.cpu().numpy(), opt.m.cpu().numpy() if opt.m is not None else np.zeros(n, f32),
                  opt.v.cpu().numpy() if opt.v is not None else np.zeros(n, f32))
        train_step(m, batch, yd, opt, ts)
        torch.cuda.synchronize()
        after = (flat.cpu().numpy(), opt.m.cpu().numpy(), opt.v.cpu().numpy())
        g = ts.grads.cpu().numpy()
        assert opt.iterations == k + 1 and np.isfinite(g).all()
        if name != "no cuts":
            assert np.abs(g[slots["out_2/kernel"]]).max() > 0
        for a, b in zip(after, before):     # non-trainable and padding slots: bit for bit
            assert a[~mask].tobytes() == b[~mask].tobytes(), (name, k)
        worst = check_step(tuple(b[mask] for b in before), tuple(a[mask] for a in after), g[mask], f32(H.tick_host(k + 1)),
                           None, False, (name, k))
        print(f"fused adam, {name}, step {k + 1}: largest error / bound {worst:.3f}")


# ---- readout gradient at the 64-cut seam -------------------------------------------------------------------------------------------------
READOUT_BOUND = lambda ref, gap: max(1e-4 * ref, 2 * gap) + 1e-7      # tests/test_gpu_model.py::_grad_check


@pytest.mark.parametrize("n_cuts", H.READOUT_CUTS)
def test_readout_gradient_across_the_64_cut_blocks(dev, n_cuts):
    from gcnn_cut_selector_amd.trainer import mse_loss
    m, params = make_model(23, dev)
    state, y = make_state(29, 41, n_cuts, 100 + n_cuts)
    y = y.astype(f32)
    p64 = {k: v.astype(f64) for k, v in params.items()}
    _, want_loss, want = O.loss_and_grads(p64, state, y, torch.float64)
    trainable = [nm for nm, _, t in O.PARAM_SPEC if t]
    for path in ("autograd", "fused"):
        res = run_autograd(m, state, y)[0] if path == "autograd" else run_step(m, state, y)[0]
        flat_g = torch.from_numpy(res["grads"])
        got = {nm: g.numpy() for nm, g in zip(trainable, m.gradients(flat_g))}
        for nm in ("out_2/kernel", "out_2/bias"):
            err = np.abs(got[nm].astype(f64) - want[nm]).max()
            print(f"readout K={n_cuts} {path} {nm}: error {err:.3e}, largest entry {np.abs(want[nm]).max():.3e}")
        assert abs(float(res["loss"].reshape(-1)[0]) - want_loss) <= 1e-4 * max(1.0, abs(want_loss)), path
        gradparity.check(got, params, state, y, READOUT_BOUND, want64=want)
    # the count slot of a data-parallel step, stored by k_score_bwd / by the reduction behind the fused head
    batch = m.prepare(state)
    flat = m.flat_parameters.detach()
    yd = torch.from_numpy(y).to(dev)
    grads = torch.zeros_like(flat)
    for path in ("autograd", "fused"):
        cbuf, count = padded(np.full(1, -1.0, f32), dev)
        ws = m._take_workspace(batch)
        if path == "autograd":
            scores = m._forward_into(flat, batch, ws)
            _, d = mse_loss(scores, yd)
            m._backward_into(flat, batch, ws, d, grads, count_slot=count)
        else:
            m._forward_loss_into(flat, batch, ws, yd, 1.0)
            m._backward_into(flat, batch, ws, None, grads, count_slot=count)
        m._give_workspace(ws)
        assert float(count.cpu()[0]) == float(n_cuts) and pad_intact(cbuf, 1), path


# ---- ranking metric --------------------------------------------------------------------------------------------------------------------
def test_ranking_metric_is_exact_on_the_ragged_batch(dev):
    from gcnn_cut_selector_amd.trainer import _EpochTotals, ranking_metric
    b = H.rank_batch()
    want_frac, credits = H.rank_expected()
    n_cuts = b["n_cuts"]
    assert n_cuts.max() == H.RK_MAX
    pred, truth = torch.from_numpy(b["pred"].copy()).to(dev), torch.from_numpy(b["truth"].copy()).to(dev)
    fr = torch.tensor(H.FRACTIONS, dtype=torch.float32, device=dev)
    prefill = np.array([3, 5, 7, 11], f32)
    acc = torch.from_numpy(prefill.copy()).to(dev)
    loss = torch.tensor([0.375], dtype=torch.float32, device=dev)
    loss_acc = torch.tensor([2.0], dtype=torch.float32, device=dev)
    frac = ranking_metric(pred, truth, n_cuts, fr, acc, loss, loss_acc).cpu().numpy()
    wrong = [(b["names"][i], frac[i], want_frac[i]) for i in np.flatnonzero(frac.view(np.int32) != want_frac.view(np.int32))]
    assert not wrong, wrong[:8]
    assert acc.cpu().numpy().tolist() == (prefill + credits.sum(0)).tolist()            # it accumulates
    weight = f32(n_cuts.sum())
    assert float(loss_acc.cpu()[0]) == float(f32(2.0) + f32(0.375) * weight) == 2.0 + 0.375 * float(n_cuts.sum())
    # the same samples through the epoch totals: on the device, and -- a 4,097-cut sample added -- on the host
    fractions = np.asarray(H.FRACTIONS, f32)
    on_dev = _EpochTotals(fractions, dev)
    on_dev.add(pred, truth, n_cuts, loss, float(weight))
    big_p, big_t = H.rank_sample(H.RK_MAX + 1, 1000)
    on_host = _EpochTotals(fractions, dev)
    on_host.add(torch.cat([pred, torch.from_numpy(big_p.copy()).to(dev)]), torch.cat([truth, torch.from_numpy(big_t.copy()).to(dev)]),
                np.append(n_cuts, H.RK_MAX + 1), loss, float(weight))
    assert on_host.acc.cpu().numpy().tolist() == [0, 0, 0, 0], "a sample above 4,096 cuts ran on the device"
    big = (H.fraction(big_p, big_t) >= fractions).astype(f64)
    assert on_dev.acc.cpu().numpy().tolist() == credits.sum(0).tolist() == (on_host.host_acc - big).tolist()
    assert float(on_dev.loss.cpu()[0]) == on_host.host_loss == 0.375 * float(weight)
