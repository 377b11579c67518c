"""What the GPU test modules share: the device fixture, a model with the oracle's seeded random weights, and the fp64 oracle's
scores.  A module takes the fixture by importing `dev`; it stays module-scoped there."""
import numpy as np
import pytest
import torch

from oracle import gcnn_oracle as O  # (checker only)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def make_model(seed, dev, randomize_seed=None):
    """(model, params): the oracle's initial weights for `seed`, randomised with seed + 1 unless `randomize_seed` is given."""
    from gcnn_cut_selector_amd.model import GCNN
    params = O.randomize_params(O.init_params(seed, np.float32), seed + 1 if randomize_seed is None else randomize_seed)
    m = GCNN(device=dev)
    m.set_weights([params[n] for n in O.PARAM_NAMES])
    return m, params


def oracle_scores(params, state):
    return O.scores({k: v.astype(np.float64) for k, v in params.items()}, state, torch.float64)


def union_of(inputs):
    """utils.collate of host states -> the model's 10-tuple with total counts, and the cut offsets."""
    from gcnn_cut_selector_amd import utils
    samples = [(({"values": c}, {"indices": cei, "values": cef}, {"values": v}, {"values": k}, {"indices": kei, "values": kef}),
                np.zeros(nk)) for c, cei, cef, v, k, kei, kef, nc, nv, nk in inputs]
    b = utils.collate(samples)
    return b[:7] + (int(b[7].sum()), int(b[8].sum()), int(b[9].sum())), np.concatenate([[0], np.cumsum(b[9])]).astype(np.int32)


def general_batch(m, inputs):
    """prepare() of the collated union, in the batch call's state of knowledge: gcnn_infer_batch does not know the union's longest
    segments (l_max_deg = v_max_deg = 0, "unknown": the edge passes' long-segment launch always runs), while a prepared Batch adopts
    them whenever their asynchronous copy happens to have landed.  The comparison graphs are therefore pinned to "unknown" too,
    so both sides issue the same launches whatever the timing -- the equality itself stays exact."""
    union, k_off = union_of(inputs)
    batch = m.prepare(union)
    for g in (batch.cons_graph, batch.cut_graph):
        g._md_ticket, g.l_max_deg, g.v_max_deg = None, 0, 0
        g._bind()
    return batch, k_off


def prenorm_stats(m, batch, ws, layer):
    """(mean[units], variance[units]) of one PreNorm layer's input from gcnn_prenorm_stats, as fp64 host arrays."""
    import ctypes as C
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.graph import _ptr, _stream
    units = O.PRENORM_LAYERS[layer][2]
    out = torch.full((2 * units,), float("nan"), dtype=torch.float64, device=m.device)
    with torch.cuda.device(m.device):
        _lib.check(_lib.lib().gcnn_prenorm_stats(C.byref(batch.dims), _ptr(m.flat_parameters.detach()), _ptr(batch.cons_feats),
                                                 _ptr(batch.var_feats), _ptr(batch.cut_feats), C.byref(batch.cons_graph.c),
                                                 C.byref(batch.cut_graph.c), _ptr(ws), ws.numel(), layer, _ptr(out),
                                                 _stream(m.device)), "gcnn_prenorm_stats")
    host = out.cpu().numpy()
    return host[:units], host[units:]


def oracle_prenorm_stats(params, state, layer):
    """Population mean and variance of one layer's input in fp64 (PreNormFit after a single batch)."""
    key, units = O.PRENORM_LAYERS[layer][1], O.PRENORM_LAYERS[layer][2]
    fit = {key: O.PreNormFit(units, torch.float64)}
    with pytest.raises(O.PreNormAbsorb):
        with torch.no_grad():
            O.forward(O.to_torch({k: np.asarray(v, np.float64) for k, v in params.items()}, torch.float64),
                      O.as_inputs(state, torch.float64), hook=fit)
    mean = fit[key].mean.reshape(-1).expand(units).numpy()
    var = fit[key].var.reshape(-1).expand(units).numpy()
    return mean, var


class _Reached(Exception):
    pass


def oracle_layer_inputs(params, state, dtype, layers, reduce=None):
    """{layer: the input of that PreNorm layer as an [n, units] tensor of `dtype`} from ONE oracle forward in `dtype`, which stops
    behind the last layer asked for.  The oracle's own hook absorbs one layer per forward (as the reference does); at 262,144 rows
    that is seconds per layer, so here `O.prenorm` is wrapped for the length of the call and hands every input on unchanged.
    `reduce`: applied to each input at once (e.g. `fp64_moments`), so that no [E, 64] tensor outlives its layer."""
    keys = {O.PRENORM_LAYERS[layer][1]: layer for layer in layers}
    got = {}
    plain = O.prenorm

    def recording(x, shift, scale, hook=None, key=None):
        if key in keys:
            layer = keys[key]
            x2 = x.detach().reshape(-1, O.PRENORM_LAYERS[layer][2])
            got[layer] = reduce(x2) if reduce else x2
            if len(got) == len(keys):
                raise _Reached
        return plain(x, shift, scale)

    O.prenorm = recording
    try:
        with torch.no_grad():
            O.forward(O.to_torch({k: np.asarray(v, np.float64) for k, v in params.items()}, dtype), O.as_inputs(state, dtype))
    except _Reached:
        pass
    finally:
        O.prenorm = plain
    return got


def fp64_moments(x):
    """(mean[units], variance[units]) of an [n, units] tensor, summed in fp64 whatever its dtype: mean 0, variance 0 when empty."""
    x = x.to(torch.float64)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1]), np.zeros(x.shape[1])
    mean = x.mean(0)
    return mean.numpy(), ((x - mean) ** 2).mean(0).numpy()


# ---- a training step through a NaN-filled, guarded workspace (tests/test_gpu_write_through.py, tests/test_gpu_wgrad_seams.py,
# tests/test_gpu_row_seams.py: with the autograd sibling and the workspace fingerprint) -----------------------------------------------
PATTERN = 0x7FC5A5A5           # a quiet NaN no arithmetic produces
GUARD = 16 * 64                # 16 guard rows behind the workspace


def make_state(n_cons, n_vars, n_cuts, seed):
    """A state 10-tuple with these row counts: every row has 1-4 edges to distinct variables, rows and columns sorted."""
    rng = np.random.default_rng(seed)

    def edges(n_rows):
        deg = rng.integers(1, 5, n_rows).clip(max=n_vars)
        rows = np.repeat(np.arange(n_rows), deg)
        cols = np.concatenate([np.sort(rng.choice(n_vars, d, replace=False)) for d in deg])
        return np.stack([rows, cols]).astype(np.int32), rng.standard_normal((len(rows), 1)).astype(np.float32)

    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    cei, cef = edges(n_cons)
    kei, kef = edges(n_cuts)
    return (f(n_cons, 4), cei, cef, f(n_vars, 14), f(n_cuts, 6), kei, kef, n_cons, n_vars, n_cuts), rng.uniform(0, 0.2, n_cuts)


def run_step(model, state, y, ws=None, floats=0, download=True):
    """One train_step (no optimizer) through a pattern-filled workspace of the library's size (or `floats`, if that is more) plus
    the guard rows, or through `ws` as it is.  Returns (results, workspace words on the host, words the library asked for, the workspace);
    `download=False`: None for the words (a large workspace stays on the device: `fingerprint`)."""
    import ctypes as C
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.trainer import TrainState, train_step
    dev = model.device
    batch = model.prepare(state)
    need = int(_lib.lib().gcnn_workspace_floats(C.byref(batch.dims)))
    if ws is None:
        ws = torch.empty(max(need, floats) + GUARD, dtype=torch.float32, device=dev)
        ws.view(torch.int32).fill_(PATTERN)
    assert ws.numel() >= need + GUARD
    model._ws_pool[:] = [ws]
    ts = TrainState(model)
    loss, scores = train_step(model, batch, torch.as_tensor(y, dtype=torch.float32).to(dev), None, ts)
    torch.cuda.synchronize()
    assert model._ws_pool and model._ws_pool[-1] is ws, "the step ran through another workspace"
    res = {"loss": loss.cpu().numpy(), "scores": scores.cpu().numpy(), "grads": ts.grads.cpu().numpy()}
    return res, (ws.view(torch.int32).cpu().numpy() if download else None), need, ws


def run_autograd(model, state, y, floats=0):
    """`run_step`'s sibling for the autograd path: the forward with gradients and the backward of the MSE loss through a pattern-filled,
    guarded workspace.  Returns (results, words the library asked for, the workspace); the workspace stays on the device
    (`fingerprint`)."""
    import ctypes as C
    from gcnn_cut_selector_amd import _lib
    dev = model.device
    batch = model.prepare(state)
    need = int(_lib.lib().gcnn_workspace_floats(C.byref(batch.dims)))
    ws = torch.empty(max(need, floats) + GUARD, dtype=torch.float32, device=dev)
    ws.view(torch.int32).fill_(PATTERN)
    model._ws_pool[:] = [ws]
    yt = torch.as_tensor(y, dtype=torch.float32).to(dev)
    pred = model(batch, True)
    loss = ((pred - yt) ** 2).mean()
    model.flat_parameters.grad = None
    loss.backward()
    torch.cuda.synchronize()
    assert model._ws_pool and model._ws_pool[-1] is ws, "the step ran through another workspace"
    res = {"loss": loss.detach().cpu().numpy(), "scores": pred.detach().cpu().numpy(), "grads": model.flat_parameters.grad.cpu().numpy()}
    return res, need, ws


FP_WORDS = 64                  # words per fingerprint: one [*, 64] row


def fingerprint(ws, words):
    """One fingerprint per FP_WORDS words of the first `words` words of a workspace, made on the device: the int32 words summed in
    int64 (no overflow, and any single changed word changes its sum), and beside it how many of them still carry PATTERN.  Returns
    (sums int64[ceil(words / 64)], pattern counts uint8[...]) on the host: 1/32 of the workspace and 1/256."""
    w = ws.view(torch.int32)[:words]
    pad = -words % FP_WORDS
    if pad:
        w = torch.cat([w, w.new_zeros(pad)])
    sums = torch.empty(w.numel() // FP_WORDS, dtype=torch.int64, device=w.device)
    pats = torch.empty(w.numel() // FP_WORDS, dtype=torch.uint8, device=w.device)
    step = 1 << 20             # rows per pass: the int64 copy stays at 512 MiB
    rows = w.view(-1, FP_WORDS)
    for lo in range(0, rows.shape[0], step):
        part = rows[lo:lo + step]
        sums[lo:lo + step] = part.sum(1, dtype=torch.int64)
        pats[lo:lo + step] = (part == PATTERN).sum(1).to(torch.uint8)
    return sums.cpu().numpy(), pats.cpu().numpy()
