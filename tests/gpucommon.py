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
