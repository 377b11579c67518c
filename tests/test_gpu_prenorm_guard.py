"""PreNorm fitting statistics (gcnn_prenorm_stats) against the fp64 oracle, and its refusal to read stale activations (GPU).

Layers 6, 8 and 10 (post_conv_module's PreNorm) read the scatter-sum outputs A, which only gcnn_forward(save_for_backward=2)
stores; after any other form the workspace holds whatever A an earlier forward left.  The library records the form of the last
forward per workspace and refuses (GCNN_E_BADARG) instead of returning statistics of stale memory (include/gcnn_hip.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gcnn_cut_selector_amd import synthetic  # noqa: E402
from gpucommon import dev, make_model, oracle_prenorm_stats as _oracle_stats, prenorm_stats as _stats  # noqa: E402


def _other_batch(state, seed):
    """Same dims and edge lists, other feature values."""
    rng = np.random.default_rng(seed)
    f = lambda a: rng.standard_normal(np.shape(a)).astype(np.float32)
    return (f(state[0]), state[1], f(state[2]), f(state[3]), f(state[4]), state[5], f(state[6])) + tuple(state[7:])


def test_stats_of_all_layers_after_two_layer_forward_match_oracle(dev):
    m, params = make_model(41, dev, 42)
    state, _, _ = synthetic.make_batch("combauc", 3)
    batch = m.prepare(state)
    ws = m._take_workspace(batch)
    m._forward_into(m.flat_parameters.detach(), batch, ws, save=2)
    for layer in range(11):
        mean, var = _stats(m, batch, ws, layer)
        want_mean, want_var = _oracle_stats(params, state, layer)
        sd = np.sqrt(want_var)
        np.testing.assert_allclose(mean, want_mean, rtol=1e-6, atol=1e-6 * sd.max(), err_msg=f"layer {layer} mean")
        np.testing.assert_allclose(var, want_var, rtol=1e-6, err_msg=f"layer {layer} variance")
    m._give_workspace(ws)


@pytest.mark.parametrize("save", [0, 1])
def test_post_conv_stats_refuse_after_other_forward_forms(dev, save):
    from gcnn_cut_selector_amd._lib import GcnnError
    m, params = make_model(41, dev, 42)
    state, _, _ = synthetic.make_batch("combauc", 2)
    batch = m.prepare(state)
    ws = m._take_workspace(batch)
    m._forward_into(m.flat_parameters.detach(), batch, ws, save=save)
    for layer in (6, 8, 10):
        with pytest.raises(GcnnError):
            _stats(m, batch, ws, layer)
    for layer in (0, 1, 2, 3, 4, 5, 7, 9):   # raw inputs, and the projections every forward form writes
        mean, var = _stats(m, batch, ws, layer)
        want_mean, want_var = _oracle_stats(params, state, layer)
        np.testing.assert_allclose(mean, want_mean, rtol=1e-6, atol=1e-6 * np.sqrt(want_var).max(), err_msg=f"layer {layer}")
        np.testing.assert_allclose(var, want_var, rtol=1e-6, err_msg=f"layer {layer}")
    m._give_workspace(ws)


def test_stale_activations_of_another_batch_are_refused(dev):
    """save=2 on X, then save=1 on Y with the same dims on the same workspace: layer 6 must refuse, not return X's statistics."""
    from gcnn_cut_selector_amd._lib import GcnnError
    m, params = make_model(41, dev, 42)
    x, _, _ = synthetic.make_batch("combauc", 2)
    y = _other_batch(x, 9)
    bx, by = m.prepare(x), m.prepare(y)
    assert (bx.dims.n_cons, bx.dims.n_vars, bx.dims.n_cuts, bx.dims.n_cons_edges, bx.dims.n_cut_edges) == \
           (by.dims.n_cons, by.dims.n_vars, by.dims.n_cuts, by.dims.n_cons_edges, by.dims.n_cut_edges)
    ws = m._take_workspace(bx)
    flat = m.flat_parameters.detach()
    m._forward_into(flat, bx, ws, save=2)
    mx, _ = _stats(m, bx, ws, 6)
    np.testing.assert_allclose(mx, _oracle_stats(params, x, 6)[0], rtol=1e-6, atol=1e-6)
    m._forward_into(flat, by, ws, save=1)
    with pytest.raises(GcnnError):
        _stats(m, by, ws, 6)
    m._forward_into(flat, by, ws, save=2)   # and after the right form on Y: Y's statistics
    my, vy = _stats(m, by, ws, 6)
    want_my, want_vy = _oracle_stats(params, y, 6)
    np.testing.assert_allclose(my, want_my, rtol=1e-6, atol=1e-6 * np.sqrt(want_vy).max())
    np.testing.assert_allclose(vy, want_vy, rtol=1e-6)
    m._give_workspace(ws)
