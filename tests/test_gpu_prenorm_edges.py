"""PreNorm fitting statistics past one grid trip, on the cap of 1,024 blocks and at degenerate inputs (GPU): the cases of
tests/prenormcases.py (tests/test_prenormcases.py proves on the host what each is and which defect it tells from a correct pass).

Layers 0 .. 4 read raw fp32 arrays and sum them in fp64, so the reference is `math.fsum` over the same arrays and the bound is the
derived one of `prenormcases.raw_bounds` (2 n 2^-53 mean|x| for the mean: 6e-11 of mean|x| at n = 262,145), not the 1e-6 of the
older tests; a constant column must come back exactly.  Layers 5 .. 10 read fp32 activations: fp64 oracle, rtol 1e-6 with atol
1e-6 sd, or twice the distance of the oracle's own fp32 evaluation where that is larger (`prenormcases.conv_bounds`).  Every figure
is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import prenormcases as P  # noqa: E402
from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
from gpucommon import dev, fp64_moments, make_model, oracle_layer_inputs, prenorm_stats  # noqa: E402,F401
from test_gpu_prenorm_group import _assert_same, _tuple  # noqa: E402

SEED = 41


class _Runs:
    """Per case, computed once: the device statistics of its layers (one save=2 forward), and for its layers >= 5 the fp64
    oracle's moments and the distance of the fp32 oracle's (one forward each, all layers at once)."""

    def __init__(self, dev):
        self.m, self.params = make_model(SEED, dev, SEED + 1)
        self.device, self.oracle = {}, {}

    def on_device(self, name):
        if name not in self.device:
            case = P.case(name)
            batch = self.m.prepare(case["state"])
            ws = self.m._take_workspace(batch)
            self.m._forward_into(self.m.flat_parameters.detach(), batch, ws, save=2)
            self.device[name] = {layer: prenorm_stats(self.m, batch, ws, layer) for layer in case["layers"]}
            self.m._give_workspace(ws)
        return self.device[name]

    def of_oracle(self, name):
        """{layer: (mean, variance, fp32 distance of the mean, of the variance)} for the case's layers >= 5."""
        if name not in self.oracle:
            case = P.case(name)
            layers = [layer for layer in case["layers"] if layer >= 5]
            m64 = oracle_layer_inputs(self.params, case["state"], torch.float64, layers, reduce=fp64_moments)
            # the oracle's fp32 evaluation: its activations in fp32, summed in fp64 as the device sums them (fp32 sums of 16 M
            # values would add an error the device does not have, and a wider bound with it)
            m32 = oracle_layer_inputs(self.params, case["state"], torch.float32, layers, reduce=fp64_moments)
            self.oracle[name] = {layer: (float(m64[layer][0][0]), float(m64[layer][1][0]),
                                         abs(float(m32[layer][0][0] - m64[layer][0][0])),
                                         abs(float(m32[layer][1][0] - m64[layer][1][0]))) for layer in layers}
        return self.oracle[name]


@pytest.fixture(scope="module")
def runs(dev):
    return _Runs(dev)


@pytest.mark.parametrize("name", P.NAMES)
def test_raw_layers_meet_the_derived_fp64_bound(runs, name):
    case = P.case(name)
    got = runs.on_device(name)
    for layer in case["layers"]:
        if layer > 4:
            continue
        x = P.raw_input(case["state"], layer)
        mean, var = got[layer]
        for u in range(x.shape[1]):
            want_mean, want_var, mean_abs = P.exact_stats(x[:, u])
            bm, bv = P.raw_bounds(x.shape[0], want_var, mean_abs)
            em, ev = abs(mean[u] - want_mean), abs(var[u] - want_var)
            print(f"{name} layer {layer} unit {u} n {x.shape[0]}: mean {want_mean:.6g} err {em:.3g} (bound {bm:.3g}), "
                  f"variance {want_var:.6g} err {ev:.3g} (bound {bv:.3g})")
            assert em <= bm and ev <= bv, (name, layer, u, mean[u], want_mean, var[u], want_var)


def test_constant_columns_come_back_exactly(runs):
    mean, var = runs.on_device("constant")[2]
    for col, c in P.CONSTANT_COLS.items():
        P.assert_constant_exact(P.case("constant")["state"][3][:, col], c)
        assert mean[col] == float(c) and var[col] == 0.0, (col, mean[col], var[col])


@pytest.mark.parametrize("name", [n for n in P.NAMES if n not in ("constant", "offset")])
def test_conv_layers_match_the_fp64_oracle(runs, name):
    case = P.case(name)
    s = P.sizes(case["state"])
    got, want = runs.on_device(name), runs.of_oracle(name)
    for layer, (want_mean, want_var, gap_mean, gap_var) in sorted(want.items()):
        mean, var = float(got[layer][0][0]), float(got[layer][1][0])
        if s[P.LAYER[layer][1]] == 0:       # nothing to absorb: exactly 0, 0
            assert (mean, var) == (0.0, 0.0) == (want_mean, want_var), (name, layer, mean, var)
            continue
        bm, bv = P.conv_bounds(want_mean, want_var, gap_mean, gap_var)
        print(f"{name} layer {layer}: mean {want_mean:.8g} device {abs(mean - want_mean):.3g} fp32 oracle {gap_mean:.3g} "
              f"(bound {bm:.3g}); variance {want_var:.8g} device {abs(var - want_var):.3g} fp32 oracle {gap_var:.3g} (bound {bv:.3g})")
        assert abs(mean - want_mean) <= bm and abs(var - want_var) <= bv, (name, layer, mean, want_mean, var, want_var)


def _batches(name, n, seed):
    """n load_batch tuples of the case's dims and edge lists: the case's own state, then other bulk values."""
    state = P.case(name)["state"]
    states = [state] + [P.other_features(state, seed + i) for i in range(1, n)]
    return [_tuple(st, np.zeros(st[9], np.float32)) for st in states]


def test_full_fit_on_seam_sized_batches_matches_the_oracle(dev):
    from gcnn_cut_selector_amd.model import GCNN
    from gcnn_cut_selector_amd.trainer import pretrain
    loader = _batches("seam-small", 2, 700)
    m = GCNN(device=dev, seed=5)
    p0 = dict(zip(O.PARAM_NAMES, m.get_weights()))
    assert pretrain(m, loader) == 11
    batches = [b[:7] + (int(b[7].sum()), int(b[8].sum()), int(b[9].sum())) for b in loader]
    fitted, n = O.pretrain({k: v.astype(np.float64) for k, v in p0.items()}, batches, torch.float64)
    assert n == 11
    scalars = 0
    for shift, scale, _ in O.PRENORM_LAYERS:
        for name in (shift, scale):
            if name:
                got = m.get_variable(name).cpu().numpy()
                scalars += got.size
                np.testing.assert_allclose(got, fitted[name], rtol=1e-4, atol=1e-6, err_msg=name)
    assert scalars == 58


def test_full_fit_freezes_a_constant_unit_exactly(dev):
    """Two batches with the same constant column: variance 0 in both, no spread between them: scale 1 (var == 0 -> 1), shift -c."""
    from gcnn_cut_selector_amd.model import GCNN
    from gcnn_cut_selector_amd.trainer import pretrain
    m = GCNN(device=dev, seed=6)
    assert pretrain(m, _batches("constant", 1, 0) * 2) == 11
    shift, scale = (m.get_variable(f"var_prenorm/{k}").cpu().numpy() for k in ("shift", "scale"))
    for col, c in P.CONSTANT_COLS.items():
        assert scale[col] == np.float32(1.0) and shift[col] == -c, (col, shift[col], scale[col])
    others = [u for u in range(14) if u not in P.CONSTANT_COLS]
    assert np.all(scale[others] != 1.0) and np.all(np.abs(scale[others] - 1.0) < 0.05)


def test_group_members_at_the_block_cap_match_solo_pretrain(dev):
    """Two members whose every statistics grid is at the cap (the twins look a block up in the prefix table past a member's first
    1,024 blocks) and a small third one."""
    from gcnn_cut_selector_amd.trainer import pretrain, pretrain_many
    loaders = [_batches("seam-small", 2, 800), _batches("seam-small", 2, 900)[::-1], _batches("tiny-no_cut_edges", 1, 0)]
    solo = [make_model(60 + i, dev)[0] for i in range(3)]
    grp = [make_model(60 + i, dev)[0] for i in range(3)]
    k_solo = [pretrain(m, ld) for m, ld in zip(solo, loaders)]
    k_grp = pretrain_many(grp, loaders)
    torch.cuda.synchronize()
    assert k_solo[:2] == [11, 11]
    for i in range(3):
        _assert_same(i, solo[i], grp[i], k_solo[i], k_grp[i])
