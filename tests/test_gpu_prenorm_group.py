"""PreNorm fitting of several models together (GPU): `trainer.pretrain_many` must give every member, bit for bit, the parameters,
PreNorm state and layer count of `trainer.pretrain` on that member alone, send same-shaped members out in the launches of one,
and read nothing back from the device in a pass but the merge states at its end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gcnn_cut_selector_amd import synthetic  # noqa: E402
from oracle import gcnn_oracle as O  # noqa: E402  (initial weights only)
from gpucommon import dev, make_model  # noqa: E402

STATE_KEYS = ["cons_feats", "cons_edge_inds", "cons_edge_feats", "var_feats", "cut_feats", "cut_edge_inds", "cut_edge_feats"]


def _tuple(state10, y):
    """a load_batch 11-tuple (one stacked sample) from a state with total counts"""
    return tuple(state10[:7]) + (np.array([state10[7]]), np.array([state10[8]]), np.array([state10[9]]), np.asarray(y, np.float32))


def _strip_cut_edges(b):
    c, cei, cef, v, k, kei, kef, nc, nv, nk, y = b
    return (c, cei, cef, v, k, np.zeros((2, 0), kei.dtype), kef[:0], nc, nv, nk, y)


def _strip_cuts(b):
    c, cei, cef, v, k, kei, kef, nc, nv, nk, y = b
    return (c, cei, cef, v, k[:0], np.zeros((2, 0), kei.dtype), kef[:0], nc, nv, np.zeros_like(nk), y[:0])


def _assert_same(i, solo, grp, k_solo, k_grp):
    assert k_solo == k_grp, (i, k_solo, k_grp)
    assert torch.equal(solo.flat_parameters.detach().view(torch.int32), grp.flat_parameters.detach().view(torch.int32)), i
    for layer, (a, b) in enumerate(zip(solo._prenorm_state, grp._prenorm_state)):
        assert (a["waiting"], a["received"]) == (b["waiting"], b["received"]), (i, layer)
        for key in ("count", "mean", "var"):
            x, y = np.asarray(a[key]), np.asarray(b[key])
            assert x.dtype == y.dtype == np.float32 and x.shape == y.shape and x.tobytes() == y.tobytes(), (i, layer, key, x, y)


def test_single_member_matches_pretrain_on_golden_batches(dev, golden_dir):
    from gcnn_cut_selector_amd.model import GCNN
    from gcnn_cut_selector_amd.trainer import pretrain, pretrain_many
    z = np.load(os.path.join(golden_dir, "pretrain_combauc.npz"))
    batches = []
    for b in range(3):
        c = z[f"b{b}_counts"]
        st = tuple(z[f"b{b}_" + k] for k in STATE_KEYS)
        batches.append(st + (np.array([c[0]]), np.array([c[1]]), np.array([c[2]]), np.zeros(int(c[2]), np.float32)))
    models = []
    for _ in range(2):
        m = GCNN(device=dev)
        m.set_weights([z["w_" + n.replace("/", "__")] for n in O.PARAM_NAMES])
        models.append(m)
    k_solo = pretrain(models[0], batches)
    (k_grp,) = pretrain_many([models[1]], [batches])
    assert k_solo == 11
    _assert_same(0, models[0], models[1], k_solo, k_grp)


@pytest.fixture(scope="module")
def loaders(dev):
    """Eight loaders: four problems, store batches and 11-tuples, different lengths and batch sizes, a batch without cut edges
    (layers 4 and 9 absorb nothing from it), a member without a single cut (it takes the solo entry inside each group call) and
    one without any batch."""
    from gcnn_cut_selector_amd.store import SampleStore
    from gcnn_cut_selector_amd.trainer import _StoreBatches
    sample = lambda prob, i, scale: synthetic.make_sample(prob, i, scale=scale)
    stores = {"setcov": SampleStore.from_samples([sample("setcov", i, 0.2) for i in range(5)], dev),
              "capfac": SampleStore.from_samples([sample("capfac", i, 0.3) for i in range(3)], dev),
              "combauc": SampleStore.from_samples([sample("combauc", i, 1.0) for i in range(2)], dev)}

    def tuples(prob, first, sizes, scale):
        out = []
        for s in sizes:
            state, y, _ = synthetic.make_batch(prob, s, first, scale)
            out.append(_tuple(state, y))
            first += s
        return out

    return [
        _StoreBatches(stores["setcov"], np.arange(4), 2),
        tuples("combauc", 10, [1, 1], 1.0) + [_strip_cut_edges(tuples("combauc", 12, [1], 1.0)[0])],
        _StoreBatches(stores["capfac"], np.arange(3), 2),
        tuples("indset", 0, [2], 0.05),
        [_strip_cuts(b) for b in tuples("setcov", 20, [1, 2], 0.2)],
        tuples("setcov", 30, [2, 1, 1], 0.15),
        _StoreBatches(stores["combauc"], np.array([1, 0]), 1),
        [],
    ]


@pytest.mark.parametrize("size", [2, 5, 8])
def test_members_match_solo_pretrain(dev, loaders, size):
    from gcnn_cut_selector_amd.trainer import pretrain, pretrain_many
    solo = [make_model(60 + i, dev)[0] for i in range(size)]
    grp = [make_model(60 + i, dev)[0] for i in range(size)]
    k_solo = [pretrain(m, ld) for m, ld in zip(solo, loaders)]
    k_grp = pretrain_many(grp, loaders[:size])
    torch.cuda.synchronize()
    for i in range(size):
        _assert_same(i, solo[i], grp[i], k_solo[i], k_grp[i])
    assert k_solo[:4] == [11] * min(size, 4)
    if size == 8:
        assert k_solo[7] == 0


def _same_shape(dev, n):
    from gcnn_cut_selector_amd.store import SampleStore
    store = SampleStore.from_samples([synthetic.make_sample("setcov", i, scale=0.2) for i in range(2)], dev)
    return [list(store.batches(np.arange(2), 2)) for _ in range(n)]


def test_same_shaped_members_share_launches(dev):
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.trainer import pretrain_many
    counts = {}
    for n in (1, 4):
        models, lds = [make_model(80 + i, dev)[0] for i in range(n)], _same_shape(dev, n)
        pretrain_many(models, lds)   # first use: launch attributes, tables
        with _lib.launch_profile() as prof:
            assert pretrain_many(models, lds) == [11] * n
        counts[n] = [name for name, _ in prof.launches]
        assert all(name.startswith("k_group_") for name in counts[n]), set(counts[n])
    assert counts[4] == counts[1]
    assert len(counts[1]) <= 11 * 13   # one group call per pass (one batch each), at most 13 launches each


def test_no_host_read_inside_a_pass(dev, monkeypatch):
    from gcnn_cut_selector_amd.model import GCNN
    from gcnn_cut_selector_amd.trainer import pretrain_many
    n = 3
    models, lds = [make_model(90 + i, dev)[0] for i in range(n)], _same_shape(dev, n)
    for ld in lds:
        ld.append(ld[0])   # two batches per pass
    events = []

    def forbidden(*a, **k):
        raise AssertionError("GCNN.pretrain must not be called")
    monkeypatch.setattr(GCNN, "pretrain", forbidden)

    def counted(name):
        orig = getattr(torch.Tensor, name)

        def wrapper(self, *a, **k):
            if self.is_cuda:
                events.append(name)
            return orig(self, *a, **k)
        return wrapper
    for name in ("cpu", "item", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counted(name))
    sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (events.append("synchronize"), sync(*a, **k))[1])
    nxt = GCNN.pretrain_next
    monkeypatch.setattr(GCNN, "pretrain_next", lambda self: (events.append("next"), nxt(self))[1])
    assert pretrain_many(models, lds) == [11] * n
    assert events == (["cpu"] + ["next"] * n) * 11, events


def test_refusals(dev):
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.trainer import _group_member, _tables, pretrain_many
    models, lds = [make_model(100 + i, dev)[0] for i in range(2)], _same_shape(dev, 2)
    with pytest.raises(ValueError):
        pretrain_many(models, lds, process_group=object())
    with pytest.raises(ValueError):
        pretrain_many([models[0]] * 2, lds)
    with pytest.raises(ValueError):
        pretrain_many([make_model(0, dev)[0] for _ in range(9)], [lds[0]] * 9)
    # overlapping merge states: refused, nothing enqueued
    batch = lds[0][0].batch
    wss = [m._take_workspace(batch) for m in models]
    members = [_group_member(m, batch, ws, None) for m, ws in zip(models, wss)]
    states = torch.full((2, _lib.PRENORM_STATE_BYTES // 4), 7.0, device=dev)
    for second in (states[0].data_ptr(), states[0].data_ptr() + 64):
        layers = (C.c_int32 * 2)(0, 0)
        ptrs = (C.c_void_p * 2)(states[0].data_ptr(), second)
        fn = lambda k, arr, host, table, nbytes, stream: _lib.lib().gcnn_group_prenorm_merge(k, arr, layers, ptrs, host, table,
                                                                                            nbytes, stream)
        with _lib.launch_profile() as prof, pytest.raises(_lib.GcnnError):
            _tables(dev).call(fn, members, "gcnn_group_prenorm_merge", dev)
        assert prof.launches == []
    torch.cuda.synchronize()
    assert bool((states == 7.0).all())
