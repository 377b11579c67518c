"""The test stage on the device (GPU): `tester.test_group` and its ranking launch (gcnn_rank_deviations) against the restatement of
model_tester.test_model (tests/tester_restate.py) fed each model's solo scores and solo MSEs.

Random models, random baselines and improvements that are noise deviate at position 0 almost everywhere, which would hide most
of the ranking.  So the test set plants samples whose candidates agree with the truth over a long prefix and then deviate late:
  * score-tuned (1..4,097 cuts, each to one model, members of all three chunks of 11): the improvements are that model's own
    scores with two late neighbours swapped, plus a 1e-12 relative offset in fp64 that reorders the tied scores of duplicate cut
    rows -- the model agrees late with the fp32 truth but early with the fp64 one;
  * hybrid-tuned (200, 257, 4,097 cuts): the improvements are the hybrid quality itself (or with a late swap), whose efficacy
    column carries 1e-13 offsets -- the hybrid agrees late with the fp64 truth but early with the fp32 one;
  * random-tuned (256, 4,100 cuts, each to one model's seed): the fp64 truth order is that seed's shuffle with a late swap.
Besides the scalar results, every per-sample deviation is compared with the restatement's, and the planting is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import tester_restate as R

pytestmark = pytest.mark.gpu

from gcnn_cut_selector_amd import _lib, synthetic, tester, utils  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402
from gcnn_cut_selector_amd.store import SampleStore, hybrid_quality  # noqa: E402
from gcnn_cut_selector_amd.trainer import forward_group, mse_loss, ranking_metric  # noqa: E402
from gpucommon import dev  # noqa: E402

BS = 4
PLANTED = (1, 255, 256, 257, 4096, 4097)
# the test set, in order: ("syn", index) | ("one",) | ("score", cuts, model[, float32 features]) | ("hybrid", cuts, swap)
# | ("random", cuts, model)
SPECS = [("syn", 0), ("one",), ("syn", 1), ("score", 200, 0), ("hybrid", 200, False), ("syn", 2), ("score", 255, 3),
         ("random", 256, 9), ("syn", 3), ("score", 256, 8), ("hybrid", 257, True), ("syn", 4), ("score", 257, 9, True),
         ("syn", 5), ("score", 4096, 10), ("syn", 6), ("score", 4097, 5), ("hybrid", 4097, False), ("syn", 7), ("score", 40, 1),
         ("random", 4100, 2), ("syn", 8), ("score", 100, 7), ("syn", 9)]


def _planted(n, idx, dtype=np.float64, efficacy=None):
    """A small setcov sample whose cuts are replaced by n planted ones: hybrid features on a coarse grid (many hybrid ties) unless
    `efficacy` is given (then int_support = parallelism = 0: the hybrid quality IS the efficacy), every seventh cut a copy of the
    one before (same features and row: tied model scores), improvements on a 0.01 grid plus a 1e-13 offset on every third cut."""
    state, _ = synthetic.make_sample("setcov", idx, scale=0.1)
    cons, cons_edge, var, cut, cut_edge = state
    n_vars = var["values"].shape[0]
    rng = np.random.default_rng(1000 + n)
    feats = np.stack([rng.standard_normal(n), rng.random(n), rng.integers(0, 3, n) * 0.5, rng.integers(1, 3, n) * 0.1,
                      rng.random(n), rng.integers(0, 2, n).astype(np.float64)], axis=1)
    if efficacy is not None:
        feats[:, 2], feats[:, 3], feats[:, 5] = 0.0, efficacy, 0.0
    rows = [np.sort(rng.choice(n_vars, 3, replace=False)) for _ in range(n)]
    vals = [rng.standard_normal(3) for _ in range(n)]
    for j in range(6, n, 7):
        feats[j], rows[j], vals[j] = feats[j - 1], rows[j - 1], vals[j - 1]
    improvements = 0.01 * rng.integers(1, 6, n) + np.where(np.arange(n) % 3 == 0, 1e-13 * np.arange(n), 0.0)
    kei = np.stack([np.repeat(np.arange(n), 3), np.concatenate(rows)])
    state = (cons, cons_edge, var, dict(cut, values=feats.astype(dtype)),
             dict(cut_edge, indices=kei, values=np.concatenate(vals).reshape(-1, 1)))
    return state, improvements


def _late_swap(key, frac=0.8):
    """`key` with the values of two neighbours of its stable descending ranking swapped at about frac * n, where they differ."""
    key = np.array(key)
    order = np.argsort(-key, kind="stable")
    for r in range(int(frac * len(key)), len(key) - 1):
        if key[order[r]] != key[order[r + 1]]:
            key[order[r]], key[order[r + 1]] = key[order[r + 1]], key[order[r]]
            return key
    raise AssertionError("no distinct late neighbours")


def _solo(model, store):
    """Each batch's scores and MSE of the model alone (`model(batch)`, `trainer.mse_loss`)."""
    preds, mses = [], []
    with torch.no_grad():
        for sb in store.batches(np.arange(len(store)), BS):
            s = model(sb.batch)
            preds.append(s.detach().cpu().numpy())
            mses.append(np.float32(mse_loss(s, sb.improvements, want_grad=False)[0].item()))
    return preds, mses


def _per_sample(preds, n_cuts):
    return np.split(np.concatenate(preds), np.cumsum(n_cuts)[:-1])


def _build_samples(dev, models, seeds):
    """SPECS -> samples, with the improvements of the planted samples tuned as the module docstring says.  Scores do not depend on
    the improvements, so they are taken from a store of the same samples in the same batches."""
    samples = []
    for k, spec in enumerate(SPECS):
        if spec[0] == "syn":
            samples.append(synthetic.make_sample("setcov", spec[1], scale=0.2))
        elif spec[0] == "one":
            samples.append(_planted(1, 60))
        elif spec[0] == "hybrid":
            n = spec[1]
            eff = 0.01 * np.random.default_rng(n).integers(1, 6, n) + np.where(np.arange(n) % 3 == 0, 1e-13 * np.arange(n), 0.0)
            samples.append(_planted(n, 50 + k, efficacy=eff))
        else:
            samples.append(_planted(spec[1], 50 + k, np.float32 if len(spec) > 3 and spec[3] else np.float64))
    n_cuts = [s[1].shape[0] for s in samples]
    draft = SampleStore.from_samples(samples, dev)
    scores = {}
    for spec in SPECS:
        if spec[0] == "score" and spec[2] not in scores:
            scores[spec[2]] = _per_sample(_solo(models[spec[2]], draft)[0], n_cuts)
    out = []
    for i, (spec, (state, imp)) in enumerate(zip(SPECS, samples)):
        n = n_cuts[i]
        if spec[0] == "score":
            imp32 = _late_swap(scores[spec[2]][i])
            imp = imp32.astype(np.float64) * (1.0 + 1e-12 * (np.arange(n) % 5))
            assert np.array_equal(imp.astype(np.float32), imp32)     # the fp32 truth is the swapped scores, exactly
        elif spec[0] == "hybrid":
            h = np.asarray(hybrid_quality(state[3]), np.float64)
            imp = _late_swap(h, 0.6) if spec[2] else h
        elif spec[0] == "random":
            perm = tester.random_rankings(seeds[spec[2]], n_cuts)[i]
            imp = np.empty(n)
            imp[perm] = n - np.arange(n, dtype=np.float64)               # fp64 truth order = the seed's shuffle
            imp = _late_swap(imp)
        out.append((state, imp))
    return out


def _restated_deviations(samples, preds, seed):
    """Per-sample (gcnn, hybrid, random) deviations of the restatement: tester_restate.deviation / random_deviation."""
    n_cuts = [s[1].shape[0] for s in samples]
    perms = tester.random_rankings(seed, n_cuts)
    rows = [[], [], []]
    for (state, imp), pred, perm in zip(samples, _per_sample(preds, n_cuts), perms):
        rows[0].append(R.deviation(pred, np.asarray(imp).astype(np.float32)))
        rows[1].append(R.deviation(R.hybrid_pred(state[3]), imp))
        rows[2].append(R.random_deviation(perm, imp))
    return np.array(rows)


@pytest.fixture(scope="module")
def world(dev):
    models = [GCNN(device=dev, seed=10 + i) for i in range(11)]
    seeds = [int(s) for s in np.random.default_rng(5).integers(0, 2 ** 31, 11)]
    samples = _build_samples(dev, models, seeds)
    store = SampleStore.from_samples(samples, dev, baselines=True)
    solo = [_solo(m, store) for m in models]
    want = [R.test_model(samples, p, l, seed, BS) for (p, l), seed in zip(solo, seeds)]
    devs = [_restated_deviations(samples, p, seed) for (p, _), seed in zip(solo, seeds)]
    return dict(samples=samples, store=store, models=models, seeds=seeds, solo=solo, want=want, devs=devs)


def test_planted_cases_are_there(world):
    """The planting worked: late deviations on the tuned samples, and the other truth would have given an earlier one."""
    samples, devs = world["samples"], world["devs"]
    sizes = [s[1].shape[0] for s in samples]
    assert all(n in sizes for n in PLANTED)
    late = 0
    for i, spec in enumerate(SPECS):
        n = sizes[i]
        state, imp = samples[i]
        if spec[0] == "score":
            pred = _per_sample(world["solo"][spec[2]][0], sizes)[i]
            assert len(np.unique(pred)) < n or n < 7                             # tied scores (duplicate rows)
            assert devs[spec[2]][0, i] >= n // 2, (spec, devs[spec[2]][0, i])
            if n >= 200:
                assert R.deviation(pred, imp) < devs[spec[2]][0, i] // 2, spec   # the fp64 truth deviates much earlier
            late += 1
        elif spec[0] == "hybrid":
            assert devs[0][1, i] >= n // 2, (spec, devs[0][1, i])
            assert devs[0][1, i] == (n if not spec[2] else devs[0][1, i])
            assert R.deviation(R.hybrid_pred(state[3]), imp.astype(np.float32)) < n // 10, spec   # the fp32 truth: early
            late += 1
        elif spec[0] == "random":
            assert devs[spec[2]][2, i] >= n // 2, (spec, devs[spec[2]][2, i])
            others = [devs[m][2, i] for m in range(11) if world["seeds"][m] != world["seeds"][spec[2]]]
            assert max(others) < n // 10, spec                                   # only that seed's shuffle agrees
            late += 1
    assert late == 13


@pytest.mark.parametrize("S", [1, 5, 8, 11])
def test_group_equals_the_restatement(world, S):
    store, models, seeds = world["store"], world["models"][:S], world["seeds"][:S]
    got = tester.test_group(models, seeds, store, BS)
    assert len(got) == S
    for m, (r, want) in enumerate(zip(got, world["want"])):
        assert (r.loss, r.gcnn, r.hybrid, r.random) == (want["loss"], want["gcnn"], want["hybrid"], want["random"]), m
        assert r.deviations.shape == (3, len(store))
        bad = np.argwhere(r.deviations != world["devs"][m])
        assert len(bad) == 0, (m, [(int(k), int(i), int(r.deviations[k, i]), int(world["devs"][m][k, i])) for k, i in bad[:5]])
    for m in {0, S - 1}:
        loss, acc = tester.process(models[m], store.batches(np.arange(len(store)), BS))
        assert abs(got[m].gcnn - acc) <= 1e-6
        assert abs(got[m].loss - loss) <= 1e-6 * abs(got[m].loss)


def test_members_equal_their_solo_call(world):
    store, models, seeds = world["store"], world["models"], world["seeds"]
    group = tester.test_group(models, seeds, store, BS)
    for m, r in enumerate(group):
        (solo,) = tester.test_group([models[m]], [seeds[m]], store, BS)
        assert (r.loss, r.gcnn, r.hybrid, r.random) == (solo.loss, solo.gcnn, solo.hybrid, solo.random), m
        assert np.array_equal(r.deviations, solo.deviations), m


def test_gcnn_deviations_match_the_ranking_metric(world, dev):
    store, models = world["store"], world["models"]
    got = tester.test_group(models, world["seeds"], store, BS)
    none = torch.zeros(0, dtype=torch.float32, device=dev)
    n_cuts = store.sizes[2]
    checked = late = 0
    for m, model in enumerate(models):
        for b, (start, (pred, _)) in enumerate(zip(range(0, len(store), BS), zip(*world["solo"][m]))):
            ids = np.arange(start, min(start + BS, len(store)))
            if n_cuts[ids].max() > 4096:
                continue
            sb = store.batch(ids)
            frac = ranking_metric(torch.from_numpy(pred).to(dev), sb.improvements, n_cuts[ids], none, none).cpu().numpy()
            want = got[m].deviations[0, ids].astype(np.float32) / n_cuts[ids].astype(np.float32)
            assert np.array_equal(frac, want), (m, b)
            checked += len(ids)
            late += int(((got[m].deviations[0, ids] >= n_cuts[ids] // 2) & (n_cuts[ids] >= 40)).sum())
    assert checked == 11 * (len(store) - 8) and late >= 5   # the score-tuned samples of the batches checked here


def test_one_ranking_launch_per_eight_models(world):
    store, models, seeds = world["store"], world["models"], world["seeds"]
    for S, launches in ((5, 1), (8, 1), (11, 2)):
        with _lib.launch_profile() as prof:
            tester.test_group(models[:S], seeds[:S], store, BS)
        names = [n for n, _ in prof.launches]
        assert names.count("k_rank_multi") == launches, (S, names.count("k_rank_multi"))


def test_forward_group_writes_into_out_views(world, dev):
    store, models = world["store"], world["models"][:3]
    sb = store.batch(np.arange(4))
    n = sb.batch.dims.n_cuts
    buf = torch.full((3, n + 5), float("nan"), dtype=torch.float32, device=dev)
    views = [buf[i, 2:2 + n] for i in range(3)]
    got = forward_group(models, [sb.batch] * 3, out=views)
    want = forward_group(models, [sb.batch] * 3)
    for i in range(3):
        assert got[i].data_ptr() == views[i].data_ptr() and torch.equal(views[i], want[i]), i
        assert torch.isnan(buf[i, :2]).all() and torch.isnan(buf[i, 2 + n:]).all(), i
    flat = torch.empty(n + 1, dtype=torch.float32, device=dev)
    with pytest.raises(_lib.GcnnError):   # overlapping outputs: the group call's overlap check refuses them
        forward_group(models[:2], [sb.batch] * 2, out=[flat[:n], flat[1:]])
    with pytest.raises(ValueError):
        forward_group(models[:1], [sb.batch], out=[flat[:n - 1]])
    with pytest.raises(ValueError):
        forward_group(models[:2], [sb.batch] * 2, out=[flat[:n]])


def test_kernel_edges_directly(dev):
    """Empty sample -> 0, more than 4,096 cuts -> -1, agreement -> n, an out-of-range permutation entry deviates there; rows
    without a hybrid vector shift up."""
    n_big = 4097
    offsets = torch.tensor([0, 0, 3, 3 + n_big, 3 + n_big + 2], dtype=torch.int32, device=dev)
    K = 3 + n_big + 2
    t32 = torch.zeros(K, dtype=torch.float32, device=dev)
    t32[:3] = torch.tensor([1.0, 3.0, 2.0])
    t32[-2:] = torch.tensor([float("nan"), 5.0])            # NaN ranks as -inf: order [1, 0]
    t64 = t32.double()
    scores = torch.stack([t32, -t32]).contiguous()
    perms = torch.zeros((1, K), dtype=torch.int32, device=dev)
    perms[0, :3] = torch.tensor([1, 2, 7])                  # 7 is out of range: deviates at rank 2
    perms[0, -2:] = torch.tensor([1, 0])
    out = torch.full((2 + 1 + 1, 4), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    lib = _lib.lib()
    with _lib.launch_profile() as prof:
        rc = lib.gcnn_rank_deviations(p(offsets), 4, p(t32), p(t64), p(scores), 2, p(t64), p(perms), 1, p(out), None)
    assert rc == 0 and [n for n, _ in prof.launches] == ["k_rank_multi"]
    want = [[0, 3, -1, 2], [0, 0, -1, 2], [0, 3, -1, 2], [0, 2, -1, 2]]   # -t32 of the last sample: [NaN, -5] ranks as [1, 0] too
    assert out.cpu().tolist() == want
    out2 = torch.full((2, 4), -7, dtype=torch.int32, device=dev)
    assert lib.gcnn_rank_deviations(p(offsets), 4, p(t32), p(t64), p(scores), 1, None, p(perms), 1, p(out2), None) == 0
    assert out2.cpu().tolist() == [want[0], want[3]]


def test_kernel_late_deviations_directly(dev):
    """0, 1, 200, 256, 257, 4,096 and 4,097 cuts in one launch with 8 score rows, a hybrid vector and 8 permutations, against
    tester_restate.  Improvements on a coarse grid with 1e-13 offsets on odd cuts: fp32 ties where fp64 does not.  Candidates: the
    fp32 truth itself (agrees: n), with a late swap, a key in the fp64 truth order (early against the fp32 truth), noise; hybrid =
    the fp64 truth with a late swap; permutations: the fp64 order, with a late swap, the fp32 order, noise.  The kernel answers -1
    above 4,096 cuts (the host ranks those) and 0 without cuts."""
    rng = np.random.default_rng(3)
    sizes = [200, 0, 256, 1, 257, 4096, 4097]
    order = lambda k: np.argsort(-k, kind="stable")
    swap = lambda k, f=0.8: _late_swap(k, f) if len(k) > 1 else np.array(k)
    t32s, t64s, hybs, scores, perms = [], [], [], [[] for _ in range(4)], [[] for _ in range(4)]
    for n in sizes:
        t64 = 0.001 * rng.integers(1, 50, n) + np.where(np.arange(n) % 2 == 1, 1e-13 * np.arange(n), 0.0)
        t32 = t64.astype(np.float32)
        o32, o64 = order(t32), order(t64)
        key64 = np.empty(n, np.float32)
        key64[o64] = (n - np.arange(n)).astype(np.float32)
        p64 = o64.copy()
        if n > 1:
            r = int(0.8 * n)
            p64[r], p64[r + 1] = p64[r + 1], p64[r]
        for row, c in zip(scores, (t32, swap(t32), key64, rng.standard_normal(n).astype(np.float32))):
            row.append(c)
        for row, c in zip(perms, (o64, p64, o32, rng.permutation(n))):
            row.append(c.astype(np.int32))
        t32s.append(t32), t64s.append(t64), hybs.append(swap(t64, 0.7))
    want = []
    for k in (0, 1, 2, 3, 3, 2, 1, 0):
        want.append([R.deviation(c, t) for c, t in zip(scores[k], t32s)])
    want.append([R.deviation(h, t) for h, t in zip(hybs, t64s)])
    for k in (3, 2, 1, 0, 0, 1, 2, 3):
        want.append([R.random_deviation(c, t) for c, t in zip(perms[k], t64s)])
    want = np.array(want)
    for j, n in enumerate(sizes):   # the planting: late agreement, and the other truth deviates early
        if n >= 200:
            assert want[0, j] == want[12, j] == n and want[1, j] >= n // 2 and want[8, j] >= n // 2 and want[14, j] >= n // 2
            assert want[2, j] < n // 10 and want[10, j] < n // 10
            assert R.deviation(hybs[j], t32s[j]) < n // 10
    want[:, np.array(sizes) > 4096] = -1
    cat = lambda parts, dt: torch.from_numpy(np.concatenate(parts).astype(dt)).to(dev)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    t32, t64, hyb = cat(t32s, np.float32), cat(t64s, np.float64), cat(hybs, np.float64)
    sc = torch.stack([cat(scores[k], np.float32) for k in (0, 1, 2, 3, 3, 2, 1, 0)]).contiguous()
    pm = torch.stack([cat(perms[k], np.int32) for k in (3, 2, 1, 0, 0, 1, 2, 3)]).contiguous()
    out = torch.full((17, len(sizes)), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert _lib.lib().gcnn_rank_deviations(p(offsets), len(sizes), p(t32), p(t64), p(sc), 8, p(hyb), p(pm), 8, p(out),
                                           None) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()


def test_refusals_enqueue_nothing(world, dev):
    store = world["store"]
    lib = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    n = len(store)
    offsets = torch.from_numpy(store.offsets[2].astype(np.int32)).to(dev)
    K = int(store.offsets[2, -1])
    scores = torch.zeros((9, K), dtype=torch.float32, device=dev)
    perms = torch.zeros((9, K), dtype=torch.int32, device=dev)
    out = torch.zeros((19, n), dtype=torch.int32, device=dev)
    t32, t64, hyb = p(store.improvements), p(store.improvements64), p(store.hybrid64)
    with _lib.launch_profile() as prof:
        assert lib.gcnn_rank_deviations(p(offsets), n, t32, t64, p(scores), 9, hyb, p(perms), 1, p(out), None) == -1
        assert lib.gcnn_rank_deviations(p(offsets), n, t32, t64, p(scores), 1, hyb, p(perms), 9, p(out), None) == -1
        assert lib.gcnn_rank_deviations(p(offsets), n, None, t64, p(scores), 1, hyb, p(perms), 1, p(out), None) == -1
        assert lib.gcnn_rank_deviations(p(offsets), n, t32, None, p(scores), 1, hyb, p(perms), 1, p(out), None) == -1
    torch.cuda.synchronize()
    assert prof.launches == []
    assert not out.any()


def test_store_keeps_the_baselines_bit_for_bit(world, dev):
    samples, store = world["samples"], world["store"]
    want_h = np.concatenate([np.asarray(R.hybrid_pred(s[0][3])).astype(np.float64) for s in samples])
    want_i = np.concatenate([np.asarray(s[1]).astype(np.float64) for s in samples])
    assert np.array_equal(store.hybrid64.cpu().numpy().view(np.uint64), want_h.view(np.uint64))
    assert np.array_equal(store.improvements64.cpu().numpy().view(np.uint64), want_i.view(np.uint64))
    assert store.hybrid64.dtype == store.improvements64.dtype == torch.float64
    plain, default = SampleStore.from_samples(samples, dev, baselines=False), SampleStore.from_samples(samples, dev)
    assert plain.nbytes == default.nbytes and store.nbytes == plain.nbytes + 16 * int(store.offsets[2, -1])
    assert not hasattr(plain, "hybrid64") and not hasattr(plain, "improvements64")
    assert torch.equal(plain.improvements, store.improvements) and torch.equal(plain.cut_feats, store.cut_feats)


def test_driver_refusals(world, dev):
    samples, models, seeds = world["samples"], world["models"][:1], world["seeds"][:1]
    plain = SampleStore.from_samples(samples[:3], dev)
    with pytest.raises(ValueError, match="baselines=True"):
        tester.test_group(models, seeds, plain)
    state, imp = samples[0]
    names = ["rhs", "support", "int_support", "other", "cutoff", "parallelism"]
    lacking = [samples[1], ((state[0], state[1], state[2], dict(state[3], features=names), state[4]), imp)]
    store = SampleStore.from_samples(lacking, dev, baselines=True)
    assert store.lacks_baselines.tolist() == [False, True]
    with pytest.raises(ValueError, match="sample 1"):
        tester.test_group(models, seeds, store)
    c, ce, v, k, ke = state
    empty = (c, ce, v, dict(k, values=k["values"][:0]), dict(ke, indices=np.zeros((2, 0), np.int64), values=ke["values"][:0]))
    store = SampleStore.from_samples([samples[1], samples[2], (empty, imp[:0])], dev, baselines=True)
    with pytest.raises(ValueError, match="sample 2 has no cuts"):
        tester.test_group(models, seeds, store)
    with pytest.raises(ValueError, match="one seed per model"):
        tester.test_group(models, [1, 2], world["store"])


def test_test_model_and_test_models_write_the_reference_files(tmp_path, dev):
    root = tmp_path
    folder = root / "data" / "samples" / "setcov" / "500r" / "test"
    folder.mkdir(parents=True)
    samples = [synthetic.make_sample("setcov", 200 + i, scale=0.2) for i in range(6)] + [_planted(300, 99)]
    for i, (state, imp) in enumerate(samples):
        utils.save_sample(str(folder / f"sample_{i + 1}.pkl"), state, imp)
    seeds = np.random.default_rng(11).integers(0, 2 ** 31, 5)
    (root / "seeds").mkdir(exist_ok=True)
    np.save(root / "seeds" / "train_seeds.npy", seeds)
    for i, seed in enumerate(seeds):
        (root / "trained_models" / "setcov" / str(seed)).mkdir(parents=True)
        GCNN(device=dev, seed=70 + i).save_state(str(root / "trained_models" / "setcov" / str(seed) / "best_params.pkl"))
    files = sorted(str(f) for f in folder.glob("sample_*.pkl"))
    loaded = [utils.load_sample(f) for f in files]
    store = SampleStore.from_samples(loaded, dev)
    want_dir = tmp_path / "want"
    for seed in seeds:
        model = GCNN(device=dev)
        model.restore_state(str(root / "trained_models" / "setcov" / str(seed) / "best_params.pkl"))
        preds, mses = _solo(model, store)
        R.write(str(want_dir), seed, R.test_model(loaded, preds, mses, seed, 4))
    out = root / "results" / "test" / "setcov"

    def check(seed):
        assert (out / f"{seed}.csv").read_bytes() == (want_dir / f"{seed}.csv").read_bytes()
        got, want = np.load(out / f"{seed}_loss.npy"), np.load(want_dir / f"{seed}_loss.npy")
        assert got.dtype == want.dtype and got.shape == want.shape and got == want

    tester.test_model("setcov", seeds[0], root=str(root), device=dev)
    check(seeds[0])
    (out / f"{seeds[0]}.csv").unlink()
    tester.test_models(("setcov",), root=str(root), device=dev)
    for seed in seeds:
        check(seed)
