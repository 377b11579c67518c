"""Test-set counterpart of the reference's `model_tester.process` (/root/reference/model_tester.py:173-237) for the HIP GCNN.

The reference's tester differs from the trainer's validation pass (model_trainer.py:239-316) in what it returns: the
cut-weighted mean squared error (model_tester.py:199, 234) and the MEAN ranking fraction over all samples (`acc += frac`,
model_tester.py:224, 235) instead of thresholded accuracies.  Forward only, inference kernels (nothing is stored for a
backward pass); loss and fractions accumulate on the device and are read once at the end.

`test_group`, `test_model` and `test_models` are the rest of the test stage (model_tester.py:38-170): the gcnn, hybrid and random
figures of `results/test/{problem}/{seed}.csv` for a group of models, ranked on the device in one launch per 8 models.
"""

from __future__ import annotations

import csv
import glob
import os
from collections import namedtuple
from datetime import timedelta
from math import ceil
from time import perf_counter

import numpy as np
import torch

from . import _lib
from .graph import _ptr, _stream
from .model import GCNN
from .store import _K_CUT, HYBRID_FEATURES
from .trainer import _unpack_batch, mse_loss, ranking_fraction, ranking_metric


def process(model: GCNN, dataloader):
    """`model_tester.process(model, dataloader)` (model_tester.py:173-237): returns (loss, mean_acc) where
    loss = sum_b n_cuts_b * MSE_b / sum_b n_cuts_b and mean_acc = mean over samples of the ranking-prefix fraction
    (first position where the predicted and the true descending rankings differ, over the number of cuts).
    `dataloader` yields `utils.load_batch` 11-tuples or `SampleStore` batches."""
    dev = model.device
    none = torch.zeros(0, dtype=torch.float32, device=dev)          # no thresholds: only the per-sample fractions
    loss_dev = torch.zeros(1, dtype=torch.float32, device=dev)
    frac_dev = torch.zeros(1, dtype=torch.float64, device=dev)
    host_frac, host_loss = 0.0, 0.0                                  # samples too large for the device metric (> 4096 cuts)
    n_samples = cut_count = 0
    for batch in dataloader:
        try:
            prepared, n_cuts, y = _unpack_batch(model, batch)
            total = int(n_cuts.sum())
            with torch.no_grad():
                predictions = model(prepared, False)                 # model_tester.py:198
            loss, _ = mse_loss(predictions, y, want_grad=False)
            if len(n_cuts) == 0:
                pass
            elif n_cuts.max() <= 4096:
                frac = ranking_metric(predictions.detach().as_subclass(torch.Tensor), y, n_cuts, none, none, loss, loss_dev,
                                      float(total))
                frac_dev += frac.double().sum()
            else:
                pred, true = predictions.detach().cpu().numpy(), y.cpu().numpy()
                start = 0
                for nk in n_cuts:
                    host_frac += ranking_fraction(pred[start:start + nk], true[start:start + nk])
                    start += nk
                host_loss += float(loss) * total
            n_samples += len(n_cuts)
            cut_count += total
        except torch.OutOfMemoryError:   # model_tester.py:229-232
            print("WARNING: batch skipped.")
    loss = (float(loss_dev) + host_loss) / max(cut_count, 1)
    mean_acc = (float(frac_dev) + host_frac) / max(n_samples, 1)
    return loss, mean_acc


# ---- the test stage: model_tester.test_model / test_models (model_tester.py:38-170) ----------------------------------------
PROBLEM_FOLDERS = {"setcov": "setcov/500r", "combauc": "combauc/100i_500b", "capfac": "capfac/100c_100f",
                   "indset": "indset/500n"}                               # model_tester.py:66-67
RANK_MAX_CUTS = 4096                                                      # k_rank_multi; larger samples are ranked here

GroupTestResult = namedtuple("GroupTestResult", "loss gcnn hybrid random deviations")
GroupTestResult.__doc__ = """One model's test result: `loss`, `gcnn`, `hybrid` and `random` as model_tester.test_model reports them, and
`deviations` [3, n_samples]: the first deviating ranking position of every sample for gcnn, hybrid and random (the gcnn row of a
skipped batch is meaningless)."""


def random_rankings(seed, n_cuts):
    """The random baseline's rankings (model_tester.py:84-85, 128-129): one rng per seed, one draw for TensorFlow's seed, then per
    sample in order `r = np.arange(n); rng.shuffle(r)`."""
    rng = np.random.default_rng(seed)
    rng.integers(np.iinfo(int).max)
    out = []
    for n in n_cuts:
        r = np.arange(n)
        rng.shuffle(r)
        out.append(r)
    return out


def _order(key):
    """Stable descending order, NaN as -inf (k_rank_multi's order) -- for the samples the kernel leaves to the host."""
    key = np.array(key)
    key[np.isnan(key)] = -np.inf
    return np.argsort(-key, kind="stable")


def _deviation(ranking, truth):
    diff = np.asarray(ranking) != np.asarray(truth)
    return int(np.argmax(diff)) if diff.any() else len(truth)


def test_group(models, seeds, store, test_batch_size=4):
    """`model_tester.test_model` (model_tester.py:51-170) for several trained models at once, one seed each, on one `SampleStore`
    built with `baselines=True` over the test files in order.  Returns one `GroupTestResult` per model.

    Every batch is collated once and scored by all models (`forward_group`, up to 8 per call, into rows of one [S, K_total]
    buffer); each model's batch MSE goes into a device array.  One `gcnn_rank_deviations` launch per 8 models then ranks every
    sample of the set: each model's scores against the fp32 improvements (what model_tester.process sees), the hybrid quality and
    each seed's random rankings against the fp64 improvements (what the baseline loop sees).  One synchronisation, then the
    reference's own fp64 sums on the host."""
    from .trainer import forward_group

    models, seeds = list(models), list(seeds)
    if not models or len(seeds) != len(models):
        raise ValueError(f"test_group: one seed per model expected, got {len(models)} models and {len(seeds)} seeds")
    if not getattr(store, "baselines", False):
        raise ValueError("test_group: the store must be built with baselines=True")
    n = len(store)
    if n == 0:
        raise ValueError("test_group: the store holds no sample")
    lacking = np.flatnonzero(store.lacks_baselines)
    if len(lacking):
        raise ValueError(f"test_group: sample {int(lacking[0])} has no {'/'.join(HYBRID_FEATURES)} cut features")
    n_cuts = store.sizes[_K_CUT]
    empty = np.flatnonzero(n_cuts == 0)
    if len(empty):
        raise ValueError(f"test_group: sample {int(empty[0])} has no cuts")   # model_tester.py:138 divides by zero
    dev = store.device
    if any(m.device != dev for m in models):
        raise ValueError("test_group: the models must live on the store's device")
    S, off = len(models), store.offsets[_K_CUT]
    K = int(off[-1])
    chunks = [list(range(c, min(c + _lib.GROUP_MAX, S))) for c in range(0, S, _lib.GROUP_MAX)]
    starts = list(range(0, n, test_batch_size))
    lib = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        stream = _stream(dev)
        scores = torch.empty((S, K), dtype=torch.float32, device=dev)
        mse = torch.zeros((S, len(starts)), dtype=torch.float32, device=dev)
        skipped = np.zeros(len(starts), bool)
        for b, start in enumerate(starts):
            ids = np.arange(start, min(start + test_batch_size, n))
            lo, hi = int(off[ids[0]]), int(off[ids[-1] + 1])
            try:
                sb = store.batch(ids)
                for ch in chunks:
                    forward_group([models[m] for m in ch], [sb.batch] * len(ch), out=[scores[m, lo:hi] for m in ch])
                for m in range(S):   # trainer.mse_loss, written into its slot
                    _lib.check(lib.gcnn_mse_loss(_ptr(scores[m, lo:hi]), _ptr(sb.improvements), hi - lo, 1.0 / (hi - lo),
                                                 _ptr(mse[m, b:b + 1]), None, stream), "gcnn_mse_loss")
            except torch.OutOfMemoryError:   # model_tester.py:229-232
                print("WARNING: batch skipped.")
                skipped[b] = True
        # the random rankings, on the host while the device works
        perms_host = torch.empty((S, K), dtype=torch.int32).pin_memory()
        ph = perms_host.numpy()
        for m, seed in enumerate(seeds):
            for i, r in enumerate(random_rankings(seed, n_cuts)):
                ph[m, off[i]:off[i + 1]] = r
        perms = perms_host.to(dev, non_blocking=True)
        offsets = torch.from_numpy(off.astype(np.int32)).pin_memory().to(dev, non_blocking=True)
        rows = [2 * len(ch) + (c == 0) for c, ch in enumerate(chunks)]   # the first chunk also ranks the hybrid quality
        deviations = torch.empty((sum(rows), n), dtype=torch.int32, device=dev)
        row = 0
        for c, ch in enumerate(chunks):
            _lib.check(lib.gcnn_rank_deviations(_ptr(offsets), n, _ptr(store.improvements), _ptr(store.improvements64),
                                                _ptr(scores[ch[0]]), len(ch), _ptr(store.hybrid64) if c == 0 else None,
                                                _ptr(perms[ch[0]]), len(ch), _ptr(deviations[row]), stream),
                       "gcnn_rank_deviations")
            row += rows[c]
        big = np.flatnonzero(n_cuts > RANK_MAX_CUTS)
        if len(big):   # what the host ranks itself, downloaded with the rest
            idx = torch.from_numpy(np.concatenate([np.arange(off[i], off[i + 1]) for i in big])).to(dev)
            big_dl = [t.index_select(-1, idx).to("cpu", non_blocking=True)
                      for t in (scores, store.improvements, store.improvements64, store.hybrid64)]
        dev_dl, mse_dl = deviations.to("cpu", non_blocking=True), mse.to("cpu", non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()   # the only one
    D, mse_host = dev_dl.numpy().astype(np.int64), mse_dl.numpy()
    gcnn_dev, rand_dev, row = np.empty((S, n), np.int64), np.empty((S, n), np.int64), 0
    for c, ch in enumerate(chunks):
        gcnn_dev[ch] = D[row:row + len(ch)]
        if c == 0:
            hyb_dev = D[row + len(ch)]
        rand_dev[ch] = D[row + rows[c] - len(ch):row + rows[c]]
        row += rows[c]
    if len(big):
        sc, t32, t64, hyb = (t.numpy() for t in big_dl)
        pos = 0
        for i in big:
            k = int(n_cuts[i])
            sl = slice(pos, pos + k)
            pos += k
            o32, o64 = _order(t32[sl]), _order(t64[sl])
            hyb_dev[i] = _deviation(_order(hyb[sl]), o64)
            for m in range(S):
                gcnn_dev[m, i] = _deviation(_order(sc[m, sl]), o32)
                rand_dev[m, i] = _deviation(ph[m, off[i]:off[i + 1]], o64)
    # the reference's fp64 arithmetic, in its order
    hybrid_acc = 0
    for i in range(n):
        hybrid_acc += int(hyb_dev[i]) / int(n_cuts[i])             # model_tester.py:150-151
    hybrid_acc /= n
    results = []
    for m in range(S):
        random_acc = 0
        for i in range(n):
            random_acc += int(rand_dev[m, i]) / int(n_cuts[i])     # model_tester.py:138-139
        random_acc /= n
        loss, mean_acc, n_samples, cut_count = 0, 0, 0, 0
        for b, start in enumerate(starts):
            if skipped[b]:
                continue
            ids = range(start, min(start + test_batch_size, n))
            total = np.int32(n_cuts[start:ids.stop].sum())
            loss += total * np.float32(mse_host[m, b])              # model_tester.py:199: int32 x float32 -> float64
            acc = 0
            for i in ids:
                acc += int(gcnn_dev[m, i]) / int(n_cuts[i])         # model_tester.py:223-224
            mean_acc += acc
            n_samples += len(ids)
            cut_count += int(total)
        loss = float(loss) / cut_count if cut_count else 0.0        # model_tester.py:234-235
        mean_acc = mean_acc / n_samples if n_samples else 0.0
        results.append(GroupTestResult(loss, mean_acc, hybrid_acc, random_acc,
                                       np.stack([gcnn_dev[m], hyb_dev, rand_dev[m]])))
    return results


def write_results(problem, seed, result, root="."):
    """`results/test/{problem}/{seed}.csv` and `{seed}_loss.npy` under `root`, as model_tester.py:70-72, 155-164 writes them."""
    folder = os.path.join(root, "results", "test", problem)
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, f"{seed}.csv"), "w", newline="") as csvfile:
        writer = csv.DictWriter(csvfile, fieldnames=["type", "seed", "fraction"])
        writer.writeheader()
        writer.writerow({"type": "random", "seed": seed, "fraction": result.random})
        writer.writerow({"type": "hybrid", "seed": seed, "fraction": result.hybrid})
        writer.writerow({"type": "gcnn", "seed": seed, "fraction": result.gcnn})
    np.save(os.path.join(folder, f"{seed}_loss"), np.array(np.float64(result.loss)))


def _test_store(problem, root, device):
    from .store import SampleStore
    files = sorted(glob.glob(os.path.join(root, "data", "samples", PROBLEM_FOLDERS[problem], "test", "sample_*.pkl")))
    return SampleStore.from_files(files, device, baselines=True)


def _trained_model(problem, seed, root, device):
    model = GCNN(device=device)
    model.restore_state(os.path.join(root, "trained_models", problem, str(seed), "best_params.pkl"))
    return model


def test_model(problem, seed, test_batch_size=4, *, root=".", device=None):
    """`model_tester.test_model(problem, seed, test_batch_size)` (model_tester.py:51-170): tests the trained model of `seed` on
    the problem's test files and writes `results/test/{problem}/{seed}.csv` and `{seed}_loss.npy`, all under `root`."""
    wall_start = perf_counter()
    store = _test_store(problem, root, device)
    result = test_group([_trained_model(problem, seed, root, store.device)], [seed], store, test_batch_size)[0]
    write_results(problem, seed, result, root)
    print("Done!")
    print(f"Wall time: {str(timedelta(seconds=ceil(perf_counter() - wall_start)))}")
    print("")
    return result


def test_models(problems=("setcov", "combauc", "capfac", "indset"), *, root=".", device=None):
    """`model_tester.test_models()` (model_tester.py:38-48): the five seeds of `seeds/train_seeds.npy` for every problem -- each
    problem's five models as ONE group on one store, not five passes over the test set."""
    seeds = np.load(os.path.join(root, "seeds", "train_seeds.npy"))
    print("Testing models...")
    out = {}
    for problem in problems:
        print(f"Testing the models for {problem} problems, iterations 1-5...")
        wall_start = perf_counter()
        store = _test_store(problem, root, device)
        group = list(seeds[:5])
        results = test_group([_trained_model(problem, s, root, store.device) for s in group], group, store)
        for seed, result in zip(group, results):
            write_results(problem, seed, result, root)
        out[problem] = results
        print("Done!")
        print(f"Wall time: {str(timedelta(seconds=ceil(perf_counter() - wall_start)))}")
        print("")
    return out
