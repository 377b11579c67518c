"""The test stage end to end: `tester.test_group` with five models on a synthetic setcov test store (default 2,000 samples) against
the way model_tester.test_model does it -- five `tester.process` passes over the set, then the reference's host baseline loop
(model_tester.py:100-153: the hybrid rule and a per-seed shuffle, ranked with sorted(), per sample and per seed) restated over the
in-memory samples (no files: its zlib time is not counted).  Both sides run on the same store; the figures agree, which is checked.
Wall-clock medians over the repeats (each side ends with a host sync).  For the kernel times, run it under
`rocprofv3 --kernel-trace --stats -- python tools/test_models.py --repeats 1`.
Usage: python tools/test_models.py [--samples N] [--models S] [--repeats R] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import synthetic, tester  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402
from gcnn_cut_selector_amd.store import SampleStore, hybrid_quality  # noqa: E402


def sorted_deviation(pred, true):
    pred_ranking = np.array(sorted(range(len(pred)), key=lambda x: pred[x], reverse=True))
    true_ranking = np.array(sorted(range(len(true)), key=lambda x: true[x], reverse=True))
    differences = pred_ranking != true_ranking
    return int(np.argmax(differences)) if np.any(differences) else len(true)


def reference_baselines(samples, seed):
    """model_tester.py:84-85, 100-153 over in-memory samples: (random_acc, hybrid_acc)."""
    rng = np.random.default_rng(seed)
    rng.integers(np.iinfo(int).max)
    random_acc = hybrid_acc = 0
    for state, true in samples:
        pred = hybrid_quality(state[3])
        random_ranking = np.arange(len(true))
        rng.shuffle(random_ranking)
        true_ranking = np.array(sorted(range(len(true)), key=lambda x: true[x], reverse=True))
        diff = random_ranking != true_ranking
        random_acc += (int(np.argmax(diff)) if np.any(diff) else len(true)) / len(true)
        hybrid_acc += sorted_deviation(pred, true) / len(true)
    return random_acc / len(samples), hybrid_acc / len(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--models", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    samples = [synthetic.make_sample("setcov", i) for i in range(args.samples)]
    store = SampleStore.from_samples(samples, dev, baselines=True)
    models = [GCNN(device=dev, seed=i) for i in range(args.models)]
    seeds = [1000 + i for i in range(args.models)]
    ids = np.arange(len(store))

    def group():
        return tester.test_group(models, seeds, store, args.batch)

    def reference():
        out = []
        for m, seed in zip(models, seeds):
            loss, acc = tester.process(m, store.batches(ids, args.batch))
            out.append((loss, acc) + reference_baselines(samples, seed))
        return out

    group(), reference()   # warm-up: kernels loaded, allocator primed
    tg, tr, res_g, res_r = [], [], None, None
    for _ in range(args.repeats):   # alternate the two sides repeat by repeat
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res_g = group()
        torch.cuda.synchronize()
        tg.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        res_r = reference()
        torch.cuda.synchronize()
        tr.append(time.perf_counter() - t0)
    for g, (loss, acc, rnd, hyb) in zip(res_g, res_r):
        assert g.random == rnd and g.hybrid == hyb, "baselines differ from the host loop"
        assert abs(g.gcnn - acc) <= 1e-6 and abs(g.loss - loss) <= 1e-6 * abs(loss), "gcnn / loss differ from tester.process"
    row = dict(samples=args.samples, models=args.models, batch=args.batch, cuts=int(store.offsets[2, -1]), repeats=args.repeats,
               test_group_s=statistics.median(tg), reference_s=statistics.median(tr),
               speedup=statistics.median(tr) / statistics.median(tg), test_group_all_s=tg, reference_all_s=tr,
               results=[dict(loss=g.loss, gcnn=g.gcnn, hybrid=g.hybrid, random=g.random) for g in res_g])
    line = json.dumps(row)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
