"""PreNorm pretraining of a group against solo runs: one `trainer.pretrain_many` of S models (default 5) against S solo
`trainer.pretrain` runs, and S = 1 against `pretrain`, on synthetic setcov samples in a `SampleStore` (default 100 pretraining
samples, batches of 2, as model_trainer pretrains on every tenth training file with pretrain_batch_size = 2).  Every result is
checked bit for bit against the solo run.  Wall-clock medians over interleaved repeats (each run ends with a host sync), in total
and per pass (11 PreNorm layers: 11 passes), and the launches per group call from a run with one batch per pass.
Usage: python tools/pretrain_group.py [--samples N] [--models S] [--batch B] [--repeats R] [--out FILE]"""
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

from gcnn_cut_selector_amd import _lib, synthetic  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402
from gcnn_cut_selector_amd.store import SampleStore  # noqa: E402
from gcnn_cut_selector_amd.trainer import _StoreBatches, pretrain, pretrain_many  # noqa: E402

PASSES = 11


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def same(a, b):
    if not torch.equal(a.flat_parameters.detach().view(torch.int32), b.flat_parameters.detach().view(torch.int32)):
        return False
    return all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for x, y in zip(a._prenorm_state, b._prenorm_state)
               for k in ("count", "mean", "var"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--models", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    store = SampleStore.from_samples([synthetic.make_sample("setcov", i) for i in range(args.samples)], dev)
    loader = _StoreBatches(store, np.arange(len(store)), args.batch)
    n = args.models
    solo = [GCNN(device=dev, seed=i) for i in range(n)]
    grp = [GCNN(device=dev, seed=i) for i in range(n)]

    sides = {
        "solo_S": lambda: [pretrain(m, loader) for m in solo],
        "group_S": lambda: pretrain_many(grp, [loader] * n),
        "solo_1": lambda: [pretrain(solo[0], loader)],
        "group_1": lambda: pretrain_many(grp[:1], [loader]),
    }
    for fn in sides.values():   # warm-up: kernels loaded, allocator and tables primed
        fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):   # alternate the sides repeat by repeat
        for k, fn in sides.items():
            t, layers = timed(fn)
            assert all(x == PASSES for x in layers), (k, layers)
            times[k].append(t)
        assert all(same(a, b) for a, b in zip(solo, grp)), "a group member differs from its solo run"
    with _lib.launch_profile() as prof:   # one batch per pass: one group call per pass
        pretrain_many(grp, [[store.batch(np.arange(args.batch))]] * n)
    launches = len(prof.launches)
    med = {k: statistics.median(v) for k, v in times.items()}
    row = dict(samples=args.samples, batch=args.batch, models=n, batches_per_pass=len(range(0, args.samples, args.batch)),
               edges_per_batch=int(store.batch(np.arange(args.batch)).batch.dims.n_cons_edges), repeats=args.repeats,
               total_s={k: med[k] for k in sides}, per_pass_ms={k: 1e3 * med[k] / PASSES for k in sides},
               speedup_S=med["solo_S"] / med["group_S"], speedup_1=med["solo_1"] / med["group_1"],
               launches_per_group_call=launches / PASSES, all_s=times)
    line = json.dumps(row)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
