"""Latency of selecting cuts from raw LP snapshots that belong to DIFFERENT models: what a scoring server holds when the evaluators'
task farm runs `seed` innermost (model_evaluator.py:211-219) and the workers send `LPSnapshot`s.  For M = 1, 2, 5, 8 models with one
setcov snapshot each, and for 5 models x 4 snapshots, alternating in one process:
  (a) one ModelSet.select_cuts_lp_many call (gcnn_lp_models: one upload, two launches build every state, the models' forward
      passes as a group, one selection launch pair, one download);
  (b) M GCNN.select_cuts_lp_many calls, one per model on its own snapshots (what a server that groups by model does);
  (c) one GCNN.select_cuts_lp call per snapshot.
Medians over --reps rounds after warm-up, host clock around the calls including their syncs, in --runs runs one after the other
(the spread between the runs is what a ratio has to beat); per path the launches.
Usage: python tools/lp_models_latency.py [--reps N] [--runs N] > profiles/lp_models.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, synthetic  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN, ModelSet  # noqa: E402

CASES = ((1, 1), (2, 1), (5, 1), (8, 1), (5, 4))      # (models, snapshots per model)
SELECT = dict(p_max=0.1, p_max_ub=0.5, max_selected=10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    models = {f"setcov/{i}": GCNN(device=dev, seed=i) for i in range(8)}
    names = list(models)
    pool = [synthetic.make_lp_snapshot("setcov", i) for i in range(20)]
    s0 = pool[0]
    print(f"microseconds per round; median of {args.reps} rounds, the three paths alternating; host clock around the calls including "
          f"their syncs; {args.runs} runs.  setcov: snapshot 0 has R={s0.row_lhs.shape[0]} V={s0.col_type.shape[0]} K={s0.cut_lhs.shape[0]}")
    for M, per in CASES:
        used = names[:M]
        mset = ModelSet({n: models[n] for n in used})
        keys = [used[i % M] for i in range(M * per)]          # interleaved, as requests arrive
        snaps = pool[:M * per]
        mine = {n: [s for key, s in zip(keys, snaps) if key == n] for n in used}
        paths = {"a": lambda: mset.select_cuts_lp_many(keys, snaps, **SELECT),
                 "b": lambda: [models[n].select_cuts_lp_many(mine[n], **SELECT) for n in used],
                 "c": lambda: [models[key].select_cuts_lp(s, **SELECT) for key, s in zip(keys, snaps)]}
        launches = {}
        for run in range(args.runs):
            times = {p: [] for p in paths}
            for i in range(args.reps + 5):
                for p, fn in paths.items():
                    t0 = time.perf_counter()
                    fn()
                    if i >= 5:
                        times[p].append(time.perf_counter() - t0)
            for p, fn in paths.items():
                with _lib.launch_profile() as prof:
                    fn()
                launches[p] = len(prof.launches)
            a, b, c = (float(np.median(times[p])) * 1e6 for p in "abc")
            print(f"  M={M} x {per} snapshot(s)  run {run + 1}  (a) {a:8.1f}  (b) {b:8.1f}  (c) {c:8.1f}   (b)/(a) {b / a:5.2f}   "
                  f"(c)/(a) {c / a:5.2f}   per snapshot (a) {a / (M * per):7.1f}   launches (a) {launches['a']} (b) {launches['b']} "
                  f"(c) {launches['c']}")
        assert mset.calls and mset.max_models_per_call == M, "path (a) did not go through gcnn_lp_models"


if __name__ == "__main__":
    main()
