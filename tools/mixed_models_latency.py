"""Latency of scoring states that belong to DIFFERENT models: what a scoring server holds when the evaluators' task farm runs
`seed` innermost (model_evaluator.py:211-219).  For M = 1, 2, 5, 8 models with one setcov state each, and for 5 models x 4 states,
alternating in one process:
  (a) one ModelSet.score_states call (gcnn_infer_models: one upload, the models' forward passes as a group, one download);
  (b) M GCNN.score_states calls, one per model on its own states (what a server that groups by model does);
  (c) one GCNN.score_state call per state.
Medians over --reps rounds after warm-up, host clock around the calls including their syncs; per path the launches.
Usage: python tools/mixed_models_latency.py [--reps N] > profiles/mixed_models.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, synthetic, utils  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN, ModelSet  # noqa: E402

CASES = ((1, 1), (2, 1), (5, 1), (8, 1), (5, 4))      # (models, states per model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    models = {f"setcov/{i}": GCNN(device=dev, seed=i) for i in range(8)}
    names = list(models)
    pool = [utils.state_to_inputs(synthetic.make_sample("setcov", i)[0]) for i in range(20)]
    c, v, k = pool[0][7:]
    print(f"microseconds per round; median of {args.reps} rounds, the three paths alternating; host clock around the calls including "
          f"their syncs.  setcov: state 0 has C={c} V={v} K={k}")
    for M, per in CASES:
        used = names[:M]
        mset = ModelSet({n: models[n] for n in used})
        keys = [used[i % M] for i in range(M * per)]          # interleaved, as requests arrive
        states = pool[:M * per]
        mine = {n: [s for key, s in zip(keys, states) if key == n] for n in used}
        paths = {"a": lambda: mset.score_states(keys, states),
                 "b": lambda: [models[n].score_states(mine[n]) for n in used],
                 "c": lambda: [models[key].score_state(s) for key, s in zip(keys, states)]}
        times = {p: [] for p in paths}
        for i in range(args.reps + 5):
            for p, fn in paths.items():
                t0 = time.perf_counter()
                fn()
                if i >= 5:
                    times[p].append(time.perf_counter() - t0)
        launches = {}
        for p, fn in paths.items():
            with _lib.launch_profile() as prof:
                fn()
            launches[p] = len(prof.launches)
        a, b, c_ = (float(np.median(times[p])) * 1e6 for p in "abc")
        print(f"  M={M} x {per} state(s)  (a) {a:8.1f}  (b) {b:8.1f}  (c) {c_:8.1f}   (b)/(a) {b / a:5.2f}   (c)/(a) {c_ / a:5.2f}   "
              f"per state (a) {a / (M * per):7.1f}   launches (a) {launches['a']} (b) {launches['b']} (c) {launches['c']}")


if __name__ == "__main__":
    main()
