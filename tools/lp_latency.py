"""Latency of scoring from a raw LP snapshot.  On one snapshot per problem, alternating in one process:
  (a) what a user could do before the device path existed: the vectorised host restatement of get_state's arithmetic
      (tests/lpstate_restate.py) followed by GCNN.score_state;
  (b) GCNN.score_lp: one upload of the packed snapshot, the state built on the device, the same forward pass;
and GCNN.score_state alone on the prebuilt state.  Medians and interquartile ranges over --reps calls after warm-up, host clock
around call + sync; the host-side phases (pack / enqueue / wait) of (b) and of score_state; the launches of both; the upload bytes.
Usage: python tools/lp_latency.py [--reps N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lpstate_restate as R  # noqa: E402
from gcnn_cut_selector_amd import _lib, synthetic  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402


def quartiles(x):
    q1, q2, q3 = np.percentile(np.asarray(x) * 1e6, [25, 50, 75])
    return q2, q3 - q1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    reps = max(args.reps, 200)
    m = GCNN(device=torch.device("cuda", 0), seed=0)
    print("microseconds; median (interquartile range) of", reps, "calls, the three paths alternating; host clock around call + sync")
    for problem in synthetic.PROBLEMS:
        snap = synthetic.make_lp_snapshot(problem, 7)
        state, _ = m.state_from_lp(snap)
        paths = {"a": lambda: m.score_state(R.host_state(snap)), "b": lambda: m.score_lp(snap), "s": lambda: m.score_state(state)}
        times = {k: [] for k in paths}
        for i in range(reps + 10):
            for k, fn in paths.items():
                t0 = time.perf_counter()
                fn()
                if i >= 10:
                    times[k].append(time.perf_counter() - t0)
        t_host = []
        for _ in range(20):
            t0 = time.perf_counter()
            R.host_state(snap)
            t_host.append(time.perf_counter() - t0)
        ph_b, ph_s = {}, {}
        phases_b, phases_s = [], []
        for _ in range(50):
            m._lp().run(snap, False, ph_b)
            m._session.run(state, False, ph_s)
            phases_b.append([ph_b["pack"], ph_b["enqueue"], ph_b["wait"]])
            phases_s.append([ph_s["pack"], ph_s["enqueue"], ph_s["wait"]])
        pb, ps = np.median(phases_b, 0) * 1e6, np.median(phases_s, 0) * 1e6
        with _lib.launch_profile() as lb:
            m.score_lp(snap)
        with _lib.launch_profile() as ls:
            m.score_state(state)
        extra = [(n, ms * 1e3) for n, ms in lb.launches if n.startswith("k_lp_")]
        (a, a_iqr), (b, b_iqr), (s, s_iqr) = (quartiles(times[k]) for k in "abs")
        C, V, K, E1, E2 = (int(x) for x in (state[7], state[8], state[9], state[1].shape[1], state[5].shape[1]))
        L = m._session.layouts[(C, V, K, E1, E2)][1]
        print(f"{problem:8s} C={C} V={V} K={K} E1={E1} E2={E2}")
        print(f"  (a) host restatement + score_state {a:9.1f} ({a_iqr:6.1f})   [restatement alone {np.median(t_host) * 1e6:9.1f}]")
        print(f"  (b) score_lp                       {b:9.1f} ({b_iqr:6.1f})   pack {pb[0]:6.1f} enqueue {pb[1]:6.1f} wait {pb[2]:6.1f}")
        print(f"      score_state on the built state {s:9.1f} ({s_iqr:6.1f})   pack {ps[0]:6.1f} enqueue {ps[1]:6.1f} wait {ps[2]:6.1f}")
        print(f"  (b) - score_state {b - s:+8.1f}; (a) - (b) {a - b:+9.1f} vs IQR of (a) {a_iqr:.1f}: {'below' if a - b > a_iqr else 'NOT below'}")
        print(f"  launches: score_lp {len(lb.launches)}, score_state {len(ls.launches)}, extra {len(extra)}: "
              + ", ".join(f"{n} {us:.1f}" for n, us in extra) + f" (event brackets) | upload bytes: score_lp {ph_b['upload_bytes']}, "
              f"score_state {int(L.in_bytes)}")


if __name__ == "__main__":
    main()
