"""Latency of one separation round's cut selection with the LP resident on the device against the full-snapshot call.  On one
snapshot per problem (`synthetic.make_lp_snapshot`, the four BASELINE shapes), alternating in one process:
  (a) GCNN.select_cuts_lp(full snapshot): the whole LP goes up, its state and the constraint edges' plan are built every call;
  (b) LPSession.select_cuts(round) after one GCNN.open_lp(rows): the solve and the cuts go up, the rows stay.
Medians and interquartile ranges over --reps calls after warm-up, host clock around call + sync (the calls synchronise
themselves); launches per call and upload bytes of both; the host-side phases pack / enqueue / wait as tools/latency.py splits
them; and what a session costs besides its rounds: open_lp, and one append_rows of 10 rows.
Usage: python tools/lp_session_latency.py [--reps N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.infer import normalize_forced  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402


def quartiles(x):
    q1, q2, q3 = np.percentile(np.asarray(x) * 1e6, [25, 50, 75])
    return q2, q3 - q1


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    reps = max(ap.parse_args().reps, 50)
    m = GCNN(device=torch.device("cuda", 0), seed=0)
    print("microseconds; median (interquartile range) of", reps, "calls, (a) and (b) alternating; host clock around call + sync")
    for problem in synthetic.PROBLEMS:
        snap = synthetic.make_lp_snapshot(problem, 0)
        rows, rnd = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
        sess = m.open_lp(rows, deep=False)
        m._lp().deep_check = False
        paths = {"a": lambda: m.select_cuts_lp(snap), "b": lambda: sess.select_cuts(rnd)}
        ra, rb = paths["a"](), paths["b"]()
        assert np.array_equal(ra.order, rb.order) and ra.n_kept == rb.n_kept and np.array_equal(ra.scores, rb.scores)
        times = {k: [] for k in paths}
        for i in range(reps + 10):
            for k, fn in paths.items():
                t0 = time.perf_counter()
                fn()
                if i >= 10:
                    times[k].append(time.perf_counter() - t0)
        none = normalize_forced(None, sess.n_cols)
        ph_a, ph_b, phases = {}, {}, {"a": [], "b": []}
        for _ in range(reps):
            m._lp().run(snap, True, ph_a, none, 0.1, 0.5)
            sess.select_cuts(rnd, timings=ph_b)
            phases["a"].append([ph_a["pack"], ph_a["enqueue"], ph_a["wait"]])
            phases["b"].append([ph_b["pack"], ph_b["enqueue"], ph_b["wait"]])
        launches = {}
        for k, fn in paths.items():
            with _lib.launch_profile() as prof:
                fn()
            launches[k] = [n for n, _ in prof.launches]
        _, dims = lpstate.check_snapshot(snap, deep=False)
        print(f"{problem}: rows {dims['n_rows']} (entries {dims['row_nnz']}), columns {dims['n_cols']}, cuts {dims['n_cuts']}")
        for k, label, nbytes in (("a", "(a) select_cuts_lp(snapshot)", ph_a["upload_bytes"]), ("b", "(b) session.select_cuts(round)", ph_b["upload_bytes"])):
            med, iqr = quartiles(times[k])
            p = np.median(phases[k], 0) * 1e6
            print(f"  {label:32s} {med:8.1f} ({iqr:5.1f})   launches {len(launches[k]):2d}   upload {nbytes:9,d} B   "
                  f"pack {p[0]:6.1f}  enqueue {p[1]:6.1f}  wait {p[2]:6.1f}")
        print(f"  (b) / (a) = {np.median(times['b']) / np.median(times['a']):.3f}; launches of (b): {', '.join(launches['b'][:2])} + "
              f"{len(launches['b']) - 2} of the forward pass and the selection")
        # what a session costs besides its rounds
        opens = timed(lambda: m.open_lp(rows, deep=False).close(), 10)
        ten = (np.arange(11, dtype=np.int32) * 3, np.tile(np.arange(3, dtype=np.int32), 10), np.ones(30), np.full(10, -1e20), np.ones(10))
        appends = []
        for _ in range(10):
            s2 = m.open_lp(rows, deep=False)
            appends += timed(lambda: s2.append_rows(*ten), 1)
            s2.close()
        print(f"  open_lp {quartiles(opens)[0]:8.1f} ({quartiles(opens)[1]:5.1f})   append_rows of 10 rows {quartiles(appends)[0]:8.1f} "
              f"({quartiles(appends)[1]:5.1f})   [medians of 10; both synchronise]")
        sess.close()


if __name__ == "__main__":
    main()
