"""Latency of the separation rounds of several resident LPs that wait at the same time (a scoring server's situation: every solver
worker keeps its own LP, `ScoringClient.open_lp`).  On sample 0 of the four problems (`synthetic.make_lp_snapshot`), for n = 1, 2,
4, 8 sessions of the same shape, alternating in one process after warm-up:
  (a) n solo calls in sequence, `sess.select_cuts(round, forced, append=10 rows)` (gcnn_lp_round_append each): what serving the
      sessions one call per round costs;
  (b) one `LPSessionGroup.select_cuts` of the same n rounds (gcnn_lp_rounds, csrc/k_lprounds.hpp).
The sessions are in a loop's steady state (they have appended twice; raw buffers and both derived sets have their capacity); before
each timed call, outside the clock, they are brought to that state again, so every repetition appends to the same resident state.
Medians and interquartile ranges over --reps calls, host clock around call + sync (the calls synchronise themselves), profiler off;
launches and upload bytes per arm; the host-side phases pack / enqueue / wait (arm (a): summed over its n calls).
Usage: python tools/lp_rounds_latency.py [--reps N] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.infer import LPSessionGroup  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402

SIZES = (1, 2, 4, 8)
WARM = 2


def quartiles(x):
    q1, q2, q3 = np.percentile(np.asarray(x) * 1e6, [25, 50, 75])
    return q2, q3 - q1


def ten_rows(snap):
    """Ten of the snapshot's cuts as rows: what a selection would have kept."""
    ptr, col, val = np.asarray(snap.cut_ptr), np.asarray(snap.cut_col), np.asarray(snap.cut_val)
    n = min(10, ptr.shape[0] - 1)
    return lpstate.LPRowBlock(ptr[:n + 1].astype(np.int32), col[:ptr[n]].astype(np.int32), val[:ptr[n]].astype(np.float64),
                              np.asarray(snap.cut_lhs)[:n].astype(np.float64), np.asarray(snap.cut_rhs)[:n].astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 50)
    dev = torch.device("cuda", 0)
    m = GCNN(device=dev, seed=0)
    group = LPSessionGroup(dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"microseconds; median (interquartile range) of {reps} calls, the two arms alternating; host clock around call(s) + sync")
    say("(a) n solo select_cuts(round, forced, append=10 rows) in sequence   (b) one LPSessionGroup.select_cuts of the same n rounds")
    meets = {}
    for problem in synthetic.PROBLEMS:
        snap = synthetic.make_lp_snapshot(problem, 0)
        rows, base_round = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
        block = ten_rows(snap)
        n_new = np.asarray(block.row_lhs).shape[0]
        V = np.asarray(snap.col_type).shape[0]
        forced = (np.array([[0, 0, 1], [0, min(2, V - 1), min(1, V - 1)]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)

        def round_for(k):
            return lpstate.LPRound(**{**base_round.__dict__, "row_dual": np.concatenate([base_round.row_dual, np.zeros(k * n_new)]),
                                      "row_basis": np.concatenate([base_round.row_basis, np.ones(k * n_new, np.int8)])})

        rnd = round_for(WARM + 1)
        sessions = {"a": [None] * max(SIZES), "b": [None] * max(SIZES)}

        def reopen(arm, n):
            for i in range(n):
                if sessions[arm][i] is not None:
                    sessions[arm][i].close()
                s = sessions[arm][i] = m.open_lp(rows, deep=False)
                s.select_cuts(base_round)           # the optional column arrays are resident, the arena has its size
                for k in range(1, WARM + 1):
                    s.select_cuts(round_for(k), append=block)
            torch.cuda.synchronize()

        def arm_a(n, timings=None):
            out = []
            for s in sessions["a"][:n]:
                ph = {} if timings is not None else None
                out.append(s.select_cuts(rnd, forced, timings=ph, append=block))
                if ph is not None:
                    timings.append([ph["pack"], ph["enqueue"], ph["wait"]])
            return out

        def arm_b(n, timings=None):
            return group.select_cuts(sessions["b"][:n], [rnd] * n, [forced] * n, appends=[block] * n, timings=timings)

        _, dims = lpstate.check_snapshot(snap, deep=False)
        say(f"{problem}: rows {dims['n_rows'] + WARM * n_new} + {n_new}, columns {dims['n_cols']}, cuts {dims['n_cuts']}")
        meets[problem] = []
        for n in SIZES:
            reopen("a", n); reopen("b", n)
            solo_bytes = sessions["a"][0].upload_bytes(rnd, (np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.float32)), append=block)
            ra, rb = arm_a(n), arm_b(n)
            for x, y in zip(ra, rb):
                assert np.array_equal(x.order, y.order) and x.n_kept == y.n_kept and np.array_equal(x.scores, y.scores)
            times = {"a": [], "b": []}
            for i in range(reps + 10):
                for arm, fn in (("a", arm_a), ("b", arm_b)):
                    reopen(arm, n)
                    t0 = time.perf_counter()
                    fn(n)
                    if i >= 10:
                        times[arm].append(time.perf_counter() - t0)
            phases = {"a": [], "b": []}
            for _ in range(reps):
                reopen("a", n); reopen("b", n)
                pa, pb = [], {}
                arm_a(n, pa)
                arm_b(n, pb)
                phases["a"].append(np.sum(pa, 0))
                phases["b"].append([pb["pack"], pb["enqueue"], pb["wait"]])
            launches = {}
            for arm, fn in (("a", arm_a), ("b", arm_b)):
                reopen(arm, n)
                with _lib.launch_profile() as prof:
                    fn(n)
                launches[arm] = len(prof.launches)
            upload = {"a": n * solo_bytes, "b": pb["upload_bytes"]}
            med = {}
            for arm in "ab":
                med[arm], iqr = quartiles(times[arm])
                p = np.median(phases[arm], 0) * 1e6
                say(f"  n={n}  ({arm}) {med[arm]:8.1f} ({iqr:6.1f})   launches {launches[arm]:3d}   upload {upload[arm]:10,d} B"
                    f"   pack {p[0]:7.1f}  enqueue {p[1]:7.1f}  wait {p[2]:7.1f}")
            say(f"  n={n}  (b) / (a) = {med['b'] / med['a']:.3f}   (a) - (b) = {med['a'] - med['b']:.1f} us")
            if n >= 2:
                meets[problem].append(med["b"] < med["a"])
        for arm in sessions:
            for s in sessions[arm]:
                if s is not None:
                    s.close()
    say("aim ((b) below (a) from n = 2 on): " + ", ".join(f"{p} {'met' if all(v) else 'NOT met'}" for p, v in meets.items()))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
