"""Latency of a separation round that first appends the cuts the last round kept (SCIP's loop: add the selected cuts to the LP,
re-solve, ask again).  On sample 0 of the four problems (`synthetic.make_lp_snapshot`), alternating in one process after warm-up:
  (a) GCNN.select_cuts_lp on the assembled snapshot (all rows, the 10 appended ones included);
  (b) a plain LPSession.select_cuts(round): no append;
  (c) LPSession.append_rows(10 rows) by rebuild, then select_cuts(round): what a loop costs through the default path;
  (d) LPSession.select_cuts(round, append=the same 10 rows): the append inside the round's call (csrc/k_lpappend.hpp).
(c) and (d) run on sessions that hold the rows without the block and have already appended twice (a loop's steady state: the raw
buffers and both derived sets have their capacity, which grows by doubling); before each timed call, outside the clock, the session
is brought to that state again, so every repetition appends to the same resident state.  Medians and interquartile ranges over --reps calls, host clock
around call + sync (the calls synchronise themselves), profiler off; launches and upload bytes per arm; and, in a run of their own,
the per-launch times of the k_lpa_* kernels from `_lib.launch_profile`.
Usage: python tools/lp_append_latency.py [--reps N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402


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
    reps = max(ap.parse_args().reps, 50)
    m = GCNN(device=torch.device("cuda", 0), seed=0)
    print("microseconds; median (interquartile range) of", reps, "calls, the four arms alternating; host clock around call + sync")
    for problem in synthetic.PROBLEMS:
        snap = synthetic.make_lp_snapshot(problem, 0)
        rows, base_round = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
        block = ten_rows(snap)
        n_new = np.asarray(block.row_lhs).shape[0]

        def round_for(k):
            return lpstate.LPRound(**{**base_round.__dict__, "row_dual": np.concatenate([base_round.row_dual, np.zeros(k * n_new)]),
                                      "row_basis": np.concatenate([base_round.row_basis, np.ones(k * n_new, np.int8)])})

        WARM = 2
        after = lpstate.rows_with(rows, *([block] * (WARM + 1)))
        rnd = round_for(WARM + 1)
        full = lpstate.assemble(after, rnd)
        m._lp().deep_check = False
        plain = m.open_lp(after, deep=False)
        state = {}

        def reopen(key):
            if key in state:
                state[key].close()
            state[key] = m.open_lp(rows, deep=False)
            state[key].select_cuts(base_round)          # the optional column arrays are resident, the arena has its size
            for k in range(1, WARM + 1):
                if key == "c":
                    state[key].append_rows(*block.arrays())
                else:
                    state[key].select_cuts(round_for(k), append=block)

        def arm_c():
            state["c"].append_rows(*block.arrays())
            return state["c"].select_cuts(rnd)

        arms = {"a": lambda: m.select_cuts_lp(full), "b": lambda: plain.select_cuts(rnd), "c": arm_c,
                "d": lambda: state["d"].select_cuts(rnd, append=block)}
        reopen("c"); reopen("d")
        results = {k: fn() for k, fn in arms.items()}
        for k in "bcd":
            assert np.array_equal(results[k].order, results["a"].order) and results[k].n_kept == results["a"].n_kept
            assert np.array_equal(results[k].scores, results["a"].scores)
        times = {k: [] for k in arms}
        for i in range(reps + 10):
            for k, fn in arms.items():
                if k in "cd":
                    reopen(k)
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 10:
                    times[k].append(time.perf_counter() - t0)
        phases = {"b": [], "d": []}
        for _ in range(reps):                               # the host-side phases of (b) and (d)
            reopen("d")
            for k, sess, kw in (("b", plain, {}), ("d", state["d"], dict(append=block))):
                ph = {}
                sess.select_cuts(rnd, timings=ph, **kw)
                phases[k].append([ph["pack"], ph["enqueue"], ph["wait"]])
        launches, upload, lpa = {}, {}, []
        for k, fn in arms.items():
            if k in "cd":
                reopen(k)
            with _lib.launch_profile() as prof:
                fn()
            launches[k] = [n for n, _ in prof.launches]
        for _ in range(reps):                               # the append's launches, in a run of their own (the profiler's events on)
            reopen("d")
            with _lib.launch_profile() as prof:
                state["d"].select_cuts(rnd, append=block)
            lpa.append([ms for n, ms in prof.launches if n.startswith("k_lpa_")])
        reopen("d")
        _, dims_full = lpstate.check_snapshot(full, deep=False)
        upload["a"] = int(lpstate.lp_layout(dims_full, 0, 0)[1].in_bytes)
        upload["b"] = plain.upload_bytes(rnd, (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)))
        barrays = lpstate.check_row_block(*block.arrays(), plain.n_cols, 1e20, False)[0]
        upload["c"] = upload["b"] + lpstate.rows_upload_layout(n_new, barrays[1].shape[0], False)[1]
        upload["d"] = state["d"].upload_bytes(rnd, (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)), append=block)
        print(f"{problem}: rows {dims_full['n_rows'] - n_new} + {n_new} (entries {dims_full['row_nnz']}), columns {dims_full['n_cols']}, "
              f"cuts {dims_full['n_cuts']}")
        labels = {"a": "(a) select_cuts_lp(snapshot)", "b": "(b) session.select_cuts(round)", "c": "(c) append_rows (rebuild) + select_cuts",
                  "d": "(d) select_cuts(round, append=block)"}
        med = {}
        for k in arms:
            med[k], iqr = quartiles(times[k])
            p = np.median(phases[k], 0) * 1e6 if k in phases else None
            print(f"  {labels[k]:42s} {med[k]:8.1f} ({iqr:5.1f})   launches {len(launches[k]):2d}   upload {upload[k]:9,d} B"
                  + (f"   pack {p[0]:6.1f}  enqueue {p[1]:6.1f}  wait {p[2]:6.1f}" if p is not None else ""))
        print(f"  (d) - (b) = {med['d'] - med['b']:.1f} us (what an append costs now)   (d) / (c) = {med['d'] / med['c']:.3f}   "
              f"(d) / (a) = {med['d'] / med['a']:.3f}")
        names = [n for n in launches["d"] if n.startswith("k_lpa_")]
        per = np.median(np.asarray(lpa), 0) * 1e3
        print("  launches of (d): " + ", ".join(f"{n} {t:.1f}" for n, t in zip(names, per)) + f" us [device, median of {reps}], then "
              f"{len(launches['d']) - len(names)} of the round")
        for s in list(state.values()) + [plain]:
            s.close()


if __name__ == "__main__":
    main()
