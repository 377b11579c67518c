"""Latency of a separation round that first drops the rows the solver's clean-up removed (SCIP's loop: add the selected cuts,
re-solve, clean the LP -- slack cuts of earlier rounds leave again -- and ask again).  On sample 0 of the four problems
(`synthetic.make_lp_snapshot`), alternating in one process after warm-up:
  (a) GCNN.select_cuts_lp on the assembled snapshot of the kept rows;
  (b) what a session offered for a removed row before: close(), open_lp(rows_without(...)), select_cuts(round);
  (c) LPSession.select_cuts(round, remove=10 rows): the removal inside the round's call (csrc/k_lpremove.hpp);
  (d) LPSession.select_cuts(round, append=10 rows, remove=10 rows): both edits inside the round's call;
  (e) LPSession.select_cuts(round, append=10 rows): the append alone (the (d) arm of tools/lp_append_latency.py), and
  (p) a plain LPSession.select_cuts(round) on the same rows, so that (e) - (p) is what the append costs and (d) - (e) what the
      removal inside (d) costs.
(c), (d) and (e) run on sessions in a loop's steady state -- the resident rows are the LP plus ten cut rows, one call has already
carried both edits, so both raw sets, the transit set and both derived sets have their capacity; before each timed call, outside
the clock, the session is brought to that state again.  Medians and interquartile ranges over --reps calls, host clock around
call + sync (the calls synchronise themselves), profiler off; launches, upload bytes and the pack / enqueue / wait phases per arm;
and, in a run of their own, the per-launch times of the k_lpd_* kernels from `_lib.launch_profile`.
Usage: python tools/lp_remove_latency.py [--reps N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402
from lp_append_latency import quartiles, ten_rows  # noqa: E402

NO_FORCED = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    reps = max(ap.parse_args().reps, 50)
    m = GCNN(device=torch.device("cuda", 0), seed=0)
    print("microseconds; median (interquartile range) of", reps, "calls, the arms alternating; host clock around call + sync")
    for problem in synthetic.PROBLEMS:
        snap = synthetic.make_lp_snapshot(problem, 0)
        rows, base_round = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
        block = ten_rows(snap)
        n_new = np.asarray(block.row_lhs).shape[0]
        R = np.asarray(rows.row_lhs).shape[0]
        gone = R + np.arange(n_new)                         # the ten cut rows of the last round

        def round_for(k):
            return lpstate.LPRound(**{**base_round.__dict__, "row_dual": np.concatenate([base_round.row_dual, np.zeros(k * n_new)]),
                                      "row_basis": np.concatenate([base_round.row_basis, np.ones(k * n_new, np.int8)])})

        one, two = lpstate.rows_with(rows, block), lpstate.rows_with(rows, block, block)
        full = {"a": lpstate.assemble(rows, base_round), "d": lpstate.assemble(one, round_for(1)), "e": lpstate.assemble(two, round_for(2))}
        m._lp().deep_check = False
        plain = m.open_lp(one, deep=False)
        state = {}

        def reopen(key):
            if key in state:
                state[key].close()
            state[key] = s = m.open_lp(rows, deep=False)
            s.select_cuts(base_round)                       # the optional column arrays are resident, the arena has its size
            s.select_cuts(round_for(1), append=block)
            s.select_cuts(round_for(1), append=block, remove=gone)      # rows + ten cut rows; every buffer has its capacity

        def arm_b():
            state["b"].close()
            state["b"] = m.open_lp(lpstate.rows_without(one, gone), deep=False)
            return state["b"].select_cuts(base_round)

        arms = {"a": lambda: m.select_cuts_lp(full["a"]), "b": arm_b, "c": lambda: state["c"].select_cuts(base_round, remove=gone),
                "d": lambda: state["d"].select_cuts(round_for(1), append=block, remove=gone),
                "e": lambda: state["e"].select_cuts(round_for(2), append=block), "p": lambda: plain.select_cuts(round_for(1))}
        for k in "bcde":
            reopen(k)
        results = {k: fn() for k, fn in arms.items()}
        want = {"a": results["a"], "d": m.select_cuts_lp(full["d"]), "e": m.select_cuts_lp(full["e"])}
        for k, ref in (("b", "a"), ("c", "a"), ("d", "d"), ("e", "e"), ("p", "d")):
            assert np.array_equal(results[k].order, want[ref].order) and results[k].n_kept == want[ref].n_kept
            assert np.array_equal(results[k].scores, want[ref].scores)
        times = {k: [] for k in arms}
        for i in range(reps + 10):
            for k, fn in arms.items():
                if k in "cde":
                    reopen(k)
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 10:
                    times[k].append(time.perf_counter() - t0)
        calls = {"p": (plain, round_for(1), {}), "c": ("c", base_round, dict(remove=gone)), "d": ("d", round_for(1), dict(append=block, remove=gone)),
                 "e": ("e", round_for(2), dict(append=block))}
        phases = {k: [] for k in calls}
        for _ in range(reps):                               # the host-side phases
            for k, (sess, rnd, kw) in calls.items():
                if k != "p":
                    reopen(k)
                    sess = state[k]
                ph = {}
                sess.select_cuts(rnd, timings=ph, **kw)
                phases[k].append([ph["pack"], ph["enqueue"], ph["wait"]])
        launches, upload, lpd = {}, {}, []
        for k, fn in arms.items():
            if k in "cde":
                reopen(k)
            with _lib.launch_profile() as prof:
                fn()
            launches[k] = [n for n, _ in prof.launches]
        for _ in range(reps):                               # the removal's launches, in a run of their own (the profiler's events on)
            reopen("c")
            with _lib.launch_profile() as prof:
                state["c"].select_cuts(base_round, remove=gone)
            lpd.append([ms for n, ms in prof.launches if n.startswith("k_lpd_")])
        for k in "cde":
            reopen(k)
        _, dims_full = lpstate.check_snapshot(full["a"], deep=False)
        upload["a"] = int(lpstate.lp_layout(dims_full, 0, 0)[1].in_bytes)
        upload["b"] = state["b"].upload_bytes(base_round, NO_FORCED) + sum(
            a.nbytes for a in lpstate.check_rows(lpstate.rows_without(one, gone), False)[0])
        upload["c"] = state["c"].upload_bytes(base_round, NO_FORCED, remove=gone)
        upload["d"] = state["d"].upload_bytes(round_for(1), NO_FORCED, append=block, remove=gone)
        upload["e"] = state["e"].upload_bytes(round_for(2), NO_FORCED, append=block)
        upload["p"] = plain.upload_bytes(round_for(1), NO_FORCED)
        print(f"{problem}: rows {R} + {n_new} cut rows (entries {dims_full['row_nnz']} + the cut rows'), columns {dims_full['n_cols']}, "
              f"cuts {dims_full['n_cuts']}")
        labels = {"a": "(a) select_cuts_lp(snapshot)", "b": "(b) close + open_lp + select_cuts", "c": "(c) select_cuts(round, remove=10)",
                  "d": "(d) select_cuts(round, append=10, remove=10)", "e": "(e) select_cuts(round, append=10)",
                  "p": "(p) session.select_cuts(round)"}
        med = {}
        for k in arms:
            med[k], iqr = quartiles(times[k])
            p = np.median(phases[k], 0) * 1e6 if k in phases else None
            print(f"  {labels[k]:46s} {med[k]:8.1f} ({iqr:5.1f})   launches {len(launches[k]):2d}   upload {upload[k]:9,d} B"
                  + (f"   pack {p[0]:6.1f}  enqueue {p[1]:6.1f}  wait {p[2]:6.1f}" if p is not None else ""))
        print(f"  (c) / (b) = {med['c'] / med['b']:.3f}   (c) / (a) = {med['c'] / med['a']:.3f}   (c) - (p) = {med['c'] - med['p']:.1f} us   "
              f"removal inside (d): (d) - (e) = {med['d'] - med['e']:.1f} us   append inside it: (e) - (p) = {med['e'] - med['p']:.1f} us")
        names = [n for n in launches["c"] if n.startswith("k_lpd_")]
        per = np.median(np.asarray(lpd), 0) * 1e3
        print("  launches of (c): " + ", ".join(f"{n} {t:.1f}" for n, t in zip(names, per)) + f" us [device, median of {reps}], then "
              f"{len(launches['c']) - len(names)} of the round")
        for s in list(state.values()) + [plain]:
            s.close()


if __name__ == "__main__":
    main()
