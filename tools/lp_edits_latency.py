"""Latency of separation rounds that append AND remove rows, for several resident LPs that wait at the same time (a scoring
server's situation once the workers' solvers clean their LPs between rounds).  On sample 0 of the four problems
(`synthetic.make_lp_snapshot`), for n = 1, 2, 4, 8 sessions of the same shape, the arms alternating in one process after warm-up:
  (a) n solo calls in sequence, `sess.select_cuts(round, forced, append=10 rows, remove=10 rows)` (gcnn_lp_round_remove each): what
      an `LPSessionGroup` without `batch_removes` does with such members;
  (b) one `LPSessionGroup(batch_removes=True).select_cuts` of the same n rounds (gcnn_lp_rounds_edit, csrc/k_lpedits.hpp);
  (c) through a `ScoringServer`, n clients (threads of this process, released together) that do what a worker had to do for a removed
      row before removals were served: close + open on the rows it holds now + the round.
The sessions are in a loop's steady state: every timed call appends ten rows and removes the ten that the call before appended, so
the resident rows are the same before every repetition and nothing has to be set up again between them.
Medians and interquartile ranges over --reps calls, host clock around call + sync (the calls synchronise themselves), profiler off;
launches and upload bytes per arm; the host-side phases pack / enqueue / wait (arm (a): summed over its n calls).
Usage: python tools/lp_edits_latency.py [--reps N] [--out FILE]"""
import argparse
import os
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, serve, synthetic  # noqa: E402
from gcnn_cut_selector_amd.infer import LPSessionGroup  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402

SIZES = (1, 2, 4, 8)


def quartiles(x):
    q1, q2, q3 = np.percentile(np.asarray(x) * 1e6, [25, 50, 75])
    return q2, q3 - q1


def ten_rows(snap):
    """Ten of the snapshot's cuts as rows: what a selection would have kept."""
    ptr, col, val = np.asarray(snap.cut_ptr), np.asarray(snap.cut_col), np.asarray(snap.cut_val)
    n = min(10, ptr.shape[0] - 1)
    return lpstate.LPRowBlock(ptr[:n + 1].astype(np.int32), col[:ptr[n]].astype(np.int32), val[:ptr[n]].astype(np.float64),
                              np.asarray(snap.cut_lhs)[:n].astype(np.float64), np.asarray(snap.cut_rhs)[:n].astype(np.float64))


class Clients:
    """n clients of one server, each on a thread of its own, released together for one step; `step` returns when all are done."""

    def __init__(self, address, n, rows, first):
        self.n, self.rows = n, rows
        self.clients = [serve.ScoringClient(address, "m") for _ in range(n)]
        self.sessions = [c.open_lp(rows, deep=False) for c in self.clients]
        for s in self.sessions:
            s.select_cuts(first)
        self.go, self.done, self.job, self.errors = threading.Barrier(n + 1), threading.Barrier(n + 1), None, []
        self.threads = [threading.Thread(target=self._loop, args=(i,), daemon=True) for i in range(n)]
        for t in self.threads:
            t.start()

    def _loop(self, i):
        while True:
            self.go.wait()
            if self.job is None:
                return
            try:
                rnd, forced = self.job
                self.sessions[i].close()
                self.sessions[i] = self.clients[i].open_lp(self.rows, deep=False)
                self.sessions[i].select_cuts(rnd, forced)
            except Exception as exc:  # noqa: BLE001
                self.errors.append(exc)
            self.done.wait()

    def step(self, rnd, forced):
        self.job = (rnd, forced)
        self.go.wait()
        self.done.wait()
        if self.errors:
            raise self.errors[0]

    def close(self):
        self.job = None
        self.go.wait()
        for s in self.sessions:
            s.close()
        for c in self.clients:
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 50)
    dev = torch.device("cuda", 0)
    m = GCNN(device=dev, seed=0)
    group = LPSessionGroup(dev, batch_removes=True)
    address = os.path.join(tempfile.mkdtemp(prefix="gcnn_lp_edits_"), "sock")
    server = serve.ScoringServer({"m": m}, address).start()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"microseconds; median (interquartile range) of {reps} calls, the arms alternating; host clock around call(s) + sync; one run on one box")
    say("(a) n solo select_cuts(round, forced, append=10 rows, remove=10 rows) in sequence   (b) one LPSessionGroup(batch_removes=True).select_cuts of the same")
    say("(c) through the server, n clients released together: close + open + select_cuts(round, forced) each")
    meets = {}
    for problem in synthetic.PROBLEMS:
        snap = synthetic.make_lp_snapshot(problem, 0)
        rows, base_round = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
        block = ten_rows(snap)
        n_new = np.asarray(block.row_lhs).shape[0]
        R0 = np.asarray(rows.row_lhs).shape[0]
        V = np.asarray(snap.col_type).shape[0]
        forced = (np.array([[0, 0, 1], [0, min(2, V - 1), min(1, V - 1)]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
        rnd = lpstate.LPRound(**{**base_round.__dict__, "row_dual": np.concatenate([base_round.row_dual, np.zeros(n_new)]),
                                  "row_basis": np.concatenate([base_round.row_basis, np.ones(n_new, np.int8)])})
        remove = R0 + np.arange(n_new)               # the rows the call before appended: the resident rows repeat
        steady = lpstate.rows_with(rows, block)

        def opened(n):
            out = []
            for _ in range(n):
                s = m.open_lp(rows, deep=False)
                s.select_cuts(base_round)           # the optional column arrays are resident, the arena has its size
                s.select_cuts(rnd, append=block)
                for _ in range(4):                  # every set of buffers (both parities, the transit set, both raw sets) has its capacity
                    s.select_cuts(rnd, forced, append=block, remove=remove)
                out.append(s)
            torch.cuda.synchronize()
            return out

        def arm_a(ss, timings=None):
            out = []
            for s in ss:
                ph = {} if timings is not None else None
                out.append(s.select_cuts(rnd, forced, timings=ph, append=block, remove=remove))
                if ph is not None:
                    timings.append([ph["pack"], ph["enqueue"], ph["wait"]])
            return out

        def arm_b(ss, timings=None):
            n = len(ss)
            return group.select_cuts(ss, [rnd] * n, [forced] * n, appends=[block] * n, removes=[remove] * n, timings=timings)

        _, dims = lpstate.check_snapshot(snap, deep=False)
        say(f"{problem}: rows {R0 + n_new} + {n_new} - {n_new}, columns {dims['n_cols']}, cuts {dims['n_cuts']}")
        meets[problem] = []
        for n in SIZES:
            sa, sb = opened(n), opened(n)
            clients = Clients(address, n, steady, rnd)
            solo_bytes = sa[0].upload_bytes(rnd, (np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.float32)), append=block, remove=remove)
            for x, y in zip(arm_a(sa), arm_b(sb)):
                assert np.array_equal(x.order, y.order) and x.n_kept == y.n_kept and np.array_equal(x.scores, y.scores)
            assert group.solo_rounds == 0
            fns = {"a": lambda: arm_a(sa), "b": lambda: arm_b(sb), "c": lambda: clients.step(rnd, forced)}
            times = {arm: [] for arm in fns}
            for i in range(reps + 10):
                for arm, fn in fns.items():
                    t0 = time.perf_counter()
                    fn()
                    if i >= 10:
                        times[arm].append(time.perf_counter() - t0)
            phases = {"a": [], "b": []}
            for _ in range(reps):
                pa, pb = [], {}
                arm_a(sa, pa)
                arm_b(sb, pb)
                phases["a"].append(np.sum(pa, 0))
                phases["b"].append([pb["pack"], pb["enqueue"], pb["wait"]])
            launches = {}
            for arm, fn in (("a", fns["a"]), ("b", fns["b"])):
                with _lib.launch_profile() as prof:
                    fn()
                launches[arm] = len(prof.launches)
            upload = {"a": n * solo_bytes, "b": pb["upload_bytes"]}
            med = {}
            for arm in "ab":
                med[arm], iqr = quartiles(times[arm])
                p = np.median(phases[arm], 0) * 1e6
                say(f"  n={n}  ({arm}) {med[arm]:8.1f} ({iqr:6.1f})   launches {launches[arm]:3d}   upload {upload[arm]:10,d} B"
                    f"   pack {p[0]:7.1f}  enqueue {p[1]:7.1f}  wait {p[2]:7.1f}")
            med["c"], iqr = quartiles(times["c"])
            say(f"  n={n}  (c) {med['c']:8.1f} ({iqr:6.1f})")
            say(f"  n={n}  (b) / (a) = {med['b'] / med['a']:.3f}   (a) - (b) = {med['a'] - med['b']:.1f} us   (c) / (b) = {med['c'] / med['b']:.2f}")
            if n >= 2:
                meets[problem].append(med["b"] < med["a"])
            clients.close()
            for s in sa + sb:
                s.close()
    say("aim ((b) below (a) from n = 2 on): " + ", ".join(f"{p} {'met' if all(v) else 'NOT met'}" for p, v in meets.items()))
    server.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
