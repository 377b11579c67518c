"""A resident LP scored by an ensemble: one separation round, M = 5 models, selection mode, end to end on the host.

  (a) session   LPEnsembleSession.select_cuts(round, forced): gcnn_lp_round_ensemble -- the rows stay on the device; one upload of
                the round, the round's two state launches once, the five forward passes as one group, k_ens_mean, the selection
                over the mean, one download.
  (b) one shot  what a user had before: ModelSet.select_cuts_lp_ensemble(keys, lpstate.assemble(rows, round), forced):
                gcnn_lp_ensemble -- every row uploaded again, the whole state and the by-variable order derived again.

Sample 7 of setcov and of capfac at full scale.  Per route the median of `--reps` rounds, five times over ("repeats"), the two
routes alternating in one process; perf_counter around the route, every download waited for.  Written down: both medians, the
run-to-run spread (max - min) of (b)'s five repeats, which is the margin the comparison is read with, the upload bytes of both and
the per-launch record of one round of each (`_lib.launch_profile`).  Where (a) is slower than (b) beyond that spread the table
says so and names the launches where the time goes.  Not measured: other M, the server, rounds with edits.
Usage: python tools/lp_ensemble_session.py [--reps N] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN, ModelSet  # noqa: E402

M = 5
REPEATS = 5


def median_us(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e6


def forced_rows(n_cols, n=3, per=2, seed=5):
    rng = np.random.default_rng(seed)
    cols = np.concatenate([np.sort(rng.choice(n_cols, size=per, replace=False)) for _ in range(n)])
    return (np.stack([np.repeat(np.arange(n), per), cols]).astype(np.int32), rng.standard_normal(n * per).astype(np.float32), n)


def by_name(launches):
    total = {}
    for name, ms in launches:
        total[name] = total.get(name, 0.0) + ms * 1e3
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    keys = [f"seed/{i}" for i in range(M)]
    mset = ModelSet({k: GCNN(device=dev, seed=i) for i, k in enumerate(keys)})
    lines = ["all times in microseconds, end to end on the host (perf_counter around the route, every download waited for); "
             f"M = {M}; selection mode with 3 forced rows; each figure the median of {args.reps} rounds; {REPEATS} repeats, the routes alternating"]
    for problem in ("setcov", "capfac"):
        snap = synthetic.make_lp_snapshot(problem, 7)
        rows, rnd = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
        sess = mset.open_lp_ensemble(keys, rows)
        forced = forced_rows(sess.n_cols)
        one_shot = mset.ensemble_session(lp=True)

        def route_a():
            return sess.select_cuts(rnd, forced)

        def route_b():
            return mset.select_cuts_lp_ensemble(keys, lpstate.assemble(rows, rnd), forced)

        for _ in range(10):
            a, b = route_a(), route_b()
        assert np.array_equal(np.asarray(a.scores), np.asarray(b.scores)) and np.array_equal(a.members, b.members)
        assert np.array_equal(a.order, b.order) and a.n_kept == b.n_kept and np.array_equal(a.cut_index, b.cut_index)
        t_a, t_b = [], []
        for _ in range(REPEATS):
            t_a.append(median_us(route_a, args.reps))
            t_b.append(median_us(route_b, args.reps))
        ta, tb = {}, {}
        sess.select_cuts(rnd, forced, timings=ta)
        before = one_shot.upload_bytes
        mset.select_cuts_lp_ensemble(keys, lpstate.assemble(rows, rnd), forced, timings=tb)
        up_a, up_b = int(ta["upload_bytes"]), int(one_shot.upload_bytes - before)
        with _lib.launch_profile() as prof_a:
            route_a()
        with _lib.launch_profile() as prof_b:
            route_b()
        spread = max(t_b) - min(t_b)
        diff = float(np.median(t_a)) - float(np.median(t_b))
        verdict = "no slower" if diff <= spread else "SLOWER by more than the spread"
        K = int(np.asarray(snap.cut_lhs).shape[0])
        lines += [
            f"{problem}: K = {K} cuts, {sess.n_rows} rows, {sess.n_cols} columns, kept {a.n_kept}",
            "  (a) session   " + " ".join(f"{t:8.1f}" for t in t_a) + f" | median {np.median(t_a):8.1f} | upload {up_a:9d} B | "
            + " ".join(f"{name} {ta[name] * 1e6:7.1f}" for name in ("pack", "enqueue", "wait")),
            "  (b) one shot  " + " ".join(f"{t:8.1f}" for t in t_b) + f" | median {np.median(t_b):8.1f} | upload {up_b:9d} B | "
            + " ".join(f"{name} {tb[name] * 1e6:7.1f}" for name in ("pack", "enqueue", "wait") if name in tb),
            f"  (a) - (b): {diff:+.1f}; spread of (b)'s repeats: {spread:.1f} -> the session is {verdict}",
            f"  (a), per launch ({len(prof_a.launches)} launches): " + " ".join(f"{n} {ms * 1e3:.1f}" for n, ms in prof_a.launches),
            f"  (b), per launch ({len(prof_b.launches)} launches): " + " ".join(f"{n} {ms * 1e3:.1f}" for n, ms in prof_b.launches),
        ]
        if diff > spread:
            sa, sb = by_name(prof_a.launches), by_name(prof_b.launches)
            worse = sorted(((sa[n] - sb.get(n, 0.0), n) for n in sa if sa[n] > sb.get(n, 0.0)), reverse=True)[:4]
            lines.append("  where (a)'s launches take longer: " + " ".join(f"{n} {d:+.1f}" for d, n in worse))
        sess.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
