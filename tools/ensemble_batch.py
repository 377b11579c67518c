"""Ensembles over many states: S states scored by M = 5 models, mean and selection per state -- host arrays in, selections out, end to end.

  (a) one call   ModelSet.select_cuts_ensemble_many(keys, states, forced): gcnn_infer_ensemble_batch -- one upload of the S states as
                 one union, one graph plan, the five forward passes over the union as one group, the mean, the selection of every
                 state, one download.
  (b) S calls    what there was before: S calls of ModelSet.select_cuts_ensemble(keys, state, forced) (gcnn_infer_ensemble), each with
                 its own upload, graph plan, 12-launch chain and download.

The states are S copies of sample 7 of the problem at full scale, each with 3 forced rows.  S = 1, 4, 16.  The two routes alternate
call by call in one process; per route the median of `--reps` calls, five times over ("repeats").  Host clock around the route, every
download waited for.  The margin a difference is read with is the run-to-run spread (max - min) of route (b)'s five repeats.

Then the rank-mode tail at S = 16, setcov, under the library's event brackets (`_lib.launch_profile`): k_eb_mean_rank, the one launch
of gcnn_infer_ensemble_batch, against k_ens_mean over the same K_total (ops.ensemble_mean on the call's member rows) plus k_ib_rank
over the same segments (GCNN.score_states(states, rank=True)) -- the two dependent launches it stands for.  Their sum leaves out the
gap between two dependent launches, so it flatters the pair.
Usage: python tools/ensemble_batch.py [--reps N] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, ops, synthetic, utils  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN, ModelSet  # noqa: E402

M = 5
REPEATS = 5
SIZES = (1, 4, 16)
N_FORCED = 3


def forced_rows(rng, state):
    """N_FORCED forced rows, each on the support of one of the state's cuts."""
    rows, cols, vals = [], [], []
    for r in range(N_FORCED):
        sup = state[5][1][state[5][0] == (r * 7) % state[9]]
        x = rng.standard_normal(len(sup))
        rows += [r] * len(sup)
        cols += list(sup)
        vals += list(x / np.linalg.norm(x))
    return np.array([rows, cols], np.int32).reshape(2, -1), np.array(vals, np.float32), N_FORCED


def alternating_medians(a, b, reps):
    """(median of a, median of b) in microseconds over `reps` calls of each, a and b alternating."""
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        a()
        t1 = time.perf_counter()
        b()
        ta.append(t1 - t0)
        tb.append(time.perf_counter() - t1)
    return float(np.median(ta)) * 1e6, float(np.median(tb)) * 1e6


def launch_us(fn, names, reps):
    """Per name in `names` the median microseconds of that launch over `reps` runs of fn under the event brackets."""
    seen = {n: [] for n in names}
    for _ in range(reps):
        with _lib.launch_profile() as prof:
            fn()
        for n, ms in prof.launches:
            if n in seen:
                seen[n].append(ms * 1e3)
    return {n: float(np.median(v)) for n, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    keys = [f"seed/{i}" for i in range(M)]
    models = {k: GCNN(device=dev, seed=i) for i, k in enumerate(keys)}
    mset = ModelSet(models)
    lines = ["all times in microseconds, end to end on the host (perf_counter around the route, every download waited for); "
             f"M = {M}; selection with {N_FORCED} forced rows per state; each figure the median of {args.reps} calls, the two routes "
             f"alternating call by call; {REPEATS} repeats in one process"]
    for problem in ("setcov", "capfac"):
        state = utils.state_to_inputs(synthetic.make_sample(problem, 7)[0])
        forced = forced_rows(np.random.default_rng(7), state)
        lines.append(f"{problem}: sample 7 at full scale, K = {int(state[9])} cuts, {int(state[7])} constraints, {int(state[8])} variables")
        for S in SIZES:
            states, rows = [state] * S, [forced] * S

            def one_call():
                return mset.select_cuts_ensemble_many(keys, states, rows)

            def s_calls():
                return [mset.select_cuts_ensemble(keys, st, f) for st, f in zip(states, rows)]

            for _ in range(10):
                got, want = one_call(), s_calls()
            sess = mset.ensemble_batch_session()
            calls = sess.calls
            one_call()
            assert sess.calls == calls + 1
            for g, w in zip(got, want):       # another union for S > 1: the same selection is expected, the same bits are not
                assert np.allclose(np.asarray(g.scores), np.asarray(w.scores), rtol=2e-4, atol=2e-4) and g.order.shape == w.order.shape
            if S == 1:
                assert np.array_equal(np.asarray(got[0].scores), np.asarray(want[0].scores)) and np.array_equal(got[0].order, want[0].order)
            pairs = [alternating_medians(one_call, s_calls, args.reps) for _ in range(REPEATS)]
            t_a, t_b = [p[0] for p in pairs], [p[1] for p in pairs]
            spread = max(t_b) - min(t_b)
            diff = float(np.median(t_a)) - float(np.median(t_b))
            if S == 1:
                verdict = "no slower" if diff <= spread else "SLOWER by more than the spread"
            else:
                verdict = "faster by more than the spread" if diff < -spread else "NOT faster beyond the spread"
            lines += [
                f"  S = {S:2d}  (a) one call " + " ".join(f"{t:8.1f}" for t in t_a) + f" | median {np.median(t_a):8.1f}",
                f"          (b) S calls  " + " ".join(f"{t:8.1f}" for t in t_b) + f" | median {np.median(t_b):8.1f} | spread {spread:.1f}",
                f"          (a) - (b): {diff:+.1f}; (b) / (a): {np.median(t_b) / np.median(t_a):.2f}x -> (a) is {verdict}",
            ]
        if problem == "setcov":
            S = 16
            states = [state] * S
            mset.score_ensemble_many(keys, states, rank=True)
            with _lib.launch_profile() as prof:
                got = mset.score_ensemble_many(keys, states, rank=True)
            lines.append(f"  rank mode, S = {S}, per launch ({len(prof.launches)} launches): "
                         + " ".join(f"{n} {ms * 1e3:.1f}" for n, ms in prof.launches))
            member_rows = [torch.from_numpy(np.concatenate([np.asarray(q.members[m]) for q in got])).to(dev) for m in range(M)]
            first = models[keys[0]]
            first.score_states(states, rank=True)
            ops.ensemble_mean(member_rows)
            fused, mean, rank = [], [], []
            for _ in range(REPEATS):
                fused.append(launch_us(lambda: mset.score_ensemble_many(keys, states, rank=True), ["k_eb_mean_rank"], args.reps)["k_eb_mean_rank"])
                mean.append(launch_us(lambda: ops.ensemble_mean(member_rows), ["k_ens_mean"], args.reps)["k_ens_mean"])
                rank.append(launch_us(lambda: first.score_states(states, rank=True), ["k_ib_rank"], args.reps)["k_ib_rank"])
            pair = [a + b for a, b in zip(mean, rank)]
            spread = max(pair) - min(pair)
            diff = float(np.median(fused)) - float(np.median(pair))
            verdict = "faster by more than the spread" if diff < -spread else "NOT faster beyond the spread"
            lines += [
                f"  rank-mode tail, S = {S}, K_total = {member_rows[0].numel()}, event brackets, medians of {args.reps} launches, {REPEATS} repeats:",
                "    k_eb_mean_rank          " + " ".join(f"{t:6.2f}" for t in fused) + f" | median {np.median(fused):6.2f}",
                "    k_ens_mean              " + " ".join(f"{t:6.2f}" for t in mean) + f" | median {np.median(mean):6.2f}",
                "    k_ib_rank               " + " ".join(f"{t:6.2f}" for t in rank) + f" | median {np.median(rank):6.2f}",
                "    k_ens_mean + k_ib_rank  " + " ".join(f"{t:6.2f}" for t in pair) + f" | median {np.median(pair):6.2f} | spread {spread:.2f}",
                f"    fused - pair: {diff:+.2f} -> the fused launch is {verdict} (the pair's sum leaves out the gap between its launches)",
            ]
    lines.append("not measured: other M, the LP forms, the server")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
