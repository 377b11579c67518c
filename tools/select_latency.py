"""Cut selection latency: GCNN.select_cuts (score + parallelism filter of cutselselect, model_evaluator.py:109-154) against
GCNN.score_state(rank=True) -- what the plugin pays today before its own Python filter -- on one state per problem, then on states
with 1,000 and 4,096 cuts with sparse and dense conflict patterns.  End to end = host clock around call + sync; device = HIP events
around the call on the current stream; launches and their event-bracketed times from _lib.launch_profile.  For contrast the host
restatement's filter (tests/cutsel_restate.py) with P precomputed -- NOT the reference's cost, which also pays K^2/2 PySCIPOpt
getRowParallelism calls that cannot be measured here.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python ...`.
Usage: python tools/select_latency.py [--reps N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cutsel_restate as R  # noqa: E402
from gcnn_cut_selector_amd import _lib, synthetic, utils  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402


def big_state(K, dense, seed=0):
    """A setcov state with K cut rows: 'sparse' = independent random rows (few conflicts), 'dense' = rows drawn from a bank of 32
    base rows, scaled or partially overlapping (most pairs conflict)."""
    state, _ = synthetic.make_sample("setcov", 0)
    inp = list(utils.state_to_inputs(state))
    V = inp[8]
    rng = np.random.default_rng(seed)
    bank = []
    for _ in range(32):
        c = np.sort(rng.choice(V, size=int(rng.integers(5, 30)), replace=False))
        v = rng.standard_normal(c.size)
        bank.append((c, (v / np.linalg.norm(v)).astype(np.float32)))
    rows, cols, vals = [], [], []
    for k in range(K):
        if dense:
            c, v = bank[rng.integers(0, 32)]
            v = v * np.float32(rng.choice([1.0, -1.0, 0.7]))
        else:
            c = np.sort(rng.choice(V, size=int(rng.integers(5, 30)), replace=False))
            v = rng.standard_normal(c.size)
            v = (v / np.linalg.norm(v)).astype(np.float32)
        rows.append(np.full(c.size, k)); cols.append(c); vals.append(v)
    inp[4] = rng.standard_normal((K, 6)).astype(np.float32)
    inp[5] = np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int32)
    inp[6] = np.concatenate(vals).astype(np.float32).reshape(-1, 1)
    inp[9] = K
    return tuple(inp)


def timed(fn, reps):
    host, devt = [], []
    stream = torch.cuda.current_stream()
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
        devt.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(host)) * 1e6, float(np.median(devt)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    m = GCNN(device=dev, seed=0)
    cases = [(p, utils.state_to_inputs(synthetic.make_sample(p, 7)[0])) for p in synthetic.PROBLEMS]
    cases += [(f"setcov K={K} {kind}", big_state(K, kind == "dense")) for K in (1000, 4096) for kind in ("sparse", "dense")]
    print("all times in microseconds, medians; host = perf_counter around call + sync, device = HIP events around the call")
    for name, inp in cases:
        K = int(inp[9])
        reps = args.reps if K <= 1000 else max(20, args.reps // 4)
        for _ in range(5):
            m.score_state(inp, rank=True)
            res = m.select_cuts(inp)
        h_rank, d_rank = timed(lambda: m.score_state(inp, rank=True), reps)
        h_sel, d_sel = timed(lambda: m.select_cuts(inp), reps)
        with _lib.launch_profile() as p_rank:
            m.score_state(inp, rank=True)
        with _lib.launch_profile() as p_sel:
            m.select_cuts(inp)
        sel_k = [(n, ms * 1e3) for n, ms in p_sel.launches if n.startswith("k_sel_")]
        # host restatement of the filter with P precomputed (not the reference's cost: no getRowParallelism calls in it)
        rows, cols = inp[5]
        A = R.dense_rows(rows, cols, np.asarray(inp[6]).reshape(-1), K, int(inp[8]))
        P = (np.abs(A @ A.T), np.zeros((0, K)))
        q = np.asarray(res.scores)
        t_host = []
        for _ in range(3 if K > 1000 else 10):
            t0 = time.perf_counter()
            order, n = R.select(q, None, None, P=P)
            t_host.append(time.perf_counter() - t0)
        assert np.array_equal(order, res.order) and n == res.n_kept
        print(f"{name:22s} K={K:5d} kept={res.n_kept:5d} | score_state(rank=True): host {h_rank:8.1f} device {d_rank:8.1f}, "
              f"{len(p_rank.launches)} launches | select_cuts: host {h_sel:8.1f} device {d_sel:8.1f}, {len(p_sel.launches)} launches "
              f"| added: host {h_sel - h_rank:+8.1f} device {d_sel - d_rank:+8.1f}, {len(p_sel.launches) - len(p_rank.launches)} launches "
              f"| event brackets " + " ".join(f"{n} {us:.1f}" for n, us in sel_k)
              + f" | host restatement, P precomputed (not the reference's cost): {np.median(t_host) * 1e6:.0f}")


if __name__ == "__main__":
    main()
