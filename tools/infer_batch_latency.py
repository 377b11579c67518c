"""Latency of the batched single-call path: for S in {1, 2, 4, 8, 16, 32} states of each BASELINE shape, GCNN.select_cuts_many
(one gcnn_infer_batch call) against S calls of the unchanged GCNN.select_cuts, and GCNN.score_states against S calls of
GCNN.score_state, in the same process; then the scoring server (gcnn_cut_selector_amd/serve.py) with 1-16 torch-free client
processes.  Host clock around call(s) + sync; medians over --reps runs after warm-up, with the 10th / 90th percentile as spread.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/infer_batch_latency.py --no-server --reps 20`.
Usage: python tools/infer_batch_latency.py [--reps N] [--no-server] [--sizes 1,2,4,...]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

CLIENT = """
import os, sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np
from gcnn_cut_selector_amd import serve, synthetic, utils
address, problem, wid, n = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
states = [utils.state_to_inputs(synthetic.make_sample(problem, 100 + 8 * wid + i)[0]) for i in range(8)]
c = serve.ScoringClient(address, "m", timeout=300)
for i in range(5):
    c.select_cuts(states[i % 8])
open(sys.argv[6], "w").close()
while not os.path.exists(sys.argv[7]):
    time.sleep(0.001)
t = []
for i in range(n):
    t0 = time.perf_counter(); c.select_cuts(states[i % 8]); t.append(time.perf_counter() - t0)
assert "torch" not in sys.modules
print(" ".join(f"{x:.7f}" for x in t))
"""


def timed(fn, reps, warm=5):
    import torch
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t = np.asarray(t) * 1e6
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--no-server", action="store_true")
    args = ap.parse_args()
    import torch
    from gcnn_cut_selector_amd import serve, synthetic, utils
    from gcnn_cut_selector_amd.model import GCNN
    dev = torch.device("cuda", 0)
    m = GCNN(device=dev, seed=0)
    sizes = [int(x) for x in args.sizes.split(",")]
    print("all times in microseconds: median [p10 .. p90] of the whole call(s), host clock incl. sync; per state = median / S")
    for problem in synthetic.PROBLEMS:
        pool = [utils.state_to_inputs(synthetic.make_sample(problem, 100 + i)[0]) for i in range(max(sizes))]
        for S in sizes:
            states = pool[:S]
            many = timed(lambda: m.select_cuts_many(states), args.reps)
            solo = timed(lambda: [m.select_cuts(s) for s in states], args.reps)
            smany = timed(lambda: m.score_states(states, rank=True), args.reps)
            ssolo = timed(lambda: [m.score_state(s, rank=True) for s in states], args.reps)
            print(f"{problem:8s} S={S:2d} | select_cuts_many {many[0]:9.1f} [{many[1]:9.1f} .. {many[2]:9.1f}] per state {many[0] / S:8.1f} | "
                  f"S x select_cuts {solo[0]:9.1f} [{solo[1]:9.1f} .. {solo[2]:9.1f}] per state {solo[0] / S:8.1f} | ratio {solo[0] / many[0]:5.2f} || "
                  f"score_states(rank) {smany[0]:9.1f} per state {smany[0] / S:8.1f} | S x score_state(rank) {ssolo[0]:9.1f} per state "
                  f"{ssolo[0] / S:8.1f} | ratio {ssolo[0] / smany[0]:5.2f}", flush=True)
    if args.no_server:
        return
    print("server: N torch-free client processes, each sending select_cuts requests back to back (setcov states, BASELINE shape); "
          "per-request round trip seen by the clients, and requests served per second")
    for n_clients in (1, 2, 4, 8, 16):
        with tempfile.TemporaryDirectory() as d:
            address = os.path.join(d, "s.sock")
            server = serve.ScoringServer({"m": m}, address).start()
            n = max(20, args.reps)
            procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, "-c", CLIENT, ROOT, address, "setcov", str(w), str(n),
                                       os.path.join(d, f"ready{w}"), os.path.join(d, "go")], stdout=subprocess.PIPE, text=True)
                     for w in range(n_clients)]
            try:
                while not all(os.path.exists(os.path.join(d, f"ready{w}")) for w in range(n_clients)):
                    if any(p.poll() is not None for p in procs):
                        raise RuntimeError("a client ended early")
                    time.sleep(0.01)
                before = dict(server.stats)
                t0 = time.perf_counter()
                open(os.path.join(d, "go"), "w").close()
                outs = [p.communicate(timeout=300)[0] for p in procs]
                wall = time.perf_counter() - t0
            finally:
                for p in procs:
                    if p.poll() is None:
                        p.kill()
                server.close()
            if any(p.returncode for p in procs):
                raise RuntimeError("a client failed")
            t = np.asarray([float(x) for o in outs for x in o.split()]) * 1e6
            calls = server.stats["calls"] - before["calls"]
            print(f"clients={n_clients:2d} | round trip {np.median(t):9.1f} [{np.percentile(t, 10):9.1f} .. {np.percentile(t, 90):9.1f}] | "
                  f"{n_clients * n / wall:8.0f} requests/s | {n_clients * n / max(calls, 1):5.2f} requests per call, largest group "
                  f"{server.stats['max_batch']}", flush=True)


if __name__ == "__main__":
    main()
