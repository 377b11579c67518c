"""Latency of the data collector's expert round (collect.Collector.collect_lp, gcnn_lp_collect) on sample 0 of the four problem shapes
(`synthetic.make_lp_snapshot(problem, 0)`), three arms that alternate in one process:

  (a)  GCNN.state_from_lp(snap) followed by HybridSelector.select_cuts(snap, forced): the closest the library offered in process
       before collect_lp -- two uploads, two downloads, the same six launches.  It ranks by the WRONG quality (the hybrid one, not
       the expert's), so it is a yardstick of cost only.
  (b)  Collector.collect_lp(snap, quality, forced): one upload, one download.
  (c)  the same through a ScoringServer (a thread of this process, holding no model) from one ScoringClient over an AF_UNIX socket.

Medians of --reps rounds (default 50) after 5 warm-up rounds; host clock (perf_counter) around the call, the wait for the download
included; the launch profiler is off while timing (it runs once afterwards, for the launch list).  Also reported: launches, upload
and download bytes of (a) and (b), and the pack / enqueue / wait split of (b).  The expert's quality is drawn with many ties, as
SCIP's dives give it.
Usage: python tools/collect_latency.py [--reps N]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, serve, synthetic  # noqa: E402
from gcnn_cut_selector_amd.collect import Collector  # noqa: E402
from gcnn_cut_selector_amd.hybrid import HybridSelector  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402


def median_us(samples):
    return float(np.median(samples)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    model, hyb, col = GCNN(device=dev, seed=0), HybridSelector(dev), Collector(dev)
    address = os.path.join(tempfile.mkdtemp(prefix="gcnn_collect_"), "sock")
    server = serve.ScoringServer({}, address).start()
    client = serve.ScoringClient(address, "none", timeout=120)
    forced = (np.array([[0, 0, 1], [0, 2, 1]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    print(f"times in microseconds, medians of {args.reps}; host clock around the call, the wait for the download included; one run on one box")
    try:
        for problem in synthetic.PROBLEMS:
            snap = synthetic.make_lp_snapshot(problem, 0)
            arrays, dims = lpstate.check_snapshot(snap, deep=False)
            K = dims["n_cuts"]
            quality = np.random.default_rng(1).integers(0, 6, K) / 64.0

            def arm_a():
                model.state_from_lp(snap)
                return hyb.select_cuts(snap, forced)

            def arm_b(timings=None):
                return col.collect_lp(snap, quality, forced, timings=timings)

            def arm_c():
                return client.collect_lp(snap, quality, forced)

            for _ in range(5):
                arm_a(), arm_b(), arm_c()
            t = {"a": [], "b": [], "c": []}
            split = {"pack": [], "enqueue": [], "wait": []}
            for _ in range(args.reps):
                for name, fn in (("a", arm_a), ("b", arm_b), ("c", arm_c)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    t[name].append(time.perf_counter() - t0)
                tm = {}
                arm_b(tm)                                      # (a round of its own: the timed ones carry no dict)
                for k in split:
                    split[k].append(tm[k])
            with _lib.launch_profile() as pa:
                arm_a()
            with _lib.launch_profile() as pb:
                res = arm_b()
            got = arm_c()
            assert np.array_equal(got.order, res.order) and got.n_kept == res.n_kept and np.array_equal(got.state[4], res.state[4])
            _, lp = lpstate.lp_layout(dims)
            up_a = int(lp.snap_bytes) + hyb._sess().upload_bytes
            down_a = sum(int(np.asarray(x).nbytes) for x in res.state[:7]) + 4 * K + 16 + int(hyb._sess().last.out_bytes)
            a, b, c = median_us(t["a"]), median_us(t["b"]), median_us(t["c"])
            print(f"{problem:8s} R={dims['n_rows']:5d} V={dims['n_cols']:5d} K={K:3d} kept={res.n_kept:3d} | (a) state_from_lp + hybrid select "
                  f"{a:7.1f}, {len(pa.launches)} launches, up {up_a} B in 2 copies, down {down_a} B in 9 + 1 copies | (b) collect_lp {b:7.1f} "
                  f"({b - a:+.1f}, {100 * (b - a) / a:+.1f} %), {len(pb.launches)} launches, up {col._sess().upload_bytes} B, down "
                  f"{col._sess().download_bytes} B, one copy each; pack {median_us(split['pack']):.1f} enqueue "
                  f"{median_us(split['enqueue']):.1f} wait {median_us(split['wait']):.1f} | (c) through the server {c:7.1f} ({c - b:+.1f} over (b))")
            print("         launches of (b): " + " ".join(f"{n} {ms * 1e3:.1f}" for n, ms in pb.launches) + "  (event brackets, profiler on)")
    finally:
        client.close()
        server.close()


if __name__ == "__main__":
    main()
