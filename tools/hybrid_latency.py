"""Latency of the hybrid cut selection from cut rows (HybridSelector, gcnn_hybrid_select) against the model's selection from the
same LP snapshot.  Per BASELINE shape and S = 1, 8, 32, alternating in one process:
  (a) S calls of GCNN.select_cuts_lp (full snapshot up, state built, forward pass, selection on the model's scores);
  (b) S calls of HybridSelector.select_cuts (cuts and three column vectors up, no model);
  (c) one HybridSelector.select_cuts_many over the S snapshots.
Medians over --reps rounds after warm-up, host clock around the calls including their syncs; per path the launches of one round and
the upload bytes from the two layout functions.  Usage: python tools/hybrid_latency.py [--reps N] > profiles/hybrid_select.txt"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.hybrid import HybridSelector  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402

SIZES = (1, 8, 32)
KW = dict(p_max=0.1, p_max_ub=0.5, max_selected=10)


def upload_bytes(snaps):
    """(sum of select_cuts_lp's uploads, sum of the solo hybrid uploads, the batched hybrid upload) from the layout functions."""
    lp = sum(int(lpstate.lp_layout(lpstate.check_snapshot(s, deep=False)[1], 0, 0)[1].in_bytes) for s in snaps)
    dims = [lpstate.check_cut_snapshot(s, deep=False)[1] for s in snaps]

    def hybrid(ds):
        L = _lib.HybridLayout()
        arr = (_lib.HybridDims * len(ds))(*(_lib.HybridDims(**d) for d in ds))
        _lib.check(_lib.lib().gcnn_hybrid_layout_for(len(ds), arr, None, None, _lib.HYBRID_SELECT, C.byref(L)), "gcnn_hybrid_layout_for")
        return int(L.in_bytes)
    return lp, sum(hybrid([d]) for d in dims), hybrid(dims)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    m, h = GCNN(device=dev, seed=0), HybridSelector(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}; microseconds per round of S snapshots; median of {args.reps} rounds, the three "
          "paths alternating; host clock around the calls including their syncs")
    for problem in synthetic.PROBLEMS:
        pool = [synthetic.make_lp_snapshot(problem, i) for i in range(max(SIZES))]
        d = lpstate.check_snapshot(pool[0], deep=False)[1]
        print(f"{problem}: sample 0 has R={d['n_rows']} V={d['n_cols']} K={d['n_cuts']} row entries {d['row_nnz']} cut entries {d['cut_nnz']}")
        for S in SIZES:
            snaps = pool[:S]
            paths = {"a": lambda: [m.select_cuts_lp(s, **KW) for s in snaps],
                     "b": lambda: [h.select_cuts(s, **KW) for s in snaps],
                     "c": lambda: h.select_cuts_many(snaps, **KW)}
            times = {k: [] for k in paths}
            for i in range(args.reps + 5):
                for k, fn in paths.items():
                    t0 = time.perf_counter()
                    fn()
                    if i >= 5:
                        times[k].append(time.perf_counter() - t0)
            launches = {}
            for k, fn in paths.items():
                with _lib.launch_profile() as prof:
                    fn()
                launches[k] = len(prof.launches)
            a, b, c = (float(np.median(times[k])) * 1e6 for k in "abc")
            up = upload_bytes(snaps)
            print(f"  S={S:2d}  (a) {a:9.1f}  (b) {b:9.1f}  (c) {c:9.1f}   (a)/(b) {a / b:5.2f}   (b)/(c) {b / c:5.2f}   per snapshot (c) "
                  f"{c / S:8.1f}   launches (a) {launches['a']} (b) {launches['b']} (c) {launches['c']}   upload bytes (a) {up[0]} (b) {up[1]} (c) {up[2]}")


if __name__ == "__main__":
    main()
