"""Latency of cut selection from S raw LP snapshots at once.  Per BASELINE shape and S = 1, 2, 8, 32, alternating in one process:
  (a) S calls of GCNN.select_cuts_lp (the single call, one snapshot each): the baseline;
  (b) one GCNN.select_cuts_lp_many (gcnn_lp_batch: one upload, two state-building launches, one forward pass over the union);
  (c) S x GCNN.state_from_lp followed by one GCNN.select_cuts_many on the built host states.
Medians over --reps rounds after warm-up, host clock around the calls including their syncs; per call the upload bytes and the
launches.  Usage: python tools/lp_batch_latency.py [--reps N] > profiles/lp_batch.txt"""
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
from gcnn_cut_selector_amd.model import GCNN  # noqa: E402

SIZES = (1, 2, 8, 32)
KW = dict(p_max=0.1, p_max_ub=0.5, max_selected=10)


def upload_bytes(snaps):
    """(sum of the single calls' uploads, the batched call's upload) from the two layout functions."""
    dims = [lpstate.check_snapshot(s, deep=False)[1] for s in snaps]
    single = sum(int(lpstate.lp_layout(d, 0, 0)[1].in_bytes) for d in dims)
    L = _lib.LpBatchLayout()
    arr = (_lib.LpDims * len(dims))(*(_lib.LpDims(**d) for d in dims))
    _lib.check(_lib.lib().gcnn_lp_batch_layout_for(len(dims), arr, None, None, _lib.IBATCH_SELECT, C.byref(L)), "gcnn_lp_batch_layout_for")
    return single, int(L.in_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    m = GCNN(device=torch.device("cuda", 0), seed=0)
    print(f"microseconds per round of S snapshots; median of {args.reps} rounds, the three paths alternating; host clock around the "
          "calls including their syncs")
    for problem in synthetic.PROBLEMS:
        pool = [synthetic.make_lp_snapshot(problem, i) for i in range(max(SIZES))]
        d = lpstate.check_snapshot(pool[0], deep=False)[1]
        print(f"{problem}: sample 0 has R={d['n_rows']} V={d['n_cols']} K={d['n_cuts']} row entries {d['row_nnz']} cut entries {d['cut_nnz']}")
        for S in SIZES:
            snaps = pool[:S]
            paths = {"a": lambda: [m.select_cuts_lp(s, **KW) for s in snaps],
                     "b": lambda: m.select_cuts_lp_many(snaps, **KW),
                     "c": lambda: m.select_cuts_many([m.state_from_lp(s)[0] for s in snaps], **KW)}
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
            single, batched = upload_bytes(snaps)
            print(f"  S={S:2d}  (a) {a:9.1f}  (b) {b:9.1f}  (c) {c:9.1f}   (a)/(b) {a / b:5.2f}   per snapshot (b) {b / S:8.1f}   "
                  f"launches (a) {launches['a']} (b) {launches['b']} (c) {launches['c']}   upload bytes (a) {single} (b) {batched}")


if __name__ == "__main__":
    main()
