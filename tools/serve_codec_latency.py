"""Host cost of the scoring server's codec (gcnn_cut_selector_amd/serve.py), without a GPU and without a socket: one request of
every kind through `decode_request(encode_*_request(...))`, and both reply shapes (scores with rankings and cut_index; a selection
with order, cut_index and features) through `decode_reply(encode_reply(...))`.  The instances are those the served runs of
tools/infer_batch_latency.py (setcov host states, sample 100) and tools/lp_edits_latency.py (`synthetic.make_lp_snapshot(problem, 0)`,
ten rows appended and removed, three forced rows) send.  Prints microseconds: the median (interquartile range) of `--reps` round
trips per line, the lines' repetitions interleaved so that a drift of the machine spreads over all of them.
Usage: python tools/serve_codec_latency.py [--reps N] [--problem setcov] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

from gcnn_cut_selector_amd import lpstate, serve, synthetic, utils  # noqa: E402


def cases(problem):
    """[(name, a callable that makes one round trip)]."""
    state = utils.state_to_inputs(synthetic.make_sample(problem, 100)[0])
    snap = synthetic.make_lp_snapshot(problem, 0)
    rows, base = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
    ptr = np.asarray(snap.cut_ptr)
    n = min(10, ptr.shape[0] - 1)
    block = lpstate.LPRowBlock(ptr[:n + 1].astype(np.int32), np.asarray(snap.cut_col)[:ptr[n]].astype(np.int32),
                               np.asarray(snap.cut_val)[:ptr[n]].astype(np.float64), np.asarray(snap.cut_lhs)[:n].astype(np.float64),
                               np.asarray(snap.cut_rhs)[:n].astype(np.float64))
    R0, V, K = np.asarray(rows.row_lhs).shape[0], np.asarray(snap.col_type).shape[0], np.asarray(snap.cut_lhs).shape[0]
    rnd = lpstate.LPRound(**{**base.__dict__, "row_dual": np.concatenate([base.row_dual, np.zeros(n)]),
                             "row_basis": np.concatenate([base.row_basis, np.ones(n, np.int8)])})
    remove = R0 + np.arange(n)
    forced = (np.array([[0, 0, 1], [0, min(2, V - 1), min(1, V - 1)]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    quality = np.linspace(0.0, 1.0, K)
    dec, key = serve.decode_request, "m"
    out = [(f"request kind {k} ({name})", (lambda k=k, f=f: dec(serve.encode_request(key, k, state, f))))
           for k, name, f in ((0, "score_state", None), (1, "score_state, rank", None), (2, "select_cuts, forced", forced))]
    out += [(f"request kind {k} ({name})", (lambda k=k, f=f: dec(serve.encode_lp_request(key, k, snap, f))))
            for k, name, f in ((3, "score_lp", None), (4, "score_lp, rank", None), (5, "select_cuts_lp, forced", forced))]
    out += [("request kind 6 (select_cuts_hybrid, forced)", lambda: dec(serve.encode_hybrid_request(key, snap, forced))),
            ("request kind 7 (open_lp)", lambda: dec(serve.encode_open_request(key, rows, False))),
            ("request kind 8 (round: select, forced)", lambda: dec(serve.encode_round_request(key, 7, serve.SESSION_SELECT, base, forced))),
            ("request kind 8 (round: select, forced, append, remove)",
             lambda: dec(serve.encode_round_request(key, 7, serve.SESSION_SELECT, rnd, forced, append=block, remove=remove))),
            ("request kind 8 (edit alone: append, remove)",
             lambda: dec(serve.encode_round_request(key, 7, serve.SESSION_APPEND, append=block, remove=remove))),
            ("request kind 9 (close)", lambda: dec(serve.encode_close_request(key, 7))),
            ("request kind 11 (collect_lp, forced)", lambda: dec(serve.encode_collect_request(key, snap, quality, forced)))]
    scores, order = np.linspace(0, 1, K, dtype=np.float32), np.arange(K, dtype=np.int32)
    features = np.zeros((K, 3))
    out += [("reply: scores, rankings, cut_index", lambda: serve.decode_reply(serve.encode_reply([scores, order, order]))),
            ("reply: selection with cut_index and features",
             lambda: serve.decode_reply(serve.encode_reply([scores, order, order, features], K, min(K, 10))))]
    return out, f"{problem}: state of sample 100; LP snapshot 0 with rows {R0}, columns {V}, cuts {K}; block of {n} rows"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3000)
    ap.add_argument("--problem", default="setcov", choices=synthetic.PROBLEMS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    todo, what = cases(args.problem)
    for _, call in todo:            # warm up: imports inside NumPy, the allocator
        for _ in range(20):
            call()
    times = [[] for _ in todo]
    for _ in range(args.reps):
        for t, (_, call) in zip(times, todo):
            t0 = time.perf_counter()
            call()
            t.append(time.perf_counter() - t0)
    lines = [f"microseconds; median (interquartile range) of {args.reps} round trips, the lines interleaved; {what}"]
    for (name, _), t in zip(todo, times):
        q1, q2, q3 = np.percentile(np.asarray(t) * 1e6, [25, 50, 75])
        lines.append(f"{name:58s} {q2:9.1f} ({q3 - q1:.1f})")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
