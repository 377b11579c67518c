"""A worker process of tests/test_gpu_collect_serve.py: NumPy only, opens no GPU, plays a data collector's rounds against the scoring
server -- hybrid rounds (`select_cuts_hybrid`) and one expert round (`collect_lp`) -- and stores what it was answered.  With BAD = 1
it also sends an expert round whose snapshot the device rejects and expects its error.  `round_of(worker, j)` is shared with the
test, which recomputes every answer in process.

usage: serve_worker_collect.py ROOT ADDRESS WORKER_ID OUT.npz BAD"""
import sys

N_HYBRID = 2
STATE_NAMES = ("cons_feats", "cons_edge_inds", "cons_edge_feats", "var_feats", "cut_feats", "cut_edge_inds", "cut_edge_feats")


def round_of(worker, j):
    """-> (snapshot, forced, quality or None).  Rounds 0 .. N_HYBRID-1 are hybrid rounds, round N_HYBRID is the expert's."""
    import numpy as np

    from gcnn_cut_selector_amd import synthetic
    problem = synthetic.PROBLEMS[(worker + j) % len(synthetic.PROBLEMS)]
    snap = synthetic.make_lp_snapshot(problem, 40 * worker + j, scale=0.2, n_cuts=40 + 9 * worker + j)
    forced = None
    if j % 2 == 0:
        forced = (np.array([[0, 0, 1], [0, 2, 1]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    quality = None
    if j == N_HYBRID:
        rng = np.random.default_rng(77 + worker)
        quality = rng.integers(0, 5, snap.cut_lhs.shape[0]) / 64.0          # many ties, as the dives give them
    return snap, forced, quality


def main():
    root, address, wid, out_path, bad = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
    sys.path.insert(0, root)
    import numpy as np

    from gcnn_cut_selector_amd import serve
    client = serve.ScoringClient(address, "no such model", timeout=100)      # the key is ignored: the server holds no model
    out = {}
    for j in range(N_HYBRID):
        snap, forced, _ = round_of(wid, j)
        res = client.select_cuts_hybrid(snap, forced, max_selected=4)
        out[f"o{j}"], out[f"n{j}"], out[f"q{j}"] = res.order, np.int64(res.n_kept), res.scores.numpy()
    if bad:
        snap, forced, quality = round_of(wid, N_HYBRID)
        try:
            client.collect_lp(snap, quality[:-1], forced)                    # refused here, in the worker: nothing is sent
        except ValueError as exc:
            assert "one value per cut" in str(exc), exc
        else:
            raise AssertionError("a short quality was accepted")
        snap.cut_col = snap.cut_col.copy()
        snap.cut_col[0] = 10 ** 6              # passes the worker's cheap check; the device finds the column out of range
        try:
            client.collect_lp(snap, quality, forced)
        except ValueError as exc:
            assert "outside" in str(exc), exc
        else:
            raise AssertionError("the server answered a bad snapshot")
    snap, forced, quality = round_of(wid, N_HYBRID)
    res = client.collect_lp(snap, quality, forced, max_selected=6)
    assert res.n_selected == min(res.n_kept, 6) and len(res.state) == 10
    for name, a in zip(STATE_NAMES, res.state[:7]):
        out[name] = a
    out["sizes"] = np.array(res.state[7:], np.int64)
    out["cut_index"], out["improvements"], out["order"], out["n_kept"] = res.cut_index, res.improvements, res.order, np.int64(res.n_kept)
    out["hybrid_quality"], out["features"] = res.hybrid_quality, res.features
    client.close()
    loaded = [m for m in sys.modules if m == "torch" or m.startswith("torch.") or m.endswith("._lib")]
    assert not loaded, loaded
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
