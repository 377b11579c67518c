"""A worker process of tests/test_gpu_lpbatch.py: NumPy only, opens no GPU, sends raw LP snapshots to the scoring server and stores
what it was answered.  `lp_request(worker, j)` is shared with the test, which recomputes every answer in process.

usage: serve_worker_lp.py ROOT ADDRESS WORKER_ID OUT.npz READY_FILE"""
import sys

N_REQUESTS = 6
KINDS = ("score", "rank", "select")


def lp_request(worker, j):
    """-> (kind, snapshot, forced).  Small snapshots of all four problems, with and without an incumbent."""
    import numpy as np

    from gcnn_cut_selector_amd import synthetic
    problem = synthetic.PROBLEMS[(worker + j) % len(synthetic.PROBLEMS)]
    snap = synthetic.make_lp_snapshot(problem, 10 * worker + j, scale=0.3, incumbent=(worker + j) % 3 != 0)
    kind = KINDS[(worker + 2 * j) % 3]
    forced = None
    if kind == "select" and j % 2:
        forced = (np.array([[0, 0, 1], [0, 2, 1]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    return kind, snap, forced


def bad_snapshot(worker):
    """Passes the worker's cheap check; the device finds the column out of range."""
    _, snap, _ = lp_request(worker, 0)
    snap.cut_col = snap.cut_col.copy()
    snap.cut_col[0] = 10 ** 6
    return snap


def main():
    root, address, wid, out_path, ready = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
    sys.path.insert(0, root)
    import numpy as np

    from gcnn_cut_selector_amd import serve
    client = serve.ScoringClient(address, "m", timeout=200)
    out = {}
    open(ready, "w").close()
    for j in range(N_REQUESTS):
        kind, snap, forced = lp_request(wid, j)
        if kind == "select":
            res = client.select_cuts_lp(snap, forced, p_max=0.1, p_max_ub=0.5, max_selected=4)
            assert res.n_selected == min(res.n_kept, 4)
            out[f"s{j}"], out[f"o{j}"], out[f"n{j}"], out[f"i{j}"] = res.scores.numpy(), res.order, np.int64(res.n_kept), res.cut_index
        else:
            q = client.score_lp(snap, rank=kind == "rank")
            out[f"s{j}"], out[f"i{j}"] = q.numpy(), q.cut_index
            if kind == "rank":
                out[f"o{j}"] = q.rankings
        if j == 2:
            try:
                client.score_lp(bad_snapshot(wid))
            except ValueError as exc:
                assert "outside" in str(exc), exc
            else:
                raise AssertionError("the server answered a bad snapshot")
    client.close()
    loaded = [m for m in sys.modules if m == "torch" or m.startswith("torch.") or m.endswith("._lib")]
    assert not loaded, loaded
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
