"""A worker process of tests/test_gpu_hybrid.py: NumPy only, opens no GPU, sends hybrid selection requests (cut rows, no LP rows, no
model) to the scoring server and stores what it was answered.  `hybrid_request(worker, j)` is shared with the test, which
recomputes every answer in process.

usage: serve_worker_hybrid.py ROOT ADDRESS WORKER_ID OUT.npz"""
import sys

N_REQUESTS = 4


def hybrid_request(worker, j):
    """-> (snapshot, forced, thresholds).  An `LPSnapshot` or the `CutSnapshot` of its fields, with and without forced rows."""
    import numpy as np

    from gcnn_cut_selector_amd import lpstate, synthetic
    problem = synthetic.PROBLEMS[(worker + j) % len(synthetic.PROBLEMS)]
    snap = synthetic.make_lp_snapshot(problem, 20 * worker + j, scale=0.3, incumbent=False)
    if j % 2:
        snap = lpstate.CutSnapshot(**{name: getattr(snap, name) for name, _ in lpstate.CUT_FIELDS}, infinity=snap.infinity)
    forced = None
    if j >= 2:
        forced = (np.array([[0, 0, 1], [0, 2, 1]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    return snap, forced, ((0.1, 0.5) if j != 3 else (0.2, 0.6))


def main():
    root, address, wid, out_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    sys.path.insert(0, root)
    import numpy as np

    from gcnn_cut_selector_amd import serve
    client = serve.ScoringClient(address, "no such model", timeout=100)      # the key is ignored: there is no model
    out = {}
    for j in range(N_REQUESTS):
        snap, forced, (p_max, p_max_ub) = hybrid_request(wid, j)
        res = client.select_cuts_hybrid(snap, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=4)
        assert res.n_selected == min(res.n_kept, 4)
        out[f"q{j}"], out[f"o{j}"], out[f"n{j}"], out[f"i{j}"], out[f"f{j}"] = (res.scores.numpy(), res.order, np.int64(res.n_kept),
                                                                                  res.cut_index, res.features)
    bad, _, _ = hybrid_request(wid, 0)
    bad.cut_col = bad.cut_col.copy()
    bad.cut_col[0] = 10 ** 6               # passes the worker's cheap check; the device finds the column out of range
    try:
        client.select_cuts_hybrid(bad)
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
