"""A worker process of tests/test_gpu_lpens_serve.py: NumPy only, opens no GPU, keeps an LP resident at the scoring server under
the name it is given -- an ensemble's or a model's, the worker cannot tell -- and runs eight rounds of the separation loop on it:
every round after the first appends the cuts the last selection kept, and once enough cut rows are resident two earlier ones
leave in the same request.  `play(worker, sess, ...)` is shared with the test, which plays the same rounds on the in-process
one-shot calls over the assembled snapshots.

usage: serve_worker_lpens.py ROOT ADDRESS WORKER_ID MODEL_KEY OUT.npz"""
import sys

N_ROUNDS = 8


def script(worker):
    """(the worker's `LPRows`, its solve generator, the base snapshot, the candidate pools of its rounds)."""
    import lpappendcases as A
    from gcnn_cut_selector_amd import lpstate
    rng, base, pools = A.loop_script(N_ROUNDS, seed=500 + 10 * worker)
    return lpstate.LPRows.from_snapshot(base), rng, base, pools


def play(worker, sess, rows, rng, base, pools):
    """Eight selections through `sess` (anything with `LPSession.select_cuts`'s signature and `n_rows`).  -> {name: array} of
    everything that was answered."""
    import numpy as np

    import lpappendcases as A
    from gcnn_cut_selector_amd import lpstate
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    forced = (np.array([[0, 0, 1], [worker, 20 + worker, 40]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    n_base = np.asarray(rows.row_lhs).shape[0]
    out, block, removals = {}, None, 0
    for r, pool in enumerate(pools):
        remove = None
        if block is not None:
            rows = lpstate.rows_with(rows, block)
            n = np.asarray(rows.row_lhs).shape[0]
            if n - n_base >= 6:
                remove = [n - 1, n_base + r % 3]                    # (any order; n - 1 points into the request's own block)
                rows = lpstate.rows_without(rows, remove)
                removals += 1
        rnd = lpstate.LPRound(**A.S._solve(rng, rows, 64, col_lp=base.col_lp), **A.S._cuts_of(pool), **(full if r == 0 else {}),
                              has_incumbent=True)
        res = sess.select_cuts(rnd, forced, p_max=0.9, p_max_ub=0.95, max_selected=6, append=block, remove=remove)
        assert res.n_selected == min(res.n_kept, 6) > 0
        out[f"s{r}"], out[f"o{r}"], out[f"n{r}"], out[f"i{r}"] = np.asarray(res.scores), res.order, np.int64(res.n_kept), res.cut_index
        block = A.cuts_as_rows(pool, res.cut_index[res.order[:res.n_selected]])
        assert sess.n_rows == np.asarray(rows.row_lhs).shape[0]
    assert removals >= 3
    out["rows"] = np.int64(sess.n_rows)
    return out


def main():
    root, address, wid, key, out_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
    sys.path.insert(0, root)
    import numpy as np

    from gcnn_cut_selector_amd import serve
    rows, rng, base, pools = script(wid)
    client = serve.ScoringClient(address, key, timeout=100)
    sess = client.open_lp(rows)
    out = play(wid, sess, rows, rng, base, pools)
    sess.close()
    client.close()
    loaded = [m for m in sys.modules if m == "torch" or m.startswith("torch.") or m.endswith("._lib")]
    assert not loaded, loaded
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
