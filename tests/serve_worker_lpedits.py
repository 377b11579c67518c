"""A worker process of tests/test_gpu_lpedits_serve.py: NumPy only, opens no GPU, keeps an LP resident at the scoring server
(`ScoringClient.open_lp`) and runs three separation rounds on it, each of which appends rows and removes rows in the round's own
request.  `play(worker, sess)` is shared with the test, which plays the same rounds on an in-process `LPSession`.

usage: serve_worker_lpedits.py ROOT ADDRESS WORKER_ID OUT.npz"""
import sys

N_ROUNDS = 3
EARLY = 3          # this worker leaves behind its last round without a close request: the server closes its session on the drop


def script(worker):
    """(the worker's `LPRows`, its solve generator, the base snapshot, the candidate pools of its rounds)."""
    import lpappendcases as A
    from gcnn_cut_selector_amd import lpstate
    rng, base, pools = A.loop_script(N_ROUNDS, seed=400 + 10 * worker)
    return lpstate.LPRows.from_snapshot(base), rng, base, pools


def play(worker, sess, rows, rng, base, pools):
    """Three rounds through `sess` (an `LPSession` or a `RemoteLPSession`), each with an append and a removal: two selections and
    a scoring.  The first appends four cuts of its pool as rows and removes two resident rows; the others append what the last
    selection kept and remove a resident row and the row just appended last.  Then, for every worker but EARLY, a removal on its
    own.  -> {name: array} of everything that was answered."""
    import numpy as np

    import lpappendcases as A
    from gcnn_cut_selector_amd import lpstate
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    forced = (np.array([[0, 0, 1], [worker, 20 + worker, 40]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    out = {}
    block = A.cuts_as_rows(pools[0], np.arange(4))
    for r, pool in enumerate(pools):
        rows = lpstate.rows_with(rows, block)
        n = np.asarray(rows.row_lhs).shape[0]
        remove = [1 + worker, 5] if r == 0 else [n - 1, 2 + r]          # (any order; n - 1 points into the request's own block)
        rows = lpstate.rows_without(rows, remove)
        rnd = lpstate.LPRound(**A.S._solve(rng, rows, 64, col_lp=base.col_lp), **A.S._cuts_of(pool), **(full if r == 0 else {}),
                              has_incumbent=True)
        if r < 2:
            res = sess.select_cuts(rnd, forced, p_max=0.9, p_max_ub=0.95, max_selected=6, append=block, remove=remove)
            assert res.n_selected == min(res.n_kept, 6) > 0
            out[f"s{r}"], out[f"o{r}"], out[f"n{r}"], out[f"i{r}"] = np.asarray(res.scores), res.order, np.int64(res.n_kept), res.cut_index
            block = A.cuts_as_rows(pool, res.cut_index[res.order[:res.n_selected]])
        else:
            q = sess.score(rnd, append=block, remove=remove)
            out[f"s{r}"], out[f"i{r}"] = np.asarray(q), q.cut_index
        assert sess.n_rows == np.asarray(rows.row_lhs).shape[0]
    if worker != EARLY:
        sess.remove_rows([0, 3])
        assert sess.n_rows == np.asarray(rows.row_lhs).shape[0] - 2
    out["rows"] = np.int64(sess.n_rows)
    return out


def main():
    root, address, wid, out_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    sys.path.insert(0, root)
    import numpy as np

    from gcnn_cut_selector_amd import serve
    rows, rng, base, pools = script(wid)
    client = serve.ScoringClient(address, f"m{wid % 2}", timeout=100)
    sess = client.open_lp(rows)
    out = play(wid, sess, rows, rng, base, pools)
    if wid != EARLY:
        sess.close()
    client.close()
    loaded = [m for m in sys.modules if m == "torch" or m.startswith("torch.") or m.endswith("._lib")]
    assert not loaded, loaded
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
