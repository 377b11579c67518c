"""A worker process of tests/test_gpu_lprounds_serve.py: NumPy only, opens no GPU, keeps an LP resident at the scoring server
(`ScoringClient.open_lp`) and runs three separation rounds on it, appending the cuts its last selection kept.  `play(worker, sess)`
is shared with the test, which plays the same rounds on an in-process `LPSession`.

usage: serve_worker_lpsession.py ROOT ADDRESS WORKER_ID OUT.npz"""
import sys

N_ROUNDS = 3


def script(worker):
    """(the worker's `LPRows`, its solve generator, the base snapshot, the candidate pools of its rounds)."""
    import lpappendcases as A
    from gcnn_cut_selector_amd import lpstate
    rng, base, pools = A.loop_script(N_ROUNDS, seed=300 + 10 * worker)
    return lpstate.LPRows.from_snapshot(base), rng, base, pools


def play(worker, sess, rows, rng, base, pools):
    """Three rounds through `sess` (an `LPSession` or a `RemoteLPSession`): a selection, a selection that appends what the first
    kept, a scoring that appends what the second kept.  -> {name: array} of everything that was answered."""
    import numpy as np

    import lpappendcases as A
    from gcnn_cut_selector_amd import lpstate
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    forced = (np.array([[0, 0, 1], [worker, 20 + worker, 40]], np.int32), np.array([0.6, -0.8, 1.0], np.float32), 2)
    out, block = {}, None
    for r, pool in enumerate(pools):
        if block is not None:
            rows = lpstate.rows_with(rows, block)
        rnd = lpstate.LPRound(**A.S._solve(rng, rows, 64, col_lp=base.col_lp), **A.S._cuts_of(pool), **(full if r == 0 else {}),
                              has_incumbent=True)
        if r < 2:
            res = sess.select_cuts(rnd, forced, p_max=0.9, p_max_ub=0.95, max_selected=6, append=block)
            assert res.n_selected == min(res.n_kept, 6) > 0
            out[f"s{r}"], out[f"o{r}"], out[f"n{r}"], out[f"i{r}"] = np.asarray(res.scores), res.order, np.int64(res.n_kept), res.cut_index
            block = A.cuts_as_rows(pool, res.cut_index[res.order[:res.n_selected]])
        else:
            q = sess.score(rnd, append=block)
            out[f"s{r}"], out[f"i{r}"] = np.asarray(q), q.cut_index
        assert sess.n_rows == np.asarray(rows.row_lhs).shape[0]
    return out


def main():
    root, address, wid, out_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    sys.path.insert(0, root)
    import numpy as np

    from gcnn_cut_selector_amd import serve
    rows, rng, base, pools = script(wid)
    with serve.ScoringClient(address, f"m{wid % 2}", timeout=100) as client:
        with client.open_lp(rows) as sess:
            out = play(wid, sess, rows, rng, base, pools)
            try:
                client._call(serve.encode_close_request("m0", sess.session + 1000))      # not this connection's: an error reply
            except serve.ServerError as exc:
                assert "no LP session" in str(exc), exc
            else:
                raise AssertionError("the server closed a session that does not exist")
    loaded = [m for m in sys.modules if m == "torch" or m.startswith("torch.") or m.endswith("._lib")]
    assert not loaded, loaded
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
