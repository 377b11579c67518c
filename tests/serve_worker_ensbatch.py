"""A worker process of tests/test_gpu_ensbatch_serve.py: NumPy only.  It sends host states and LP snapshots under an ensemble's name
through the kinds 1, 2, 4 and 5 as they are -- rank, select, LP rank, LP select -- a few rounds of each, and stores what it was
answered.  The server it talks to groups the ensemble requests that wait together; the worker cannot tell.

usage: serve_worker_ensbatch.py ROOT ADDRESS WORKER_ID ENSEMBLE_NAME OUT.npz READY_FILE"""
import sys

if __name__ == "__main__":       # (the test imports this module for `request`: the package is on its path already)
    sys.path.insert(0, sys.argv[1])

import numpy as np  # noqa: E402

from gcnn_cut_selector_amd import serve, synthetic, utils  # noqa: E402

ROUNDS = 2
KINDS = (serve.KIND_RANK, serve.KIND_SELECT, serve.KIND_LP_RANK, serve.KIND_LP_SELECT)
N_REQUESTS = ROUNDS * len(KINDS)
PROBLEMS = ("setcov", "capfac", "indset")
MAX_SELECTED = 4
THRESHOLDS = (0.1, 0.5)          # every worker's: selections that wait together can share a call


def request(wid, j):
    """(kind, the state or snapshot, forced rows) of worker wid's j-th request: the kind changes with every request."""
    kind = KINDS[j % len(KINDS)]
    problem = PROBLEMS[(wid + j) % 3]
    rng = np.random.default_rng(100 * wid + j)
    if kind in serve._LP_BASE:
        what = synthetic.make_lp_snapshot(problem, 700 + 20 * wid + j, scale=0.2, incumbent=j % 3 != 0, n_cuts=4 + 5 * j + wid)
        n_vars = int(np.asarray(what.col_type).shape[0])
    else:
        what = utils.state_to_inputs(synthetic.make_sample(problem, 400 + 20 * wid + j, scale=0.2)[0])
        n_vars = int(what[8])
    cols = np.sort(rng.choice(n_vars, size=6, replace=False))
    forced = (np.stack([np.repeat([0, 1], 3), cols]).astype(np.int32), rng.standard_normal(6).astype(np.float32), 2)
    select = serve._LP_BASE.get(kind, kind) == serve.KIND_SELECT
    return kind, what, forced if select and (wid + j) % 2 == 0 else None


def main(address, wid, name, out_path, ready):
    client = serve.ScoringClient(address, name, timeout=100)
    out = {}
    open(ready, "w").close()
    for j in range(N_REQUESTS):
        kind, what, forced = request(wid, j)
        lp, base = kind in serve._LP_BASE, serve._LP_BASE.get(kind, kind)
        if base == serve.KIND_SELECT:
            select = client.select_cuts_lp if lp else client.select_cuts
            res = select(what, forced, p_max=THRESHOLDS[0], p_max_ub=THRESHOLDS[1], max_selected=MAX_SELECTED)
            assert res.n_selected == min(res.n_kept, MAX_SELECTED)
            out[f"s{j}"], out[f"o{j}"], out[f"n{j}"] = res.scores.numpy(), res.order, np.int64(res.n_kept)
            index = res.cut_index
        else:
            q = (client.score_lp if lp else client.score_state)(what, rank=True)
            out[f"s{j}"], out[f"o{j}"] = q.numpy(), q.rankings
            index = q.cut_index
        assert (index is not None) == lp
        if lp:
            out[f"i{j}"] = index
    client.close()
    assert not [m for m in sys.modules if m == "torch" or m.startswith("torch.")]
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6])
