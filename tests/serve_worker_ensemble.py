"""A worker process of tests/test_gpu_ensemble_serve.py: NumPy only.  It sends host states and LP snapshots under an ensemble's
name and under a plain model key, interleaved, through the kinds 0-5 as they are, and stores what it was answered; half-way it
asks for something an ensemble's name cannot have (a resident LP) and goes on after the error reply.

usage: serve_worker_ensemble.py ROOT ADDRESS WORKER_ID ENSEMBLE_NAME MODEL_KEY OUT.npz READY_FILE"""
import sys

if __name__ == "__main__":       # (the test imports this module for `request`: the package is on its path already)
    sys.path.insert(0, sys.argv[1])

import numpy as np  # noqa: E402

from gcnn_cut_selector_amd import lpstate, serve, synthetic, utils  # noqa: E402

N_REQUESTS = 12     # per worker: (ensemble, plain) x (host state, LP snapshot) x (score, rank, select)
PROBLEMS = ("setcov", "capfac")
MAX_SELECTED = 4


def request(wid, j):
    """(under the ensemble's name?, from an LP snapshot?, kind 0 / 1 / 2, the state or snapshot, forced rows, thresholds) of
    worker wid's j-th request: the name alternates with every request, the form every two, the kind every four."""
    ens, lp, kind = j % 2 == 0, (j // 2) % 2 == 1, (j // 4) % 3
    problem = PROBLEMS[(wid + j) % 2]
    thresholds = ((0.1, 0.5), (0.3, 0.6))[(wid + j // 2) % 2]
    rng = np.random.default_rng(100 * wid + j)
    if lp:
        what = synthetic.make_lp_snapshot(problem, 900 + 20 * wid + j, scale=0.2, incumbent=j % 3 != 0, n_cuts=5 + 7 * j)
        n_vars = int(np.asarray(what.col_type).shape[0])
    else:
        what = utils.state_to_inputs(synthetic.make_sample(problem, 300 + 20 * wid + j, scale=0.2)[0])
        n_vars = int(what[8])
    cols = np.sort(rng.choice(n_vars, size=6, replace=False))
    forced = (np.stack([np.repeat([0, 1], 3), cols]).astype(np.int32), rng.standard_normal(6).astype(np.float32), 2)
    return ens, lp, kind, what, forced if kind == 2 and wid == 0 else None, thresholds     # worker 1 selects without forced rows


def main(address, wid, name, key, out_path, ready):
    clients = {True: serve.ScoringClient(address, name, timeout=100), False: serve.ScoringClient(address, key, timeout=100)}
    out = {}
    open(ready, "w").close()
    for j in range(N_REQUESTS):
        ens, lp, kind, what, forced, (p_max, p_max_ub) = request(wid, j)
        client = clients[ens]
        if j == N_REQUESTS // 2:
            # a request that must fail -- an ensemble has no resident LP -- followed, below, by one that must not
            rows = lpstate.LPRows.from_snapshot(synthetic.make_lp_snapshot("setcov", 5, scale=0.2, n_cuts=3))
            try:
                clients[True].open_lp(rows)
                raise AssertionError("the open under an ensemble's name was answered")
            except serve.ServerError as exc:
                out["refused"] = np.frombuffer(str(exc).encode(), np.uint8)
        if kind == serve.KIND_SELECT:
            select = client.select_cuts_lp if lp else client.select_cuts
            res = select(what, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=MAX_SELECTED)
            assert res.n_selected == min(res.n_kept, MAX_SELECTED)
            out[f"s{j}"], out[f"o{j}"], out[f"n{j}"] = res.scores.numpy(), res.order, np.int64(res.n_kept)
            index = res.cut_index
        else:
            q = (client.score_lp if lp else client.score_state)(what, rank=kind == serve.KIND_RANK)
            out[f"s{j}"] = q.numpy()
            if kind == serve.KIND_RANK:
                out[f"o{j}"] = q.rankings
            index = q.cut_index
        assert (index is not None) == lp
        if lp:
            out[f"i{j}"] = index
    for client in clients.values():
        client.close()
    assert not [m for m in sys.modules if m == "torch" or m.startswith("torch.")]
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6], sys.argv[7])
