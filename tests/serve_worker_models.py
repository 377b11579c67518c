"""A worker process of tests/test_gpu_mbatch.py: NumPy only, ONE model key of its own (the evaluators' farm with `seed` innermost:
the workers that wait hold different models), stores what it was answered.

usage: serve_worker_models.py ROOT ADDRESS WORKER_ID MODEL_KEY OUT.npz READY_FILE"""
import sys

if __name__ == "__main__":       # (the test imports this module for N_REQUESTS: the package is on its path already)
    sys.path.insert(0, sys.argv[1])

import numpy as np  # noqa: E402

from gcnn_cut_selector_amd import serve  # noqa: E402

from serve_worker_requests import request  # noqa: E402

N_REQUESTS = 6      # kinds cycle score / rank / select; every worker sends the same kind at the same step


def main(address, wid, key, out_path, ready):
    client = serve.ScoringClient(address, key, timeout=100)
    out = {}
    open(ready, "w").close()
    for j in range(N_REQUESTS):
        _, kind, state, (p_max, p_max_ub) = request(wid, j)
        if kind == serve.KIND_SELECT:
            res = client.select_cuts(state, p_max=p_max, p_max_ub=p_max_ub, max_selected=4)
            assert res.n_selected == min(res.n_kept, 4)
            out[f"s{j}"], out[f"o{j}"], out[f"n{j}"] = res.scores.numpy(), res.order, np.int64(res.n_kept)
        else:
            q = client.score_state(state, rank=kind == serve.KIND_RANK)
            out[f"s{j}"] = q.numpy()
            if kind == serve.KIND_RANK:
                out[f"o{j}"] = q.rankings
    client.close()
    assert not [m for m in sys.modules if m == "torch" or m.startswith("torch.")]
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6])
