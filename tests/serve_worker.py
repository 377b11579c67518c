"""A worker process of tests/test_gpu_serve.py: NumPy only, talks to the scoring server and stores what it was answered.

usage: serve_worker.py ROOT ADDRESS WORKER_ID OUT.npz READY_FILE"""
import sys

ROOT, ADDRESS, WID, OUT, READY = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gcnn_cut_selector_amd import serve  # noqa: E402

from serve_worker_requests import N_REQUESTS, request  # noqa: E402


def main():
    client = serve.ScoringClient(ADDRESS, "a", timeout=200)
    f = client.get_concrete_function()
    out = {}
    open(READY, "w").close()
    for j in range(N_REQUESTS):
        key, kind, state, (p_max, p_max_ub) = request(WID, j)
        client.model_key = key
        if kind == serve.KIND_SELECT:
            res = client.select_cuts(state, p_max=p_max, p_max_ub=p_max_ub, max_selected=4)
            assert res.n_selected == min(res.n_kept, 4)
            out[f"s{j}"], out[f"o{j}"], out[f"n{j}"] = res.scores.numpy(), res.order, np.int64(res.n_kept)
        else:
            q = f(state, False, rank=kind == serve.KIND_RANK)
            out[f"s{j}"] = q.numpy()
            if kind == serve.KIND_RANK:
                out[f"o{j}"] = q.rankings
        if j == 7 and WID % 2 == 0:
            # requests that must fail, each followed by one that must not: a bad index, an unknown model, a message that is not one
            bad = list(state); bad[1] = bad[1].copy(); bad[1][1, 0] = state[8]
            for attempt, want in ((lambda: client.score_state(tuple(bad)), ValueError), (None, serve.ServerError)):
                try:
                    if attempt is None:
                        client.model_key = "no such model"
                        client.score_state(state)
                    else:
                        attempt()
                except want as exc:
                    assert want is not ValueError or "out of range" in str(exc), exc
                else:
                    raise AssertionError("the server answered a bad request")
                client.model_key = key
                assert np.array_equal(client.score_state(state).numpy(), client.score_state(state).numpy())
            try:
                client._call(b"this is no request")
            except ValueError as exc:            # ProtocolError travels as a ValueError
                assert "ProtocolError" in str(exc), exc
            else:
                raise AssertionError("the server answered garbage")
            assert client.score_state(state).shape == (state[9],)
    client.close()
    assert not [m for m in sys.modules if m == "torch" or m.startswith("torch.")]
    np.savez(OUT, **out)


main()
