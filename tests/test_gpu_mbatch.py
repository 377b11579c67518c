"""States of several models in one call (GPU): `ModelSet.score_states` / `ModelSet.select_cuts_many` through gcnn_infer_models, and the
scoring server on top of it.

The equality reference is the existing path: for every model, `GCNN.score_states` / `GCNN.select_cuts_many` of that model on its own
states in their relative order -- the same plan, the same kernels through their group twins, the same sub-union -- must match bit
for bit (scores, rankings, order, n_kept: `np.array_equal`, no tolerance).  Every state is also held against the fp64 oracle at
the project's 1e-4."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
from gcnn_cut_selector_amd import _lib, serve, synthetic, utils  # noqa: E402
from gcnn_cut_selector_amd.model import ModelSet  # noqa: E402

import serve_worker_models as WM  # noqa: E402
import serve_worker_requests as W  # noqa: E402
from gpucommon import dev, make_model, oracle_scores as _oracle  # noqa: E402,F401
from test_gpu_ibatch import _bad_states, _forced_like_cuts, _mixed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32
N_MODELS = 9


@pytest.fixture(scope="module")
def farm(dev):
    """Nine models with distinct seeds, their parameters, 70 mixed states, and a cache of fp64 scores by (model, state)."""
    made = [make_model(300 + i, dev) for i in range(N_MODELS)]
    names = [f"setcov/{i}" for i in range(N_MODELS)]
    return dict(names=names, models={n: m for n, (m, _) in zip(names, made)}, params={n: p for n, (_, p) in zip(names, made)},
                states=_mixed(70, first=500), oracle={})


def _sample(problem, seed, scale):
    return utils.state_to_inputs(synthetic.make_sample(problem, seed, scale=scale)[0])


def _fp64(farm, key, inp, tag=None):
    if tag is None:
        return _oracle(farm["params"][key], inp)
    if (key, tag) not in farm["oracle"]:
        farm["oracle"][key, tag] = _oracle(farm["params"][key], inp)
    return farm["oracle"][key, tag]


def _check(farm, keys, inputs, forced=None, thresholds=(0.1, 0.5), tags=None, mset=None, calls=1, select=True):
    """One `ModelSet` call per entry point against every model's own call on its own states, and against fp64."""
    models = farm["models"]
    used = list(dict.fromkeys(keys))
    mset = mset or ModelSet({k: models[k] for k in used})
    p_max, p_max_ub = thresholds
    for k in used:                                   # the reference sessions exist, so that their call counts can be read
        models[k].score_states([])
    before = {k: models[k]._batch_session.calls for k in used}
    scored = mset.score_states(keys, inputs, rank=True)
    assert mset.calls == calls and mset.max_models_per_call == min(len(used), 8)
    selected = mset.select_cuts_many(keys, inputs, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=5) if select else None
    assert mset.calls == calls * (2 if select else 1)
    # it went through gcnn_infer_models: no model's own batch session was called
    assert {k: models[k]._batch_session.calls for k in used} == before
    for k in used:
        mine = [i for i, key in enumerate(keys) if key == k]
        ref = models[k].score_states([inputs[i] for i in mine], rank=True)
        ref_sel = models[k].select_cuts_many([inputs[i] for i in mine], None if forced is None else [forced[i] for i in mine],
                                             p_max=p_max, p_max_ub=p_max_ub, max_selected=5) if select else None
        for j, i in enumerate(mine):
            q = scored[i]
            assert q.dtype == f32 and q.shape == (inputs[i][9],), (k, i)
            assert np.array_equal(q.numpy(), ref[j].numpy()), (k, i)
            assert np.array_equal(q.rankings, ref[j].rankings), (k, i)
            assert list(q.rankings) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (k, i)
            if select:
                s, r = selected[i], ref_sel[j]
                assert np.array_equal(s.scores.numpy(), r.scores.numpy()) and np.array_equal(s.scores.numpy(), q.numpy()), (k, i)
                assert np.array_equal(s.order, r.order) and s.n_kept == r.n_kept and s.n_selected == r.n_selected, (k, i)
                assert sorted(np.asarray(s.order).tolist()) == list(range(inputs[i][9])), (k, i)
            np.testing.assert_allclose(q.numpy(), _fp64(farm, k, inputs[i], None if tags is None else tags[i]), rtol=1e-4, atol=1e-4)
    return scored, selected


def _interleaved(farm, M, S):
    """S states of the pool on M models, keys interleaved in descending order: sorting by model moves every state."""
    names = farm["names"]
    keys = [names[(M - 1 - i) % M] for i in range(S)]
    return keys, farm["states"][:S], list(range(S))


@pytest.mark.parametrize("S", [1, 3])
def test_one_model(farm, S):
    keys, inputs, tags = _interleaved(farm, 1, S)
    _check(farm, keys, inputs, tags=tags)


@pytest.mark.parametrize("M,S", [(M, S) for M in (2, 3, 5, 8) for S in (M, 17, 64)])
def test_same_bits_as_each_models_own_call_and_fp64(farm, M, S):
    keys, inputs, tags = _interleaved(farm, M, S)
    _check(farm, keys, inputs, tags=tags)


def test_one_state_beside_many_and_a_shared_parameter_buffer(farm):
    names, pool = farm["names"], farm["states"]
    keys = [names[1]] * 4 + [names[0]] + [names[1]] * 5
    _check(farm, keys, pool[20:30])
    # two keys, one GCNN: the same parameter pointer twice in one call
    m = farm["models"][names[2]]
    twin = dict(farm, models={"x": m, "y": m}, params={"x": farm["params"][names[2]], "y": farm["params"][names[2]]})
    _check(twin, ["y", "x", "x", "y", "x"], pool[30:35])


def test_members_of_different_regimes(farm):
    names = farm["names"]
    # row sets past 256 tiles with 4/8-wave row programs beside four-waves-per-tile programs; long segments beside short ones
    _check(farm, [names[0], names[1]], [_sample("capfac", 31, 1.0), _sample("setcov", 32, 0.2)])
    _check(farm, [names[1], names[0], names[2]], [_sample("setcov", 33, 0.2), _sample("combauc", 34, 1.0), _sample("setcov", 35, 0.5)])


def _without_cons_edges(inp):
    c, cei, cef, v, k, kei, kef, nc, nv, nk = inp
    return (c, np.zeros((2, 0), i32), np.zeros((0, 1), f32), v, k, kei, kef, nc, nv, nk)


def _drop_variables(inp, drop):
    c, cei, cef, v, k, kei, kef, nc, nv, nk = inp
    keep = ~np.isin(cei[1], drop)
    return (c, cei[:, keep], cef[keep], v, k, kei, kef, nc, nv, nk)


def _one_cut(inp):
    c, cei, cef, v, k, kei, kef, nc, nv, nk = inp
    keep = kei[0] == 0
    return (c, cei, cef, v, k[:1], kei[:, keep], kef[keep], nc, nv, 1)


def test_seams_of_the_per_model_split(farm):
    names = farm["names"]
    a, b, c = names[:3]
    s = [_sample(("setcov", "indset", "capfac")[i % 3], 40 + i, 0.2) for i in range(8)]
    # a model whose states have no constraint edges between two that have
    _check(farm, [a, b, c, b, a, c], [s[0], _without_cons_edges(s[1]), s[2], _without_cons_edges(s[3]), s[4], s[5]])
    # first and last variable of a model with degree 0 (the middle model's first state loses variable 0, its last state its last)
    first, last = _drop_variables(s[1], [0]), _drop_variables(s[3], [s[3][8] - 1])
    assert first[1].shape[1] < s[1][1].shape[1] and last[1].shape[1] < s[3][1].shape[1]
    _check(farm, [a, b, b, c], [s[0], first, last, s[2]])
    _check(farm, [b, a, c], [_drop_variables(s[6], [0, s[6][8] - 1]), s[0], s[2]])      # ... and of a model's only state
    # a model's only state with one cut, in front, between and behind
    _check(farm, [b, a, c], [_one_cut(s[1]), s[0], s[2]])
    _check(farm, [a, b, c], [_one_cut(s[0]), s[1], _one_cut(s[2])])


def _without_constraints(inp):
    c, cei, cef, v, k, kei, kef, nc, nv, nk = inp
    return (np.zeros((0, 4), f32), np.zeros((2, 0), i32), np.zeros((0, 1), f32), v, k, kei, kef, 0, nv, nk)


def test_a_degenerate_member_takes_its_solo_path_inside_the_call(farm):
    """A model whose sub-union has no constraints is no group member: its forward pass runs alone behind the group's launches,
    in the same call, with the bits of its own call."""
    names = farm["names"]
    a, b, c = names[:3]
    s = [_sample(("setcov", "indset", "capfac")[i % 3], 60 + i, 0.2) for i in range(4)]
    _check(farm, [a, b, c, a], [s[0], _without_constraints(s[1]), s[2], s[3]])      # between two regular members
    _check(farm, [b, a], [_without_constraints(s[1]), s[0]])                          # in front
    _check(farm, [a], [_without_constraints(s[3])])                                   # and with no regular member at all


@pytest.mark.parametrize("p_max,p_max_ub", [(0.1, 0.5), (0.0, 0.0), (2.0, 2.0)])
def test_forced_rows_per_state(farm, p_max, p_max_ub):
    names, rng = farm["names"], np.random.default_rng(11)
    inputs = farm["states"][40:47]
    keys = [names[i] for i in (2, 0, 1, 2, 0, 1, 2)]
    counts = (0, 1, 40, 0, 3, 40, 2)
    forced = [None if F == 0 and s == 0 else _forced_like_cuts(rng, inp, F) for s, (inp, F) in enumerate(zip(inputs, counts))]
    _, selected = _check(farm, keys, inputs, forced, (p_max, p_max_ub))
    removed = sum(inp[9] - res.n_kept for inp, res in zip(inputs, selected))
    assert removed == 0 if p_max == 2.0 else (removed > 0 or p_max > 0.0)
    # valid on the reply's own scores, from the restated filter (no forced rows there: the unforced states)
    for s in (0, 3):
        rec = {}
        inp = inputs[s]
        order, n = R.select(selected[s].scores, R.dense_rows(inp[5][0], inp[5][1], inp[6].reshape(-1), inp[9], inp[8]), None,
                            p_max, p_max_ub, record=rec)
        if R.margins_ok(rec, p_max, p_max_ub):
            assert np.array_equal(selected[s].order, order) and selected[s].n_kept == n, s


def test_isolation(farm):
    names, models = farm["names"], farm["models"]
    a, b, c = names[:3]
    bad_index, unsorted, huge, hub = _bad_states(np.random.default_rng(7))
    clean = farm["states"][50:55]
    inputs = [clean[0], bad_index, clean[1], unsorted, huge, clean[2], hub, clean[3], clean[4]]
    keys = [a, b, c, b, b, a, b, b, c]                       # every bad state belongs to model b
    mset = ModelSet({k: models[k] for k in (a, b, c)})
    scored = mset.score_states(keys, inputs, rank=True, return_exceptions=True)
    selected = mset.select_cuts_many(keys, inputs, return_exceptions=True)
    assert mset.calls == 2 and mset.max_models_per_call == 3
    assert isinstance(scored[1], ValueError) and "out of range" in str(scored[1]) and isinstance(selected[1], ValueError)
    assert isinstance(selected[4], _lib.GcnnError) and "4097" in str(selected[4])
    solo = models[b].score_state(huge, rank=True)             # the 4,097-cut state went through its own model's score_state
    assert np.array_equal(scored[4].numpy(), solo.numpy()) and np.array_equal(scored[4].rankings, solo.rankings)
    # every state of the OTHER models keeps the bits of its model's own call; so do b's states next to b's own call on them
    for k in (a, c, b):
        mine = [i for i, key in enumerate(keys) if key == k]
        ref = models[k].score_states([inputs[i] for i in mine], rank=True, return_exceptions=True)
        ref_sel = models[k].select_cuts_many([inputs[i] for i in mine], return_exceptions=True)
        for j, i in enumerate(mine):
            if isinstance(ref[j], Exception):
                assert type(scored[i]) is type(ref[j]) and type(selected[i]) is type(ref_sel[j]), (k, i)
                continue
            assert np.array_equal(scored[i].numpy(), ref[j].numpy()) and np.array_equal(scored[i].rankings, ref[j].rankings), (k, i)
            if not isinstance(ref_sel[j], Exception):
                assert np.array_equal(selected[i].order, ref_sel[j].order) and selected[i].n_kept == ref_sel[j].n_kept, (k, i)
            if i != 4:      # (the 4,097-cut state is its model's solo answer, compared above)
                np.testing.assert_allclose(scored[i].numpy(), _oracle(farm["params"][k], inputs[i]), rtol=1e-4, atol=1e-4)
    # without return_exceptions the error is raised, after the others were served
    with pytest.raises(ValueError, match="out of range"):
        mset.score_states(keys[:3], inputs[:3])
    assert mset.calls == 3
    # an unknown key is its own state's error; an empty call is empty; a state without cuts comes back in place
    got = mset.score_states([a, "nobody", c], [clean[0], clean[1], clean[1]], return_exceptions=True)
    assert isinstance(got[1], KeyError) and np.array_equal(got[0].numpy(), models[a].score_states([clean[0]])[0].numpy())
    assert mset.score_states([], []) == [] and mset.select_cuts_many([], []) == []
    empty = clean[1][:4] + (np.zeros((0, 6), f32), np.zeros((2, 0), i32), np.zeros((0, 1), f32)) + clean[1][7:9] + (0,)
    got = mset.score_states([a, b, a], [clean[0], empty, clean[2]], rank=True)
    assert got[1].shape == (0,) and np.array_equal(got[2].numpy(), models[a].score_states([clean[0], clean[2]])[1].numpy())
    with pytest.raises(ValueError, match="one model key per state"):
        mset.score_states([a], [clean[0], clean[1]])


def test_one_device_or_a_value_error(farm):
    class Elsewhere:
        device = "cuda:7"
    with pytest.raises(ValueError, match="one device"):
        ModelSet({"a": farm["models"][farm["names"][0]], "b": Elsewhere()})
    with pytest.raises(ValueError):
        ModelSet({})


def test_nine_models_and_seventy_states_take_several_calls(farm):
    names = farm["names"]
    keys = [names[(i * 4 + 3) % 9] for i in range(70)]
    mset = ModelSet(farm["models"])
    _check(farm, keys, farm["states"], mset=mset, calls=2)                     # 8 models first, then the ninth; scores, ranks, selection


def test_launch_profile_of_five_same_shaped_states(farm):
    names, models = farm["names"][:5], farm["models"]
    state = _sample("setcov", 77, 0.2)
    mset = ModelSet({k: models[k] for k in names})
    mset.score_states(names, [state] * 5, rank=True)                            # buffers and layouts exist
    models[names[0]].score_states([state])
    with _lib.launch_profile() as solo:
        models[names[0]].score_states([state])
    forward_solo = [n for n, _ in solo.launches if n not in ("k_ib_unpack", "k_ib_by_variable")]
    assert len(forward_solo) >= 6, solo.launches
    for call, tail in ((lambda: mset.score_states(names, [state] * 5), []),
                       (lambda: mset.score_states(names, [state] * 5, rank="device"), ["k_mb_rank"]),
                       (lambda: mset.select_cuts_many(names, [state] * 5), ["k_sel_pairs", "k_sel_filter"])):
        with _lib.launch_profile() as prof:
            call()
        got = [n for n, _ in prof.launches]
        assert got[:3] == ["k_mb_unpack", "k_mb_by_variable", "k_mb_vptr"], got     # one index pass, one by-variable stage
        assert [got.count(n) for n in got[:3]] == [1, 1, 1], got
        forward = got[3:len(got) - len(tail)]
        assert got[len(got) - len(tail):] == tail, got
        # five members, every stage ONE launch of a group kernel: as many launches as one solo inference forward has
        assert all(n.startswith("k_group_") for n in forward) and len(forward) == len(forward_solo), (got, forward_solo)
        assert not [n for n in got if n in ("k_ib_unpack", "k_check_edges", "k_ib_rank") or n.startswith("k_infer_s")], got


def _serve_eight(tmp_path, models, cross_model):
    keys = list(models)
    address = str(tmp_path / f"gcnn{int(cross_model)}.sock")
    server = serve.ScoringServer(models, address, cross_model=cross_model)
    worker = os.path.join(ROOT, "tests", "serve_worker_models.py")
    tag = f"c{int(cross_model)}"
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), keys[w],
                               str(tmp_path / f"{tag}w{w}.npz"), str(tmp_path / f"{tag}ready{w}")]) for w in range(8)]
    try:
        # first requests queued before start(): the first sweep finds eight requests of eight models waiting
        deadline = time.time() + 100
        while not all(os.path.exists(tmp_path / f"{tag}ready{w}") for w in range(8)):
            assert time.time() < deadline and all(p.poll() is None for p in procs), "a worker did not get ready"
            time.sleep(0.02)
        time.sleep(0.3)
        assert server.stats["requests"] == 0
        server.start()
        codes = [p.wait(timeout=130) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * 8
    for w in range(8):
        got = np.load(tmp_path / f"{tag}w{w}.npz")
        for j in range(WM.N_REQUESTS):
            _, kind, state, (p_max, p_max_ub) = W.request(w, j)
            q = got[f"s{j}"]
            assert q.dtype == f32 and q.shape == (state[9],)
            np.testing.assert_allclose(q, models[keys[w]].score_state(state).numpy(), rtol=1e-4, atol=1e-4)
            if kind == serve.KIND_SELECT:
                rec = {}
                order, n = R.select(q, R.dense_rows(state[5][0], state[5][1], state[6].reshape(-1), state[9], state[8]), None,
                                    p_max, p_max_ub, record=rec)
                assert R.margins_ok(rec, p_max, p_max_ub), (w, j)
                assert np.array_equal(got[f"o{j}"], order) and int(got[f"n{j}"]) == n, (w, j)
            elif kind == serve.KIND_RANK:
                assert list(got[f"o{j}"]) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (w, j)
    assert server.stats["errors"] == 0 and server.stats["requests"] == 8 * WM.N_REQUESTS
    return server.stats


def test_server_with_eight_workers_of_eight_models(farm, tmp_path):
    models = {k: farm["models"][k] for k in farm["names"][:8]}
    stats = _serve_eight(tmp_path, models, True)
    assert stats["max_models_per_call"] >= 2 and stats["calls"] < stats["requests"], stats
    stats = _serve_eight(tmp_path, models, False)
    assert stats["max_models_per_call"] == 1, stats
