"""LP snapshots of several models in one call (GPU): `ModelSet.score_lps` / `ModelSet.select_cuts_lp_many` through gcnn_lp_models,
and the scoring server on top of it.

The equality reference is the existing path: for every model, `GCNN.score_lps` / `GCNN.select_cuts_lp_many` of that model on its
own snapshots in their relative order -- the same builder bodies, the same plan, the same kernels through their group twins, the
same sub-union -- must match bit for bit (scores, rankings, cut_index, order, n_kept: `np.array_equal`, no tolerance), and every
built state must be `state_from_lp`'s of the snapshot alone.  Every snapshot's scores are also held against the fp64 oracle on its
built state at the project's 1e-4.  Only the server test, whose grouping depends on timing, compares scores with the in-process
single call within the 1e-4 of tests/test_gpu_serve.py.

Snapshots are the seam cases of tests/lpcases.py and small `synthetic.make_lp_snapshot`s (scale <= 0.3): the smallest shapes at
which the builder and the per-model split change path."""
import dataclasses
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
import lpcases  # noqa: E402
import serve_worker_lp as W  # noqa: E402
from gcnn_cut_selector_amd import _lib, serve, synthetic  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN, ModelSet  # noqa: E402

from gpucommon import dev, make_model, oracle_scores as _oracle  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MODELS = 9
SEAMS = ("rows257", "cuts513", "cols257", "rows1", "cuts256", "rows600", "cuts1100", "cuts255", "cuts257", "rows255", "rows256",
         "cols255", "cols256")
PROBLEMS = ("setcov", "indset", "capfac")


def _pool_snapshot(i):
    """Snapshot i of the pool: the seam cases first, then small synthetic ones of three problems, every third without an incumbent."""
    if i < len(SEAMS):
        return lpcases.snapshot(SEAMS[i])
    return synthetic.make_lp_snapshot(PROBLEMS[i % 3], 700 + i, scale=(0.2, 0.3)[i % 2], incumbent=i % 3 != 0, n_cuts=3 + (5 * i) % 23)


@pytest.fixture(scope="module")
def farm(dev):  # noqa: F811
    """Nine models with distinct seeds, their parameters, 70 snapshots, and caches that are computed once and never written to:
    `alone` -- (state, cut_index) of `state_from_lp` on a snapshot alone, by tag --, `oracle` -- fp64 scores by (model, tag)."""
    made = [make_model(400 + i, dev) for i in range(N_MODELS)]
    names = [f"setcov/{i}" for i in range(N_MODELS)]
    return dict(names=names, models={n: m for n, (m, _) in zip(names, made)}, params={n: p for n, (_, p) in zip(names, made)},
                snaps=[_pool_snapshot(i) for i in range(70)], alone={}, oracle={})


def _alone(farm, snap, tag):
    """`state_from_lp` of the snapshot alone (the state does not depend on the model)."""
    if tag not in farm["alone"]:
        farm["alone"][tag] = next(iter(farm["models"].values())).state_from_lp(snap)
    return farm["alone"][tag]


def _fp64(farm, key, snap, tag):
    if (key, tag) not in farm["oracle"]:
        farm["oracle"][key, tag] = _oracle(farm["params"][key], _alone(farm, snap, tag)[0])
    return farm["oracle"][key, tag]


def _same_state(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:7], b[:7]))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _forced_for(n_vars, seed):
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(n_vars, size=6, replace=False))
    return (np.stack([np.repeat([0, 1], 3), cols]).astype(np.int32), rng.standard_normal(6).astype(np.float32), 2)


def _own_calls(models, used):
    for k in used:                                   # the reference sessions exist, so that their call counts can be read
        models[k].score_lps([])
    return {k: models[k]._lp_batch_session.calls for k in used}


def _check(farm, keys, snaps, tags, forced=None, thresholds=(0.1, 0.5), mset=None, calls=1, select=True, fp64=True):
    """One `ModelSet` call per entry point against every model's own call on its own snapshots, the built states against
    `state_from_lp` alone, and (`fp64`) the scores against the fp64 oracle."""
    models = farm["models"]
    used = list(dict.fromkeys(keys))
    mset = mset or ModelSet({k: models[k] for k in used})
    p_max, p_max_ub = thresholds
    before = _own_calls(models, used)
    calls0 = mset.calls
    scored = mset.score_lps(keys, snaps, rank=True)
    assert mset.calls == calls0 + calls and mset.max_models_per_call == min(len(used), 8)
    if calls == 1:
        # the arena holds the call's states in the call's order: sorted stably by model
        number = {k: m for m, k in enumerate(mset.models)}
        order = sorted(range(len(keys)), key=lambda i: number[keys[i]])
        built = mset._sess(lp=True).last_states()
        assert len(built) == len(order)
        for have, i in zip(built, order):
            assert _same_state(have, _alone(farm, snaps[i], tags[i])[0]), (keys[i], tags[i])
    selected = mset.select_cuts_lp_many(keys, snaps, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=5) if select else None
    assert mset.calls == calls0 + calls * (2 if select else 1)
    # it went through gcnn_lp_models: no model's own LP batch session was called
    assert {k: models[k]._lp_batch_session.calls for k in used} == before
    for k in used:
        mine = [i for i, key in enumerate(keys) if key == k]
        ref = models[k].score_lps([snaps[i] for i in mine], rank=True)
        ref_sel = models[k].select_cuts_lp_many([snaps[i] for i in mine], None if forced is None else [forced[i] for i in mine],
                                                p_max=p_max, p_max_ub=p_max_ub, max_selected=5) if select else None
        for j, i in enumerate(mine):
            q, index = scored[i], _alone(farm, snaps[i], tags[i])[1]
            assert q.dtype == np.float32 and q.shape == index.shape, (k, i)
            assert _same(q, ref[j]) and np.array_equal(q.rankings, ref[j].rankings), (k, i)
            assert np.array_equal(q.cut_index, ref[j].cut_index) and np.array_equal(q.cut_index, index), (k, i)
            assert list(q.rankings) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (k, i)
            if select:
                s, r = selected[i], ref_sel[j]
                assert _same(s.scores, r.scores) and _same(s.scores, q), (k, i)
                assert np.array_equal(s.order, r.order) and (s.n_kept, s.n_selected) == (r.n_kept, r.n_selected), (k, i)
                assert np.array_equal(s.cut_index, index) and sorted(np.asarray(s.order).tolist()) == list(range(len(q))), (k, i)
            if fp64:
                np.testing.assert_allclose(q.numpy(), _fp64(farm, k, snaps[i], tags[i]), rtol=1e-4, atol=1e-4)
    return scored, selected


def _interleaved(farm, M, S):
    """S snapshots of the pool on M models, keys interleaved in descending order: sorting by model moves every snapshot."""
    names = farm["names"]
    return [names[(M - 1 - i) % M] for i in range(S)], farm["snaps"][:S], list(range(S))


@pytest.mark.parametrize("S", [1, 3])
def test_one_model(farm, S):
    _check(farm, *_interleaved(farm, 1, S))


@pytest.mark.parametrize("M,S", [(M, S) for M in (2, 3, 5, 8) for S in (M, 17, 64)])
def test_same_bits_as_each_models_own_call_and_fp64(farm, M, S):
    _check(farm, *_interleaved(farm, M, S))


@pytest.mark.parametrize("with_forced", [False, True])
@pytest.mark.parametrize("p_max,p_max_ub", [(0.1, 0.5), (0.0, 0.0), (2.0, 2.0)])
def test_selection_thresholds_and_forced_rows(farm, p_max, p_max_ub, with_forced):
    names = farm["names"]
    at = (13, 1, 14, 3, 15, 5, 16)                   # seam cases and synthetic ones, alternating
    snaps = [farm["snaps"][i] for i in at]
    keys = [names[i] for i in (2, 0, 1, 2, 0, 1, 2)]
    forced = [_forced_for(s.col_type.shape[0], i) if i % 3 else None for i, s in enumerate(snaps)] if with_forced else None
    _, selected = _check(farm, keys, snaps, list(at), forced, (p_max, p_max_ub))
    removed = sum(len(res.order) - res.n_kept for res in selected)
    assert removed == 0 if p_max == 2.0 else (removed > 0 or p_max > 0.0)
    if not with_forced:                              # valid on the reply's own scores, from the restated filter
        for s in (0, 3):
            state = _alone(farm, snaps[s], at[s])[0]
            rec = {}
            order, n = R.select(selected[s].scores, R.dense_rows(state[5][0], state[5][1], state[6].reshape(-1), state[9], state[8]), None,
                                p_max, p_max_ub, record=rec)
            if R.margins_ok(rec, p_max, p_max_ub):
                assert np.array_equal(selected[s].order, order) and selected[s].n_kept == n, s


def _without_rows(snap):
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    return dataclasses.replace(snap, row_ptr=np.zeros(1, np.int32), row_col=z(np.int32), row_val=z(np.float64), row_lhs=z(np.float64),
                               row_rhs=z(np.float64), row_dual=z(np.float64), row_basis=z(np.int8))


def _without_cuts(snap):
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    return dataclasses.replace(snap, cut_ptr=np.zeros(1, np.int32), cut_col=z(np.int32), cut_val=z(np.float64), cut_lhs=z(np.float64),
                               cut_rhs=z(np.float64))


def _one_cut(snap):
    n = int(snap.cut_ptr[1])
    return dataclasses.replace(snap, cut_ptr=snap.cut_ptr[:2].copy(), cut_col=snap.cut_col[:n].copy(), cut_val=snap.cut_val[:n].copy(),
                               cut_lhs=snap.cut_lhs[:1].copy(), cut_rhs=snap.cut_rhs[:1].copy())


def _drop_columns(snap, cols):
    """The snapshot without the row entries of `cols`: those variables have degree 0 among the constraint edges."""
    keep = ~np.isin(snap.row_col, cols)
    rows = np.repeat(np.arange(snap.row_lhs.shape[0]), np.diff(snap.row_ptr))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=snap.row_lhs.shape[0]))]).astype(np.int32)
    assert ptr[-1] < snap.row_ptr[-1]
    return dataclasses.replace(snap, row_ptr=ptr, row_col=snap.row_col[keep], row_val=snap.row_val[keep])


def test_seams_of_the_per_model_split(farm):
    names, pool = farm["names"], farm["snaps"]
    a, b, c = names[:3]
    s = [pool[i] for i in (13, 14, 15, 16, 17, 3)]
    t = [13, 14, 15, 16, 17, 3]
    # a middle model whose only snapshot has no LP rows: no constraint, no constraint edge, its forward pass alone behind the group's
    _check(farm, [a, b, c, a], [s[0], _without_rows(s[1]), s[2], s[3]], [t[0], "norows14", t[2], t[3]])
    _check(farm, [b, a], [_without_rows(s[1]), s[0]], ["norows14", t[0]])
    # a middle model whose only snapshot has one cut; in front and behind as well
    _check(farm, [a, b, c], [s[0], _one_cut(s[1]), s[2]], [t[0], "onecut14", t[2]])
    _check(farm, [b, a, c, c], [_one_cut(s[0]), s[1], _one_cut(s[2]), s[3]], ["onecut13", t[1], "onecut15", t[3]])
    # a model whose first and last variable have degree 0: its first snapshot loses column 0, its last one its last column
    last = s[3].col_type.shape[0] - 1
    _check(farm, [a, b, b, c], [s[0], _drop_columns(s[1], [0]), _drop_columns(s[3], [last]), s[2]], [t[0], "first14", "last16", t[2]])
    only = s[4].col_type.shape[0] - 1
    _check(farm, [b, a, c], [_drop_columns(s[4], [0, only]), s[0], s[5]], ["ends17", t[0], t[5]])       # ... and of its only snapshot
    # the same GCNN under two keys: one parameter pointer twice in one call
    m = farm["models"][names[2]]
    twin = dict(farm, models={"x": m, "y": m}, params={"x": farm["params"][names[2]], "y": farm["params"][names[2]]})
    _check(twin, ["y", "x", "x", "y", "x"], s[:5], t[:5])


def test_zero_block_and_arena_are_reusable(farm):
    names, pool = farm["names"][:3], farm["snaps"]
    models = {k: farm["models"][k] for k in names}
    big_keys = [names[i % 3] for i in range(12)]
    big = [pool[i] for i in (6, 5, 1, 0, 13, 14, 15, 16, 2, 3, 4, 17)]
    small_keys, small = [names[2], names[0], names[1]], [pool[3], pool[7], pool[2]]
    mset = ModelSet(models)
    mset.select_cuts_lp_many(big_keys, big, max_selected=5)
    mset.score_lps(big_keys, big, rank=True)
    again = mset.score_lps(small_keys, small, rank=True)
    again_sel = mset.select_cuts_lp_many(small_keys, small, max_selected=5)
    fresh_models = {}
    for k, m in models.items():                      # fresh sessions: fresh pinned buffers and a fresh arena
        fresh_models[k] = GCNN(device=m.device)
        fresh_models[k].set_weights(m.get_weights())
    fresh_set = ModelSet(fresh_models)
    fresh = fresh_set.score_lps(small_keys, small, rank=True)
    fresh_sel = fresh_set.select_cuts_lp_many(small_keys, small, max_selected=5)
    assert mset.calls == 4 and fresh_set.calls == 2
    for a, b in zip(again, fresh):
        assert _same(a, b) and np.array_equal(a.rankings, b.rankings) and np.array_equal(a.cut_index, b.cut_index)
    for a, b in zip(again_sel, fresh_sel):
        assert np.array_equal(a.order, b.order) and a.n_kept == b.n_kept and _same(a.scores, b.scores)


def test_isolation(farm):
    names, models, pool = farm["names"], farm["models"], farm["snaps"]
    a, b, c = names[:3]
    good = [pool[i] for i in (13, 0, 14, 15, 3)]
    out_of_range = dataclasses.replace(pool[16], cut_col=pool[16].cut_col.copy())
    out_of_range.cut_col[0] = 10 ** 6                          # passes the host's cheap check; the device flags it
    not_finite = dataclasses.replace(pool[17], obj_norm=float("nan"))
    snaps = [good[0], out_of_range, good[1], not_finite, good[2], good[3], pool[18], good[4]]
    keys = [a, b, c, b, b, a, "nobody", c]
    # The run without them: the two snapshots that never reach the device left out, the one the device flags replaced by its
    # intact original, so that model b's sub-union has the same sizes (a state's score bits may depend on its neighbours' sizes
    # through the forward pass's dispatch choice; they must not depend on what a flagged neighbour holds)
    clean_at = [0, 2, 4, 5, 7]
    with_original = sorted(clean_at + [1])
    mset = ModelSet({k: models[k] for k in (a, b, c)})
    clean = mset.score_lps([keys[i] for i in with_original], [pool[16] if i == 1 else snaps[i] for i in with_original], rank=True)
    clean_sel = mset.select_cuts_lp_many([keys[i] for i in with_original], [pool[16] if i == 1 else snaps[i] for i in with_original],
                                         max_selected=5)
    clean, clean_sel = ([r for i, r in zip(with_original, res) if i != 1] for res in (clean, clean_sel))
    scored = mset.score_lps(keys, snaps, rank=True, return_exceptions=True)
    selected = mset.select_cuts_lp_many(keys, snaps, max_selected=5, return_exceptions=True)
    assert mset.calls == 4 and mset.max_models_per_call == 3
    for res in (scored, selected):
        assert isinstance(res[1], ValueError) and "outside" in str(res[1])
        assert isinstance(res[3], ValueError) and "obj_norm finite" in str(res[3])
        assert isinstance(res[6], KeyError) and "nobody" in str(res[6])
    # every other snapshot keeps the bits of the run without the three
    for j, i in enumerate(clean_at):
        assert _same(scored[i], clean[j]) and np.array_equal(scored[i].rankings, clean[j].rankings), i
        assert np.array_equal(scored[i].cut_index, clean[j].cut_index), i
        assert np.array_equal(selected[i].order, clean_sel[j].order) and selected[i].n_kept == clean_sel[j].n_kept, i
    # without return_exceptions the first error is raised, after the others were served
    with pytest.raises(ValueError, match="outside"):
        mset.score_lps(keys[:3], snaps[:3])
    assert mset.calls == 5
    assert mset.score_lps([], []) == [] and mset.select_cuts_lp_many([], []) == []
    with pytest.raises(ValueError, match="one model key per state"):
        mset.score_lps([a], good[:2])


def test_admission_and_splitting(farm):
    names, models, pool = farm["names"], farm["models"], farm["snaps"]
    a, b, c = names[:3]
    huge, empty = lpcases.snapshot("cuts4097"), _without_cuts(pool[14])
    keys, snaps = [a, b, b, c, a], [pool[13], empty, huge, pool[15], pool[3]]
    mset = ModelSet({k: models[k] for k in (a, b, c)})
    scored = mset.score_lps(keys, snaps, rank=True)
    selected = mset.select_cuts_lp_many(keys, snaps, max_selected=5, return_exceptions=True)
    assert mset.calls == 2 and mset.max_models_per_call == 2            # b's two snapshots went through b's own solo entry points
    alone = models[b].score_lp(huge, rank=True)
    assert _same(scored[2], alone) and np.array_equal(scored[2].rankings, alone.rankings) and np.array_equal(scored[2].cut_index, alone.cut_index)
    assert scored[1].shape == (0,) and scored[1].cut_index.shape == (0,)
    assert isinstance(selected[2], _lib.GcnnError) and "4097" in str(selected[2])
    own = models[b].select_cuts_lp_many([empty, huge], max_selected=5, return_exceptions=True)
    assert type(own[1]) is type(selected[2]) and type(own[0]) is type(selected[1])
    if not isinstance(own[0], Exception):
        assert selected[1].n_kept == own[0].n_kept == 0 and len(selected[1].order) == len(own[0].order) == 0
    rest = [0, 3, 4]
    without = mset.score_lps([keys[i] for i in rest], [snaps[i] for i in rest], rank=True)
    without_sel = mset.select_cuts_lp_many([keys[i] for i in rest], [snaps[i] for i in rest], max_selected=5)
    for j, i in enumerate(rest):
        assert _same(scored[i], without[j]) and np.array_equal(scored[i].rankings, without[j].rankings)
        assert np.array_equal(selected[i].order, without_sel[j].order) and selected[i].n_kept == without_sel[j].n_kept


def test_nine_models_and_seventy_snapshots_take_several_calls(farm):
    names = farm["names"]
    keys = [names[(i * 4 + 3) % 9] for i in range(70)]
    mset = ModelSet(farm["models"])
    # 8 models first, then the ninth.  Bits against every model's own call, as everywhere; no fp64 comparison here: this pairing
    # puts "cuts255" on the model of seed 404, whose scores on it reach 2,175 in magnitude and hold one value of -9.6 that the
    # oracle ITSELF, evaluated in fp32, gives 1.8e-3 away from its fp64 value -- at 1e-4 that comparison would measure the number
    # format on a cancelling sum, not the call (which returns that model's own bits, 5.5e-3 away).
    _check(farm, keys, farm["snaps"], list(range(70)), mset=mset, calls=2, fp64=False)
    assert mset.max_models_per_call == 8


def test_launch_record_of_same_shaped_snapshots(farm):
    names, models = farm["names"], farm["models"]
    snap = farm["snaps"][14]
    records = {}
    for M in (2, 5, 8):
        used = names[:M]
        mset = ModelSet({k: models[k] for k in used})
        for call, tail in ((lambda: mset.score_lps(used, [snap] * M), []),
                           (lambda: mset.score_lps(used, [snap] * M, rank=True), ["k_mb_rank"]),
                           (lambda: mset.select_cuts_lp_many(used, [snap] * M), ["k_sel_pairs", "k_sel_filter"])):
            call()                                                               # buffers and layouts exist
            with _lib.launch_profile() as prof:
                call()
            got = [n for n, _ in prof.launches]
            assert got[:3] == ["k_lpm_stats", "k_lpm_emit", "k_mb_unpack"], got
            assert got[len(got) - len(tail):] == tail, got
            assert not [n for n in got if n.startswith(("k_lpset_", "k_lp_", "k_ib_"))], got
            records.setdefault(len(tail), {})[M] = got
    # the same record whatever the number of models, and, behind the two builder launches, gcnn_infer_models' own
    for by_m in records.values():
        assert by_m[2] == by_m[5] == by_m[8]
    state = _alone(farm, snap, 14)[0]
    mset = ModelSet({k: models[k] for k in names[:5]})
    mset.score_states(names[:5], [state] * 5)
    with _lib.launch_profile() as plain:
        mset.score_states(names[:5], [state] * 5)
    assert records[0][5][2:] == [n for n, _ in plain.launches]


def test_server_with_eight_lp_workers_of_eight_models(farm, tmp_path):
    """Eight torch-free workers that open no GPU, one per model key, send LP score, rank and select requests and one bad snapshot
    each (tests/serve_worker_lp.py's requests)."""
    keys = farm["names"][:8]
    models = {k: farm["models"][k] for k in keys}
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer(models, address)
    worker = os.path.join(ROOT, "tests", "serve_worker_lpmodels.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), str(tmp_path / f"w{w}.npz"),
                               str(tmp_path / f"ready{w}"), keys[w]]) for w in range(8)]
    try:
        # first requests queued before start(): the first sweep finds eight requests of eight models waiting
        deadline = time.time() + 100
        while not all(os.path.exists(tmp_path / f"ready{w}") for w in range(8)):
            assert time.time() < deadline and all(p.poll() is None for p in procs), "a worker did not get ready"
            time.sleep(0.02)
        time.sleep(0.3)
        server.start()
        codes = [p.wait(timeout=130) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * 8
    stats = server.stats
    assert stats["errors"] == 8 and stats["requests"] == 8 * (W.N_REQUESTS + 1)
    assert stats["batched_calls"] >= 1 and stats["max_batch"] >= 2, stats
    if server.cross_model and server.cross_model_lp:
        assert stats["max_models_per_call"] > 1 and stats["calls"] < stats["requests"], stats
    else:
        assert stats["max_models_per_call"] == 1, stats
    for w in range(8):
        model = models[keys[w]]
        got = np.load(tmp_path / f"w{w}.npz")
        for j in range(W.N_REQUESTS):
            kind, snap, forced = W.lp_request(w, j)
            q, index = got[f"s{j}"], got[f"i{j}"]
            assert q.dtype == np.float32 and index.dtype == np.int32
            if kind == "select":
                direct = model.select_cuts_lp(snap, forced, p_max=0.1, p_max_ub=0.5, max_selected=4)
                np.testing.assert_allclose(q, direct.scores.numpy(), rtol=1e-4, atol=1e-4)
                assert np.array_equal(index, direct.cut_index)
                state = model.state_from_lp(snap)[0]
                K, V = state[9], state[8]
                frows = None if forced is None else R.dense_rows(forced[0][0], forced[0][1], forced[1], forced[2], V)
                rec = {}
                order, n = R.select(q, R.dense_rows(state[5][0], state[5][1], state[6].reshape(-1), K, V), frows, 0.1, 0.5, record=rec)
                assert sorted(got[f"o{j}"].tolist()) == list(range(K))
                if R.margins_ok(rec, 0.1, 0.5):       # (a parallelism on a threshold is the restatement's to decline, not a failure)
                    assert np.array_equal(got[f"o{j}"], order) and int(got[f"n{j}"]) == n, (w, j)
            else:
                direct = model.score_lp(snap)
                np.testing.assert_allclose(q, direct.numpy(), rtol=1e-4, atol=1e-4)
                assert np.array_equal(index, direct.cut_index)
                if kind == "rank":
                    assert list(got[f"o{j}"]) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (w, j)
