"""Ensembles (GPU): one state scored by up to 8 models, their mean ranked and selected -- `ops.ensemble_mean`,
`ModelSet.score_ensemble` / `select_cuts_ensemble` and their LP forms through gcnn_infer_ensemble / gcnn_lp_ensemble, and the
general path behind them.

Every layer is held against a path that already exists, bit for bit (`np.array_equal`, no tolerance): the members against
`ModelSet.score_states(keys, [state] * M)` (LP: `score_lps`), the mean against the float32 loop of its definition over those
rows, the rankings against Python's stable sort of the mean, the selection against `ops.select_cuts` on the uploaded mean over
`model.prepare(state).cut_graph`, `cut_index` against `state_from_lp`.  One case is also held against the fp64 oracle at the
project's 1e-4: each member is within 1e-4 of its oracle, so their mean is within 1e-4 of the oracles' mean.

Shapes: K around the wave (63, 64, 65) and block (255, 256, 257) sizes of k_ens_mean and its grid-stride limit, one state past
HOST_RANK_MAX, one past the single call's 32,768 variables and one past the selection's 4,096 cuts."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lpcases  # noqa: E402
from gcnn_cut_selector_amd import _lib, ops, synthetic  # noqa: E402
from gcnn_cut_selector_amd.infer import normalize_forced  # noqa: E402
from gcnn_cut_selector_amd.model import ModelSet  # noqa: E402

from gpucommon import dev, make_model, oracle_scores  # noqa: E402,F401
from test_gpu_ibatch import _forced_like_cuts  # noqa: E402
from test_gpu_select import state_with_cuts  # noqa: E402

N_MODELS = 9                      # eight for the largest ensemble and one more for the refusal of nine keys
KEYS = [f"seed/{i}" for i in range(N_MODELS)]
SIZES = (1, 2, 5, 8)
CUTS = (1, 64, 65, 257)
PROBLEMS = ("setcov", "capfac")
OTHER_THRESHOLDS = (0.9, 0.95)


def mean_loop(rows):
    """The definition: acc = member[0]; acc += member[m] in order; acc / float32(M); every step float32."""
    rows = [np.asarray(r, np.float32) for r in rows]
    if len(rows) == 1:
        return rows[0].copy()
    acc = rows[0].copy()
    with np.errstate(all="ignore"):
        for r in rows[1:]:
            acc = (acc + r).astype(np.float32)
        return (acc / np.float32(len(rows))).astype(np.float32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def farm(dev):  # noqa: F811
    made = [make_model(600 + i, dev) for i in range(N_MODELS)]
    models = {k: m for k, (m, _) in zip(KEYS, made)}
    return dict(models=models, params={k: p for k, (_, p) in zip(KEYS, made)}, mset=ModelSet(models), states={}, members={}, snaps={},
                lp_members={}, alone={})


def _state(farm, problem, K):
    if (problem, K) not in farm["states"]:
        rng = np.random.default_rng(1000 + K)
        farm["states"][problem, K] = state_with_cuts(problem, 3, rng, K, scale=0.2)[0]
    return farm["states"][problem, K]


def _members(farm, problem, K, M):
    """The reference rows: entry m of `ModelSet.score_states(keys, [state] * M)`, computed once per case and never written to."""
    if (problem, K, M) not in farm["members"]:
        rows = farm["mset"].score_states(KEYS[:M], [_state(farm, problem, K)] * M)
        farm["members"][problem, K, M] = np.stack([np.asarray(r) for r in rows])
    return farm["members"][problem, K, M]


def _select_reference(model, state, mean, forced, p_max, p_max_ub):
    """`ops.select_cuts` on the uploaded mean over the prepared state's cut graph."""
    batch = model.prepare(state)
    packed = normalize_forced(forced, batch.dims.n_vars)
    forced_dev = tuple(torch.from_numpy(a).to(model.device) for a in packed)
    order, n_kept = ops.select_cuts(torch.from_numpy(np.ascontiguousarray(mean)).to(model.device), batch.cut_graph, None, forced_dev,
                                    p_max=p_max, p_max_ub=p_max_ub)
    return order.cpu().numpy(), int(n_kept.cpu()[0])


def _single_upload(key, forced_shape, mode):
    """in_bytes of gcnn_infer_batch's upload of this ONE state (+ forced rows in selection mode)."""
    dims = (_lib.Dims * 1)(_lib.Dims(*key))
    nf, nfe = (C.c_int32 * 1)(forced_shape[0]), (C.c_int32 * 1)(forced_shape[1])
    L = _lib.IbatchLayout()
    assert _lib.lib().gcnn_infer_batch_layout_for(1, dims, nf, nfe, mode, C.byref(L)) == 0
    return int(L.in_bytes)


def _key(state):
    return (state[7], state[8], state[9], state[1].shape[1], state[5].shape[1])


# ---- ops.ensemble_mean alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_ensemble_mean_equals_the_float32_loop(dev, M):  # noqa: F811
    rng = np.random.default_rng(40 + M)
    for K in (0, 1, 63, 64, 65, 255, 256, 257, 4096):
        rows = [(rng.standard_normal(K) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(M)]
        got = ops.ensemble_mean([torch.from_numpy(r).to(dev) for r in rows]).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, mean_loop(rows)), (M, K)
        if M == 1:
            assert same(got, rows[0])


def test_ensemble_mean_with_nan_and_infinities(dev):  # noqa: F811
    rng = np.random.default_rng(7)
    rows = [rng.standard_normal(257).astype(np.float32) for _ in range(5)]
    rows[2][10] = np.nan
    rows[0][64] = np.inf
    rows[4][65] = -np.inf
    rows[1][200], rows[3][200] = np.inf, -np.inf            # inf - inf: a NaN mean
    got = ops.ensemble_mean([torch.from_numpy(r).to(dev) for r in rows]).cpu().numpy()
    want = mean_loop(rows)
    assert np.isnan(got[10]) and np.isnan(got[200]) and got[64] == np.inf and got[65] == -np.inf
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(want))
    one = ops.ensemble_mean([torch.from_numpy(rows[2]).to(dev)]).cpu().numpy()
    assert same(one, rows[2])                                # M = 1: the row's own bits, its NaN included
    with pytest.raises(ValueError):
        ops.ensemble_mean([])
    with pytest.raises(ValueError):
        ops.ensemble_mean([torch.zeros(3, device=dev)] * 9)
    with pytest.raises(ValueError):
        ops.ensemble_mean([torch.zeros(3, device=dev), torch.zeros(4, device=dev)])


# ---- the one-call path on host states --------------------------------------------------------------------------------------------
def _check_one_call(farm, problem, K, M, rank=True):
    mset, models = farm["mset"], farm["models"]
    state, keys = _state(farm, problem, K), KEYS[:M]
    ref = _members(farm, problem, K, M)
    want = mean_loop(ref)
    sess = mset.ensemble_session()
    calls, up = sess.calls, sess.upload_bytes
    got = mset.score_ensemble(keys, state, rank=rank)
    assert sess.calls == calls + 1, "exactly one C call"
    mode = _lib.IBATCH_RANK if (rank == "device" or K > models[keys[0]].HOST_RANK_MAX) else _lib.IBATCH_SCORES
    assert sess.upload_bytes - up == _single_upload(_key(state), (0, 0), mode), "the state goes up once, not M times"
    assert got.members.dtype == np.float32 and got.members.shape == (M, K)
    for m in range(M):
        assert same(got.members[m], ref[m]), (problem, K, M, m)
    assert same(np.asarray(got), want), (problem, K, M)
    assert got.rankings.tolist() == sorted(range(K), key=want.tolist().__getitem__, reverse=True)
    return state, keys, want, sess


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("K", CUTS)
@pytest.mark.parametrize("problem", PROBLEMS)
def test_one_call_members_mean_rankings_and_selection(farm, problem, K, M):
    state, keys, want, sess = _check_one_call(farm, problem, K, M)
    first = farm["models"][keys[0]]
    rng = np.random.default_rng(K + M)
    forced = _forced_like_cuts(rng, state, min(3, K))
    for p_max, p_max_ub in ((0.1, 0.5), OTHER_THRESHOLDS):
        calls, up = sess.calls, sess.upload_bytes
        res = farm["mset"].select_cuts_ensemble(keys, state, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=5)
        assert sess.calls == calls + 1
        packed = normalize_forced(forced, state[8])
        assert sess.upload_bytes - up == _single_upload(_key(state), (packed[0].size - 1, packed[1].size), _lib.IBATCH_SELECT)
        assert same(np.asarray(res.scores), want) and same(res.members, _members(farm, problem, K, M))
        order, n_kept = _select_reference(first, state, want, forced, p_max, p_max_ub)
        assert np.array_equal(res.order, order) and res.n_kept == n_kept and res.n_selected == min(n_kept, 5)
    # without forced rows, at the default thresholds
    res = farm["mset"].select_cuts_ensemble(keys, state)
    order, n_kept = _select_reference(first, state, want, None, 0.1, 0.5)
    assert np.array_equal(res.order, order) and res.n_kept == n_kept == res.n_selected


def test_device_ranking_of_the_mean_past_host_rank_max(farm):
    K = 1025
    assert K > next(iter(farm["models"].values())).HOST_RANK_MAX
    _check_one_call(farm, "setcov", K, 5, rank="device")
    # and below it on request
    _check_one_call(farm, "capfac", 65, 2, rank="device")


def test_mean_against_the_fp64_oracle(farm):
    state = _state(farm, "setcov", 65)
    got = farm["mset"].score_ensemble(KEYS[:5], state)
    want = np.mean([oracle_scores(farm["params"][k], state) for k in KEYS[:5]], axis=0)
    np.testing.assert_allclose(np.asarray(got), want, rtol=1e-4, atol=1e-4)


# ---- the LP forms -------------------------------------------------------------------------------------------------------------------
def _snap(farm, problem, K):
    if (problem, K) not in farm["snaps"]:
        snap = synthetic.make_lp_snapshot(problem, 800 + K, scale=0.2, incumbent=K % 2 == 1, n_cuts=K)
        assert int(np.asarray(snap.cut_lhs).shape[0]) == K
        farm["snaps"][problem, K] = snap
        farm["alone"][problem, K] = next(iter(farm["models"].values())).state_from_lp(snap)
    return farm["snaps"][problem, K]


def _lp_members(farm, problem, K, M):
    if (problem, K, M) not in farm["lp_members"]:
        rows = farm["mset"].score_lps(KEYS[:M], [_snap(farm, problem, K)] * M)
        farm["lp_members"][problem, K, M] = np.stack([np.asarray(r) for r in rows])
    return farm["lp_members"][problem, K, M]


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("K", CUTS)
@pytest.mark.parametrize("problem", PROBLEMS)
def test_lp_forms_members_mean_cut_index_and_selection(farm, problem, K, M):
    mset, keys = farm["mset"], KEYS[:M]
    snap = _snap(farm, problem, K)
    state, cut_index = farm["alone"][problem, K]
    ref = _lp_members(farm, problem, K, M)
    want = mean_loop(ref)
    sess = mset.ensemble_session(lp=True)
    calls = sess.calls
    got = mset.score_lp_ensemble(keys, snap, rank=True)
    assert sess.calls == calls + 1
    assert same(got.members, ref) and same(np.asarray(got), want) and np.array_equal(got.cut_index, cut_index)
    assert got.rankings.tolist() == sorted(range(K), key=want.tolist().__getitem__, reverse=True)
    rng = np.random.default_rng(3 * K + M)
    forced = _forced_like_cuts(rng, state, min(2, K))
    first = farm["models"][keys[0]]
    for p_max, p_max_ub in ((0.1, 0.5), OTHER_THRESHOLDS):
        calls, up = sess.calls, sess.upload_bytes
        res = mset.select_cuts_lp_ensemble(keys, snap, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=4)
        assert sess.calls == calls + 1
        # one snapshot's upload: less than two of them would take, whatever M is
        solo = first._lp_batch_session
        assert 0 < sess.upload_bytes - up < 2 * _lp_single_upload(solo, snap, forced, state[8])
        assert same(np.asarray(res.scores), want) and same(res.members, ref) and np.array_equal(res.cut_index, cut_index)
        order, n_kept = _select_reference(first, state, want, forced, p_max, p_max_ub)
        assert np.array_equal(res.order, order) and res.n_kept == n_kept and res.n_selected == min(n_kept, 4)


def _lp_single_upload(session, snap, forced, n_vars):
    """in_bytes of gcnn_lp_batch's upload of this ONE snapshot with its forced rows."""
    _, dims = session.check(snap)
    packed = normalize_forced(forced, n_vars)
    nf, nfe = (C.c_int32 * 1)(packed[0].size - 1), (C.c_int32 * 1)(packed[1].size)
    L = _lib.LpBatchLayout()
    d = (_lib.LpDims * 1)(_lib.LpDims(**dims))
    assert _lib.lib().gcnn_lp_batch_layout_for(1, d, nf, nfe, _lib.IBATCH_SELECT, C.byref(L)) == 0
    return int(L.in_bytes)


def test_lp_upload_is_the_single_snapshot_upload(farm):
    mset = farm["mset"]
    snap = _snap(farm, "setcov", 65)
    state, _ = farm["alone"]["setcov", 65]
    sess = mset.ensemble_session(lp=True)
    first = farm["models"][KEYS[0]]
    first.score_lps([])                                      # the reference session exists
    want = _lp_single_upload(first._lp_batch_session, snap, None, state[8])
    for M in (1, 8):
        up = sess.upload_bytes
        mset.select_cuts_lp_ensemble(KEYS[:M], snap)
        assert sess.upload_bytes - up == want, M


# ---- the general path -----------------------------------------------------------------------------------------------------------------
def test_general_path_gives_the_bits_of_the_one_call_path(farm, dev):  # noqa: F811
    mset, keys = farm["mset"], KEYS[:5]
    state = _state(farm, "setcov", 65)
    forced = _forced_like_cuts(np.random.default_rng(5), state, 3)
    one = mset.score_ensemble(keys, state, rank=True)
    one_sel = mset.select_cuts_ensemble(keys, state, forced, max_selected=7)
    sess = mset.ensemble_session()
    calls = sess.calls
    as_tensors = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in state[:7]) + tuple(state[7:])
    prepared = farm["models"][keys[0]].prepare(state)
    for form in (as_tensors, prepared):
        got = mset.score_ensemble(keys, form, rank=True)
        assert same(np.asarray(got), np.asarray(one)) and same(got.members, one.members)
        assert np.array_equal(got.rankings, one.rankings)
        sel = mset.select_cuts_ensemble(keys, form, forced, max_selected=7)
        assert same(np.asarray(sel.scores), np.asarray(one)) and same(sel.members, one.members)
        assert np.array_equal(sel.order, one_sel.order) and (sel.n_kept, sel.n_selected) == (one_sel.n_kept, one_sel.n_selected)
    assert sess.calls == calls, "device tensors and prepared batches do not take the one-call path"


def test_a_state_the_one_call_path_declines_takes_the_general_path(farm):
    """More than 32,768 variables: gcnn_infer_ensemble_layout_for declines, `prepare` + `forward_group` + `ensemble_mean` answer
    with the bits of `score_states` on the same state (the batched call has no variable limit)."""
    mset, keys = farm["mset"], KEYS[:3]
    c, cei, cef, v, k, kei, kef, nc, nv, nk = _state(farm, "setcov", 64)
    V = 32769
    big_v = np.zeros((V, 14), np.float32)
    big_v[:nv] = v
    big = (c, cei, cef, big_v, k, kei, kef, nc, V, nk)
    L = _lib.EnsembleLayout()
    dims = _lib.Dims(nc, V, nk, cei.shape[1], kei.shape[1])
    assert _lib.lib().gcnn_infer_ensemble_layout_for(C.byref(dims), 0, 0, 0, 3, C.byref(L)) == -4
    ref = np.stack([np.asarray(r) for r in mset.score_states(keys, [big] * 3)])
    sess = mset.ensemble_session()
    calls = sess.calls
    got = mset.score_ensemble(keys, big, rank=True)
    sel = mset.select_cuts_ensemble(keys, big)
    assert sess.calls == calls
    want = mean_loop(ref)
    assert same(got.members, ref) and same(np.asarray(got), want) and same(np.asarray(sel.scores), want)
    order, n_kept = _select_reference(farm["models"][keys[0]], big, want, None, 0.1, 0.5)
    assert np.array_equal(sel.order, order) and sel.n_kept == n_kept


# ---- refusals and empty states ---------------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_work(farm):
    mset = farm["mset"]
    state = _state(farm, "setcov", 64)
    snap = _snap(farm, "setcov", 64)
    sessions = (mset.ensemble_session(), mset.ensemble_session(lp=True))
    calls = [s.calls for s in sessions]
    for keys in ([KEYS[0], KEYS[1], KEYS[0]], [KEYS[0], "nobody"], [], KEYS[:9]):
        for call, arg in ((mset.score_ensemble, state), (mset.select_cuts_ensemble, state), (mset.score_lp_ensemble, snap),
                          (mset.select_cuts_lp_ensemble, snap)):
            with pytest.raises(ValueError):
                call(keys, arg)
    assert [s.calls for s in sessions] == calls


def test_4097_cuts_select_refuses_and_scores_answer(farm):
    mset, keys = farm["mset"], KEYS[:2]
    snap = lpcases.snapshot("cuts4097")
    with pytest.raises(_lib.GcnnError):
        mset.select_cuts_lp_ensemble(keys, snap)
    got = mset.score_lp_ensemble(keys, snap, rank=True)
    ref = np.stack([np.asarray(r) for r in mset.score_lps(keys, [snap] * 2)])
    want = mean_loop(ref)
    assert got.shape == (4097,) and same(got.members, ref) and same(np.asarray(got), want)
    assert np.array_equal(got.rankings, np.argsort(-want, kind="stable"))
    state, cut_index = farm["models"][keys[0]].state_from_lp(snap)
    assert np.array_equal(got.cut_index, cut_index)
    with pytest.raises(_lib.GcnnError):
        mset.select_cuts_ensemble(keys, state)
    host = mset.score_ensemble(keys, state)
    assert same(np.asarray(host), want)


def test_a_state_without_cuts_returns_empty_results(farm):
    mset, keys = farm["mset"], KEYS[:3]
    c, cei, cef, v, k, kei, kef, nc, nv, nk = _state(farm, "setcov", 64)
    empty = (c, cei, cef, v, k[:0], kei[:, :0], kef[:0], nc, nv, 0)
    got = mset.score_ensemble(keys, empty, rank=True)
    assert got.shape == (0,) and got.dtype == np.float32 and got.members.shape == (3, 0) and got.rankings.shape == (0,)
    sel = mset.select_cuts_ensemble(keys, empty)
    assert sel.order.shape == (0,) and sel.n_kept == 0 == sel.n_selected and sel.members.shape == (3, 0)
    snap = _snap(farm, "setcov", 64)
    none = dataclasses.replace(snap, cut_ptr=np.zeros(1, np.int32), cut_col=snap.cut_col[:0], cut_val=snap.cut_val[:0],
                               cut_lhs=snap.cut_lhs[:0], cut_rhs=snap.cut_rhs[:0])
    got = mset.score_lp_ensemble(keys, none)
    assert got.shape == (0,) and got.members.shape == (3, 0) and got.cut_index.shape == (0,)
    sel = mset.select_cuts_lp_ensemble(keys, none)
    assert sel.n_kept == 0 and sel.cut_index.shape == (0,)
