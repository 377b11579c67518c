"""A resident LP scored by an ensemble (GPU): `ModelSet.open_lp_ensemble` -> `infer.LPEnsembleSession` through
gcnn_lp_round_ensemble.

Every equality is on bytes (`np.array_equal`, dtype and shape included; no tolerance).  By definition a round's result is what
`ModelSet.score_lp_ensemble` / `select_cuts_lp_ensemble` give for the same keys on `lpstate.assemble(rows after the call's edits,
round)` -- mean, members, rankings or order, n_kept, n_selected, cut_index --, `members[m]` is what model m's own plain session
returns, the mean is the float32 loop of its definition over those rows, and the session afterwards holds what a plain
`LPSession` holds that received the same calls.  One case is also held against the fp64 oracle at the project's 1e-4: each member
is within 1e-4 of its oracle, so their mean is within 1e-4 of the oracles' mean.

Shapes (scale 0.2): K = 0, 1, around the 16-byte seam of a member's row (3, 4, 5), around a wave (64, 65) and a block (257) of
the mean's launch, K = 1,025 (ranked on the device), 4,097 (past the orders), an LP of 32,769 columns (past the one-shot call's
variable limit), a state without constraint rows (the group's degenerate members)."""
import dataclasses

import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

import lpappendcases as A  # noqa: E402
import lpcases  # noqa: E402
import lpremovecases as D  # noqa: E402
import lpsessioncases as S  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate, synthetic  # noqa: E402
from gcnn_cut_selector_amd.infer import LPEnsembleSession, LPSession, LPSessionGroup  # noqa: E402
from gcnn_cut_selector_amd.model import ModelSet  # noqa: E402

from gpucommon import dev, make_model, oracle_scores  # noqa: E402,F401

N_MODELS = 9                      # eight for the largest ensemble and one more for the refusal of nine keys
KEYS = [f"seed/{i}" for i in range(N_MODELS)]
SIZES = (1, 2, 5, 8)
CUTS = (0, 1, 3, 4, 5, 64, 65, 257)
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


def same_scores(got, want, rank):
    assert same(got, want) and same(got.members, want.members) and same(got.cut_index, want.cut_index)
    if rank:
        assert same(got.rankings, want.rankings)


def same_selection(got, want):
    assert same(got.scores, want.scores) and same(got.members, want.members) and same(got.order, want.order)
    assert (got.n_kept, got.n_selected) == (want.n_kept, want.n_selected) and same(got.cut_index, want.cut_index)


def same_state(a, b):
    (sa, ia), (sb, ib) = a, b
    return all(same(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(sa, sb)) and same(ia, ib)


class GuardedEnsembleSession(LPEnsembleSession):
    GUARD = 256


@pytest.fixture(scope="module")
def farm(dev):  # noqa: F811
    made = [make_model(600 + i, dev) for i in range(N_MODELS)]
    models = {k: m for k, (m, _) in zip(KEYS, made)}
    return dict(models=models, params={k: p for k, (_, p) in zip(KEYS, made)}, mset=ModelSet(models), snaps={}, members={})


def _snap(farm, problem, K):
    """(snapshot, its rows, its round): built once per (problem, K) and never written to."""
    if (problem, K) not in farm["snaps"]:
        snap = synthetic.make_lp_snapshot(problem, 800 + K, scale=0.2, incumbent=K % 2 == 1, n_cuts=max(K, 1))
        if K == 0:                    # (the generator draws at least one cut: a round without cuts is that LP with its cut dropped)
            snap = dataclasses.replace(snap, cut_ptr=np.zeros(1, np.int32), cut_col=np.zeros(0, np.int32), cut_val=np.zeros(0),
                                       cut_lhs=np.zeros(0), cut_rhs=np.zeros(0))
        assert int(np.asarray(snap.cut_lhs).shape[0]) == K
        farm["snaps"][problem, K] = (snap,) + S.split(snap)
    return farm["snaps"][problem, K]


def _plain_members(farm, problem, K, M):
    """Row m: what model m's own plain session returns for the round; computed once per case."""
    if (problem, K, M) not in farm["members"]:
        _, rows, rnd = _snap(farm, problem, K)
        out = []
        for k in KEYS[:M]:
            sess = farm["models"][k].open_lp(rows)
            out.append(np.asarray(sess.score(rnd)).copy())
            sess.close()
        farm["members"][problem, K, M] = np.stack(out) if out else None
    return farm["members"][problem, K, M]


def _forced(n_cols, seed=5, n=3, per=2):
    rng = np.random.default_rng(seed)
    per = min(per, n_cols)
    cols = np.concatenate([np.sort(rng.choice(n_cols, size=per, replace=False)) for _ in range(n)])
    return (np.stack([np.repeat(np.arange(n), per), cols]).astype(np.int32), rng.standard_normal(n * per).astype(np.float32), n)


def _open(farm, M, rows, guarded=True, **kw):
    models = farm["mset"]._ensemble_models(KEYS[:M])
    return (GuardedEnsembleSession if guarded else LPEnsembleSession)(models, rows, **kw)


# ---- plain rounds ------------------------------------------------------------------------------------------------------------------
def test_open_lp_ensemble_scores_a_round_as_the_one_shot_call(farm):
    """(fails without the feature: there is no `open_lp_ensemble`)"""
    snap, rows, rnd = _snap(farm, "setcov", 65)
    mset = farm["mset"]
    sess = mset.open_lp_ensemble(KEYS[:5], rows)
    assert isinstance(sess, LPEnsembleSession) and isinstance(sess, LPSession) and sess.models == [farm["models"][k] for k in KEYS[:5]]
    assert sess.model is farm["models"][KEYS[0]] and sess.n_rows == np.asarray(rows.row_lhs).shape[0]
    same_scores(sess.score(rnd, rank=True), mset.score_lp_ensemble(KEYS[:5], snap, rank=True), True)
    same_selection(sess.select_cuts(rnd, max_selected=4), mset.select_cuts_lp_ensemble(KEYS[:5], snap, max_selected=4))
    assert same_state(sess.state(rnd), farm["models"][KEYS[0]].state_from_lp(snap))
    sess.close()
    with pytest.raises(_lib.GcnnError):
        sess.score(rnd)


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("K", CUTS)
@pytest.mark.parametrize("problem", PROBLEMS)
def test_plain_rounds(farm, problem, K, M):
    mset, keys = farm["mset"], KEYS[:M]
    snap, rows, rnd = _snap(farm, problem, K)
    sess = _open(farm, M, rows)
    calls = sess.calls
    got = sess.score(rnd, rank=True)
    assert sess.calls == calls + 1                                     # one C call per round
    same_scores(got, mset.score_lp_ensemble(keys, snap, rank=True), True)
    same_scores(sess.score(rnd), mset.score_lp_ensemble(keys, snap), False)
    # the members against M plain sessions, the mean against the float32 loop, M = 1: the member's own bits
    if K:
        ref = _plain_members(farm, problem, K, M)
        assert same(got.members, ref) and same(np.asarray(got), mean_loop(ref))
        if M == 1:
            assert same(np.asarray(got), ref[0])
    else:
        assert got.members.shape == (M, 0) and got.shape == (0,)
    forced = _forced(sess.n_cols, seed=3 * K + M, n=min(2, max(K, 1)))
    for p_max, p_max_ub in ((0.1, 0.5), OTHER_THRESHOLDS):
        calls = sess.calls
        res = sess.select_cuts(rnd, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=4)
        assert sess.calls == calls + 1
        same_selection(res, mset.select_cuts_lp_ensemble(keys, snap, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=4))
    same_selection(sess.select_cuts(rnd), mset.select_cuts_lp_ensemble(keys, snap))
    assert sess.guards_intact()
    sess.close()


def test_device_ranking_of_the_mean_past_host_rank_max(farm):
    K = 1025
    assert K > next(iter(farm["models"].values())).HOST_RANK_MAX
    snap, rows, rnd = _snap(farm, "setcov", K)
    sess = _open(farm, 5, rows)
    with _lib.launch_profile() as prof:
        got = sess.score(rnd, rank=True)
    assert "k_rank_scores" in [n for n, _ in prof.launches]
    same_scores(got, farm["mset"].score_lp_ensemble(KEYS[:5], snap, rank=True), True)
    want = np.asarray(got)
    assert got.rankings.tolist() == sorted(range(K), key=want.tolist().__getitem__, reverse=True)
    # and below it on request
    snap, rows, rnd = _snap(farm, "capfac", 65)
    small = _open(farm, 2, rows)
    same_scores(small.score(rnd, rank="device"), farm["mset"].score_lp_ensemble(KEYS[:2], snap, rank="device"), True)
    assert sess.guards_intact() and small.guards_intact()


def test_mean_against_the_fp64_oracle(farm):
    snap, rows, rnd = _snap(farm, "setcov", 65)
    state, _ = farm["models"][KEYS[0]].state_from_lp(snap)
    sess = _open(farm, 5, rows)
    got = sess.score(rnd)
    want = np.mean([oracle_scores(farm["params"][k], state) for k in KEYS[:5]], axis=0)
    np.testing.assert_allclose(np.asarray(got), want, rtol=1e-4, atol=1e-4)


# ---- sequences of rounds on one session ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k_sequence", "none_rules"))
def test_a_sequence_of_rounds_on_one_session(farm, name):
    """K = 600 -> 5 -> 0 -> 513 -> 1,100 through one session, and the optional column arrays kept across rounds."""
    steps = S.case(name)
    mset, keys = farm["mset"], KEYS[:5]
    sess = _open(farm, 5, steps[0][1])
    for i, (_, rnd, snap) in enumerate(steps[1:]):
        forced = _forced(sess.n_cols, seed=i)
        same_selection(sess.select_cuts(rnd, forced, max_selected=7), mset.select_cuts_lp_ensemble(keys, snap, forced, max_selected=7))
        same_scores(sess.score(rnd, rank=True), mset.score_lp_ensemble(keys, snap, rank=True), True)
        assert sess.guards_intact()
    sess.close()


# ---- edits inside the call -----------------------------------------------------------------------------------------------------------
def _lockstep(farm, M, rows, before):
    """An ensemble session and a plain session of model 0 on the same rows, both after the same first round."""
    sess, twin = _open(farm, M, rows), farm["models"][KEYS[0]].open_lp(rows)
    sess.score(before)
    twin.score(before)
    return sess, twin


def _check_edit(farm, M, sess, twin, rnd, snap, forced=None, **edit):
    keys = KEYS[:M]
    got = sess.select_cuts(rnd, forced, max_selected=5, **edit)
    twin.select_cuts(rnd, forced, max_selected=5, **edit)
    same_selection(got, farm["mset"].select_cuts_lp_ensemble(keys, snap, forced, max_selected=5))
    assert sess.n_rows == twin.n_rows
    assert same_state(sess.state(rnd), twin.state(rnd))
    a, b = sess.resident_state(), twin.resident_state()
    assert all(np.array_equal(a[n], b[n], equal_nan=True) for n in a)
    assert sess.guards_intact()
    return got


def _fused_case(idx, seed):
    c = A.case("kinds")
    after = lpstate.rows_without(lpstate.rows_with(c.rows, c.block), idx)
    rnd = A._round_for(np.random.default_rng(seed), after, c.snap)
    return c, np.asarray(idx), rnd, lpstate.assemble(after, rnd)


@pytest.mark.parametrize("M", (1, 5))
def test_an_append_a_removal_and_both_in_one_call(farm, M):
    c = A.case("kinds")
    sess, twin = _lockstep(farm, M, c.rows, c.before)
    _check_edit(farm, M, sess, twin, c.rnd, c.snap, _forced(sess.n_cols), append=c.block)
    d = D.case("kinds")
    sess, twin = _lockstep(farm, M, d.rows, d.before)
    _check_edit(farm, M, sess, twin, d.rnd, d.snap, _forced(sess.n_cols), remove=d.idx)
    c, idx, rnd, snap = _fused_case([2, 44, 9, 49, 40], 31)
    sess, twin = _lockstep(farm, M, c.rows, c.before)
    _check_edit(farm, M, sess, twin, rnd, snap, _forced(sess.n_cols), append=c.block, remove=idx)
    # the scoring entry with both edits, ranked
    sess, twin = _lockstep(farm, M, c.rows, c.before)
    got = sess.score(rnd, rank=True, append=c.block, remove=idx)
    twin.score(rnd, rank=True, append=c.block, remove=idx)
    same_scores(got, farm["mset"].score_lp_ensemble(KEYS[:M], snap, rank=True), True)
    assert same_state(sess.state(rnd), twin.state(rnd)) and sess.guards_intact()


def test_six_rounds_of_the_separation_loop(farm):
    """Each round appends the cuts the previous selection kept and, once there are enough, removes three earlier cut rows."""
    M = 5
    rng, base, pools = A.loop_script(n_rounds=6)
    pick = np.random.default_rng(181)
    rows = lpstate.LPRows.from_snapshot(base)
    n_base = np.asarray(rows.row_lhs).shape[0]
    sess, twin = _open(farm, M, rows), farm["models"][KEYS[0]].open_lp(rows)
    forced = _forced(64, seed=9)
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    block, removals = None, 0
    for i, pool in enumerate(pools):
        idx = None
        if block is not None:
            rows = lpstate.rows_with(rows, block)
            n = np.asarray(rows.row_lhs).shape[0]
            if n - n_base >= 6:
                idx = n_base + pick.choice(n - n_base, size=3, replace=False)
                rows = lpstate.rows_without(rows, idx)
                removals += 1
        rnd = lpstate.LPRound(**S._solve(rng, rows, 64, col_lp=base.col_lp), **S._cuts_of(pool), **(full if i % 4 == 0 else {}),
                              has_incumbent=True)
        got = _check_edit(farm, M, sess, twin, rnd, lpstate.assemble(rows, rnd, full), forced, append=block, remove=idx)
        block = A.cuts_as_rows(pool, got.cut_index[got.order[:got.n_selected]])
        assert np.asarray(block.row_lhs).shape[0] == got.n_selected > 0
    assert removals >= 3


@pytest.mark.parametrize("name", ("free_only", "free_left"))
def test_free_rows_removed_and_only_free_rows_left(farm, name):
    """free_only: only free rows leave, so no state row moves.  free_left: only free rows stay -- the state has no constraint
    rows, so every member takes the group's degenerate path (its solo launches inside the call)."""
    d = D.case(name)
    if name == "free_left":
        assert lpstate.check_rows(lpstate.rows_without(d.rows, d.idx), True)[1]["n_state_rows"] == 0
    for M in (1, 5):
        sess, twin = _lockstep(farm, M, d.rows, d.before)
        _check_edit(farm, M, sess, twin, d.rnd, d.snap, _forced(sess.n_cols), remove=d.idx)
        same_scores(sess.score(d.rnd, rank=True), farm["mset"].score_lp_ensemble(KEYS[:M], d.snap, rank=True), True)


def test_an_lp_past_the_one_shot_calls_variable_limit(farm):
    snap = lpcases._make(seed=63, R=6, V=32769, K=9, short_rows=True)
    rows, rnd = S.split(snap)
    sess = _open(farm, 5, rows)
    assert sess.n_cols == 32769
    same_scores(sess.score(rnd, rank=True), farm["mset"].score_lp_ensemble(KEYS[:5], snap, rank=True), True)
    forced = _forced(sess.n_cols)
    same_selection(sess.select_cuts(rnd, forced), farm["mset"].select_cuts_lp_ensemble(KEYS[:5], snap, forced))
    assert sess.guards_intact()


# ---- what the session must not do -------------------------------------------------------------------------------------------------
def test_the_session_follows_a_members_weights(farm, dev):  # noqa: F811
    from oracle import gcnn_oracle as O
    snap, rows, rnd = _snap(farm, "setcov", 64)
    own = {k: make_model(700 + i, dev)[0] for i, k in enumerate(KEYS[:3])}
    mset = ModelSet(own)
    sess = mset.open_lp_ensemble(KEYS[:3], rows)
    first = sess.score(rnd)
    same_scores(first, mset.score_lp_ensemble(KEYS[:3], snap), False)
    params = O.randomize_params(O.init_params(5, np.float32), 6)
    own[KEYS[1]].set_weights([params[n] for n in O.PARAM_NAMES])
    second = sess.score(rnd)
    same_scores(second, mset.score_lp_ensemble(KEYS[:3], snap), False)
    assert same(second.members[0], first.members[0]) and same(second.members[2], first.members[2])
    assert not same(second.members[1], first.members[1]) and not same(second, first)


def test_a_flagged_round_raises_and_leaves_the_session_as_it_was(farm):
    """deep=False: the device finds the cut column out of range.  The round raises, the append that came with it is not adopted,
    and the next round equals a fresh session's."""
    c = A.case("kinds")
    M, keys = 5, KEYS[:5]
    sess = _open(farm, M, c.rows, deep=False)
    first = sess.score(c.before, rank=True)
    R0, V = sess.n_rows, sess.n_cols
    bad = dataclasses.replace(c.rnd, cut_col=np.where(np.arange(c.rnd.cut_col.size) == 3, V + 5, c.rnd.cut_col))
    with pytest.raises(ValueError, match="outside"):
        sess.select_cuts(bad, append=c.block)
    assert sess.n_rows == R0 and sess.guards_intact()
    plain = dataclasses.replace(c.before, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    fresh = _open(farm, M, c.rows, deep=False)
    fresh.score(c.before)
    same_scores(sess.score(plain, rank=True), fresh.score(plain, rank=True), True)
    same_scores(sess.score(plain, rank=True), first, True)
    a, b = sess.resident_state(), fresh.resident_state()
    assert all(np.array_equal(a[n], b[n], equal_nan=True) for n in a)
    # the same edit with a sound round then succeeds
    same_selection(sess.select_cuts(c.rnd, append=c.block), farm["mset"].select_cuts_lp_ensemble(keys, c.snap))
    assert sess.n_rows == R0 + np.asarray(c.block.row_lhs).shape[0] and sess.guards_intact()


def test_4097_cuts_select_refuses_and_scores_answer(farm):
    snap = lpcases._make(seed=64, R=8, V=300, K=4097, short_rows=False)
    rows, rnd = S.split(snap)
    sess = _open(farm, 2, rows)
    calls = sess.calls
    with pytest.raises(_lib.GcnnError, match="4097"):
        sess.select_cuts(rnd)
    assert sess.calls == calls
    same_scores(sess.score(rnd, rank=True), farm["mset"].score_lp_ensemble(KEYS[:2], snap, rank=True), True)
    small = lpcases._make(seed=64, R=8, V=300, K=5, short_rows=False)
    rnd5 = lpstate.LPRound.from_snapshot(small)
    same_selection(sess.select_cuts(rnd5), farm["mset"].select_cuts_lp_ensemble(KEYS[:2], lpstate.assemble(rows, rnd5)))
    assert sess.guards_intact()


def test_refusals_before_any_device_work(farm):
    snap, rows, rnd = _snap(farm, "setcov", 5)
    mset = farm["mset"]
    for bad in ([], KEYS, [KEYS[0], KEYS[0]], [KEYS[0], "nobody"]):
        with pytest.raises(ValueError):
            mset.open_lp_ensemble(bad, rows)
    sess = mset.open_lp_ensemble(KEYS[:2], rows)
    plain = farm["models"][KEYS[0]].open_lp(rows)
    group = LPSessionGroup(sess.model.device)
    for call in (lambda: group.score([sess, plain], [rnd, rnd]), lambda: group.select_cuts([plain, sess], [rnd, rnd]),
                 lambda: mset.score_rounds([KEYS[0], KEYS[0]], [sess, plain], [rnd, rnd]),
                 lambda: mset.select_cuts_rounds([KEYS[0]], [sess], [rnd])):
        with pytest.raises(ValueError, match="ensemble"):
            call()
    assert group.calls == 0 and sess.calls == 0


# ---- counts ---------------------------------------------------------------------------------------------------------------------------
def test_upload_bytes_and_launches_do_not_depend_on_the_number_of_models(farm):
    snap, rows, rnd = _snap(farm, "capfac", 65)
    forced = _forced(np.asarray(rows.col_obj).shape[0])
    plain = farm["models"][KEYS[0]].open_lp(rows)
    packed = (np.asarray([0, 2, 4, 6], np.int32), np.zeros(6, np.int32), np.zeros(6, np.float32))      # three forced rows of two entries
    want_bytes = plain.upload_bytes(rnd, packed)
    t_plain = {}
    plain.select_cuts(rnd, forced, timings=t_plain)
    assert t_plain["upload_bytes"] == want_bytes
    with _lib.launch_profile() as prof:
        plain.select_cuts(rnd, forced)
    plain_names = [n for n, _ in prof.launches]
    lists = {}
    for M in (1, 8):
        sess = _open(farm, M, rows, guarded=False)
        sess.select_cuts(rnd, forced)
        timings, calls = {}, sess.calls
        with _lib.launch_profile() as prof:
            sess.select_cuts(rnd, forced, timings=timings)
        assert sess.calls == calls + 1
        assert timings["upload_bytes"] == want_bytes == sess.upload_bytes(rnd, packed)
        lists[M] = [n for n, _ in prof.launches]
    assert len(lists[1]) == len(lists[8])
    # the round's two state launches once, the forward passes under the group's names, one mean, the plain round's tail
    for names in lists.values():
        assert names[:2] == plain_names[:2] == ["k_lpr_stats", "k_lpr_emit"] and names.count("k_ens_mean") == 1
        forward = names[2:names.index("k_ens_mean")]
        assert forward and all(n.startswith("k_group_") for n in forward)
        assert len(forward) == len(plain_names) - 2 - len(names[names.index("k_ens_mean") + 1:])
        assert names[names.index("k_ens_mean") + 1:] == plain_names[len(plain_names) - len(names[names.index("k_ens_mean") + 1:]):]
