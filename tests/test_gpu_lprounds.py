"""Rounds of several resident LPs in one call (`infer.LPSessionGroup`, gcnn_lp_rounds; csrc/k_lprounds.hpp) on the GPU.  The oracle
of every member is a twin `LPSession` that gets the same sequence through solo calls: results, the resident state and the host's
bookkeeping are compared with `np.array_equal`.  No tolerance anywhere."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lpappendcases as A  # noqa: E402
import lpcases  # noqa: E402
import lpsessioncases as S  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate  # noqa: E402
from gcnn_cut_selector_amd.infer import LPSession, LPSessionGroup  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

SCALARS = ("l_max_deg", "v_max_deg", "n_rows", "n_state_rows", "n_state_edges")
ARRAYS = ("cons_feats", "row_place", "row_scale", "l_ptr", "edge_row", "edge_col", "edge_coef", "v_ptr", "v_oth", "v_coef")
EMPTY_FORCED = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))


@pytest.fixture(scope="module")
def model(dev):  # noqa: F811
    return make_model(93, dev)[0]


@pytest.fixture(scope="module")
def model2(dev):  # noqa: F811
    return make_model(17, dev)[0]


class GuardedSession(LPSession):
    GUARD = 256


class GuardedGroup(LPSessionGroup):
    GUARD = 256


def _same_resident(sess, other, bookkeeping=True):
    """The resident state and, with `bookkeeping`, everything the host keeps beside it (capacities, the current set, the kept and
    stale optional arrays, the per-column degrees)."""
    a, b = sess.resident_state(), other.resident_state()
    for name in SCALARS:
        assert a[name] == b[name], name
    for name in ARRAYS:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name], equal_nan=True), name
    assert sess.n_rows == other.n_rows and sess._lhs == other._lhs and sess._max_deg == other._max_deg
    assert np.array_equal(sess._col_deg, other._col_deg)
    if not bookkeeping:
        return
    assert (sess.n_rows, sess._lhs, sess._max_deg, sess._cap) == (other.n_rows, other._lhs, other._max_deg, other._cap)
    assert sess._cur_set == other._cur_set and sess._stale == other._stale and sorted(sess._kept) == sorted(other._kept)
    for name in sess._kept:
        assert np.array_equal(sess._kept[name], other._kept[name])
    assert [None if s is None else s[1] for s in sess._sets] == [None if s is None else s[1] for s in other._sets]


def _same_selection(s, s0):
    assert np.array_equal(s.order, s0.order) and (s.n_kept, s.n_selected) == (s0.n_kept, s0.n_selected)
    assert np.array_equal(s.scores, s0.scores, equal_nan=True) and np.array_equal(s.cut_index, s0.cut_index)


def _same_scores(q, q0, rank=True):
    assert q.shape == q0.shape and np.array_equal(q.numpy(), q0.numpy(), equal_nan=True) and np.array_equal(q.cut_index, q0.cut_index)
    if rank:
        assert np.array_equal(q.rankings, q0.rankings)


def _forced(n_cols, seed=5, n=3, per=2):
    rng = np.random.default_rng(seed)
    per = min(per, n_cols)
    cols = np.concatenate([np.sort(rng.choice(n_cols, size=per, replace=False)) for _ in range(n)])
    return (np.stack([np.repeat(np.arange(n), per), cols]).astype(np.int32), rng.standard_normal(n * per).astype(np.float32), n)


def _pairs(models, rows_list, cls=LPSession, **kw):
    """(sessions, twins): one of each per entry of `rows_list`, member i on models[i % len(models)]."""
    sessions = [cls(models[i % len(models)], r, **kw) for i, r in enumerate(rows_list)]
    twins = [LPSession(models[i % len(models)], r, **kw) for i, r in enumerate(rows_list)]
    return sessions, twins


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_modes_on_the_row_seams(model, dev, n):  # noqa: F811
    """n sessions on R = 255 / 256 / 257 in the three modes: every result and every resident state equals the twin's."""
    cases = [S.case(S.ROW_CASES[i % 3]) for i in range(n)]
    rows, rounds = [c[0][1] for c in cases], [c[1][1] for c in cases]
    sessions, twins = _pairs([model], rows)
    group = LPSessionGroup(dev)
    forced = [_forced(s.n_cols, seed=i) if i % 2 == 0 else None for i, s in enumerate(sessions)]
    for got, twin, rnd in zip(group.score(sessions, rounds), twins, rounds):
        _same_scores(got, twin.score(rnd), rank=False)
    for got, twin, rnd in zip(group.score(sessions, rounds, rank="device"), twins, rounds):
        _same_scores(got, twin.score(rnd, rank="device"))
    got = group.select_cuts(sessions, rounds, forced, max_selected=7)
    for g, twin, rnd, f in zip(got, twins, rounds, forced):
        _same_selection(g, twin.select_cuts(rnd, f, max_selected=7))
    for s, t in zip(sessions, twins):
        _same_resident(s, t)
    assert group.calls == 3 and group.max_sessions_per_call == n
    # a ranking the host makes (the default below 1,024 cuts) goes through the solo call and comes back in place
    for got, twin, rnd in zip(group.score(sessions, rounds, rank=True), twins, rounds):
        _same_scores(got, twin.score(rnd, rank=True))


def test_mixed_shapes_models_and_kernels(model, model2, dev):  # noqa: F811
    """One call: `kinds`, a seam case, the 300-row hub (appended in the call), V = 33,000 whose append makes a segment long (its
    edge kernel differs from the others', so stages hold more than one kernel), two models, two sessions sharing one model."""
    kinds, hub, big = A.case("kinds"), A.case("hub300"), A.case("v33000")
    seam = S.case("rows256")
    rows = [kinds.rows, seam[0][1], hub.rows, big.rows, kinds.rows, seam[0][1]]
    models = [model, model2, model, model2, model2, model]
    sessions = [LPSession(m, r) for m, r in zip(models, rows)]
    twins = [LPSession(m, r) for m, r in zip(models, rows)]
    first = [kinds.before, seam[1][1], hub.before, big.before, kinds.before, seam[1][1]]
    group = LPSessionGroup(dev)
    for got, twin, rnd in zip(group.score(sessions, first, rank="device"), twins, first):
        _same_scores(got, twin.score(rnd, rank="device"))
    rounds = [kinds.before, seam[1][1], hub.rnd, big.rnd, kinds.rnd, seam[1][1]]
    appends = [None, None, hub.block, big.block, kinds.block, None]
    forced = [_forced(s.n_cols, seed=3 + i) for i, s in enumerate(sessions)]
    got = group.select_cuts(sessions, rounds, forced, max_selected=5, appends=appends)
    for g, twin, rnd, f, a in zip(got, twins, rounds, forced, appends):
        _same_selection(g, twin.select_cuts(rnd, f, max_selected=5, append=a))
    for s, t in zip(sessions, twins):
        _same_resident(s, t)
    # the definition itself: the selection on the assembled snapshot
    _same_selection(got[2], model.select_cuts_lp(hub.snap, forced[2], max_selected=5))
    _same_selection(got[3], model2.select_cuts_lp(big.snap, forced[3], max_selected=5))
    _same_selection(got[4], model2.select_cuts_lp(kinds.snap, forced[4], max_selected=5))
    assert not np.array_equal(got[0].scores, model2.select_cuts_lp(lpstate.assemble(kinds.rows, kinds.before), forced[0]).scores)
    assert group.max_sessions_per_call == 6


def test_mixed_appends_in_one_call(model, dev):  # noqa: F811
    """Members with and without an append; dL = 0, L0 = 0, dR = 1 / 256 / 257: results, resident state and fresh sessions."""
    names = ["kinds", "dl0", "l0_zero", "seam_256_1", "seam_256_256", "seam_256_257", "h0_zero"]
    cases = [A.case(n) for n in names]
    sessions, twins = _pairs([model], [c.rows for c in cases], GuardedSession)
    group = GuardedGroup(dev)
    before = [c.before for c in cases]
    for got, twin, rnd in zip(group.score(sessions, before), twins, before):
        _same_scores(got, twin.score(rnd), rank=False)
    appends = [None if n == "kinds" else c.block for n, c in zip(names, cases)]
    rounds = [c.before if a is None else c.rnd for c, a in zip(cases, appends)]
    got = group.select_cuts(sessions, rounds, max_selected=5, appends=appends)
    for g, twin, rnd, a, c in zip(got, twins, rounds, appends, cases):
        _same_selection(g, twin.select_cuts(rnd, max_selected=5, append=a))
        if a is not None:
            _same_selection(g, model.select_cuts_lp(c.snap, max_selected=5))
    for s, t, a, c in zip(sessions, twins, appends, cases):
        _same_resident(s, t)
        if a is not None:
            fresh = LPSession(model, lpstate.rows_with(c.rows, c.block))
            fresh.select_cuts(c.rnd)
            a_, b_ = s.resident_state(), fresh.resident_state()
            for name in ARRAYS + SCALARS:
                assert np.array_equal(a_[name], b_[name], equal_nan=True), name
        assert s.guards_intact()
    assert group.guards_intact()
    # the scores mode with appends (a second block behind the first) and the ranking mode without
    again = [None if a is None else c.block for a, c in zip(appends, cases)]
    rounds2 = []
    rng = np.random.default_rng(7)
    for s, c, a in zip(twins, cases, again):
        rows_now = lpstate.rows_with(c.rows, c.block) if a is not None else c.rows
        rows_next = lpstate.rows_with(rows_now, c.block) if a is not None else rows_now
        rounds2.append(A._round_for(rng, rows_next, c.snap))
    for g, twin, rnd, a in zip(group.score(sessions, rounds2, rank="device", appends=again), twins, rounds2, again):
        _same_scores(g, twin.score(rnd, rank="device", append=a))
    for s, t in zip(sessions, twins):
        _same_resident(s, t)
    assert group.guards_intact()


def test_lock_step_separation_loops(model, model2, dev):  # noqa: F811
    """Eight rounds over three sessions in lock step: each appends the cuts its last selection kept.  Every round equals the
    twins'; raw buffers and derived sets double on the way; the final states equal fresh sessions' on both ping-pong parities."""
    scripts = [A.loop_script(8, seed=171 + 10 * i) for i in range(3)]
    models = [model, model2, model]
    rows = [lpstate.LPRows.from_snapshot(sc[1]) for sc in scripts]
    sessions = [GuardedSession(m, r) for m, r in zip(models, rows)]
    twins = [LPSession(m, r) for m, r in zip(models, rows)]
    group = GuardedGroup(dev)
    forced = [_forced(64, seed=9 + i) for i in range(3)]
    full = [dict(col_lb=sc[1].col_lb, col_ub=sc[1].col_ub, col_primal=sc[1].col_primal, col_primal_avg=sc[1].col_primal_avg) for sc in scripts]
    blocks = [None] * 3
    raw_caps, set_caps, parities = [{s._cap} for s in sessions], [[set(), set()] for _ in sessions], [set() for _ in sessions]
    for r in range(8):
        if r == 4:
            blocks[1] = None            # one member skips an append: the parities of the sessions differ from here on
        rounds = []
        for i, (rng, base, pools) in enumerate(scripts):
            if blocks[i] is not None:
                rows[i] = lpstate.rows_with(rows[i], blocks[i])
            rounds.append(lpstate.LPRound(**A.S._solve(rng, rows[i], 64, col_lp=base.col_lp), **A.S._cuts_of(pools[r]),
                                          **(full[i] if r % 4 == 0 else {}), has_incumbent=True))
        got = group.select_cuts(sessions, rounds, forced, p_max=0.9, p_max_ub=0.95, max_selected=12, appends=blocks)
        for i, (g, twin) in enumerate(zip(got, twins)):
            _same_selection(g, twin.select_cuts(rounds[i], forced[i], p_max=0.9, p_max_ub=0.95, max_selected=12, append=blocks[i]))
            _same_selection(g, models[i].select_cuts_lp(lpstate.assemble(rows[i], rounds[i], full[i]), forced[i], p_max=0.9, p_max_ub=0.95,
                                                         max_selected=12))
            _same_resident(sessions[i], twin)
            s = sessions[i]
            raw_caps[i].add(s._cap)
            if s._cur_set >= 0:
                set_caps[i][s._cur_set].add(s._sets[s._cur_set][1])
                parities[i].add(s._cur_set)
            blocks[i] = A.cuts_as_rows(scripts[i][2][r], g.cut_index[g.order[:g.n_selected]])
            assert g.n_selected > 0
    assert any(len(c) >= 3 for c in raw_caps), raw_caps
    assert any(len(s) >= 2 for caps in set_caps for s in caps), set_caps
    assert {s._cur_set for s in sessions} == {0, 1} and all(p == {0, 1} for p in parities)
    for s, r in zip(sessions, rows):
        fresh = LPSession(s.model, r)
        a, b = s.resident_state(), fresh.resident_state()
        for name in ARRAYS + SCALARS:
            x, y = (a[name], b[name]) if name != "cons_feats" else (a[name][:, [0, 2]], b[name][:, [0, 2]])
            assert np.array_equal(x, y, equal_nan=True), name
        assert s.guards_intact()
    assert group.guards_intact()


def test_none_rules_behind_a_round_without_cuts(model, dev):  # noqa: F811
    """A round without cuts is a member of a batched call (it only refreshes the resident optional columns); a later member round
    without optional arrays reads what that one gave."""
    c, other = A.case("kinds"), S.case("rows257")
    sessions, twins = _pairs([model], [c.rows, other[0][1]])
    group = LPSessionGroup(dev)
    V = sessions[0].n_cols
    ub = np.where(np.arange(V) % 3 == 0, lpcases.INF, 2.0)
    none = dict(cut_ptr=np.zeros(1, np.int32), cut_col=np.zeros(0, np.int32), cut_val=np.zeros(0), cut_lhs=np.zeros(0), cut_rhs=np.zeros(0))
    empty = dataclasses.replace(c.before, col_ub=ub, **none)
    got = group.select_cuts(sessions, [empty, other[1][1]])
    for g, twin, rnd in zip(got, twins, [empty, other[1][1]]):
        _same_selection(g, twin.select_cuts(rnd))
    assert got[0].n_kept == 0 and got[0].scores.shape == (0,)
    bare = dataclasses.replace(c.before, col_lb=None, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    kept = dict(col_lb=c.before.col_lb, col_ub=ub, col_primal=c.before.col_primal, col_primal_avg=c.before.col_primal_avg)
    got = group.score([sessions[1], sessions[0]], [other[1][1], bare], rank="device")
    _same_scores(got[1], twins[0].score(bare, rank="device"))
    _same_scores(got[1], model.score_lp(lpstate.assemble(c.rows, bare, kept), rank="device"))
    _same_scores(got[0], twins[1].score(other[1][1], rank="device"))
    for s, t in zip(sessions, twins):
        _same_resident(s, t)


def test_rejection_is_per_member(model, dev):  # noqa: F811
    """deep=False, guards on the sessions and the group.  One member carries a cut column out of range, one an append block with
    unsorted columns, one a row_dual that is too short (refused on the host), one 4,097 cuts in selection mode: each gets its own
    exception in its own slot, every other member equals its twin, every rejected session equals a twin that never saw the call,
    and the same members go through in a later call once corrected."""
    c = A.case("kinds")
    names = ("bad_cut", "bad_block", "short_dual", "many_cuts", "good", "good_append")
    sessions, twins = _pairs([model], [c.rows] * len(names), GuardedSession, deep=False)
    group = GuardedGroup(dev)
    first = group.score(sessions, [c.before] * len(names), rank="device")
    want_first = twins[0].score(c.before, rank="device")
    for t in twins[1:]:
        t.score(c.before, rank="device")
    for q in first:
        _same_scores(q, want_first)
    V = sessions[0].n_cols
    ptr, col, val, lhs, rhs = c.block.arrays()
    unsorted = col.copy()
    unsorted[ptr[2]], unsorted[ptr[2] + 1] = col[ptr[2] + 1], col[ptr[2]]
    ub_bad = np.where(np.arange(V) % 2 == 0, lpcases.INF, 3.0)
    bad_round = dataclasses.replace(c.before, cut_col=np.where(np.arange(c.before.cut_col.size) == 3, V + 5, c.before.cut_col), col_ub=ub_bad,
                                    col_primal=np.asarray(c.before.col_primal) + 1.0)
    many = lpcases.snapshot("cuts4097")
    wide = dataclasses.replace(c.before, **{n: getattr(many, n) for n in ("cut_ptr", "cut_col", "cut_val", "cut_lhs", "cut_rhs")})
    rounds = [bad_round, c.rnd, c.before, wide, c.before, c.rnd]
    appends = [None, lpstate.LPRowBlock(ptr, unsorted, val, lhs, rhs), c.block, None, None, c.block]
    got = group.select_cuts(sessions, rounds, max_selected=5, appends=appends, return_exceptions=True)
    assert isinstance(got[0], ValueError) and "outside" in str(got[0])
    assert isinstance(got[1], ValueError) and "increasing" in str(got[1])
    assert isinstance(got[2], ValueError) and "row_dual" in str(got[2])
    assert isinstance(got[3], _lib.GcnnError) and "4097 cuts" in str(got[3])
    _same_selection(got[4], twins[4].select_cuts(c.before, max_selected=5))
    _same_selection(got[5], twins[5].select_cuts(c.rnd, max_selected=5, append=c.block))
    _same_resident(sessions[4], twins[4])
    _same_resident(sessions[5], twins[5])
    with pytest.raises(ValueError, match="outside"):
        group.select_cuts(sessions, rounds, max_selected=5, appends=appends[:5] + [None])      # (the first exception, after all were served)
    twins[4].select_cuts(c.before, max_selected=5)
    twins[5].select_cuts(c.rnd, max_selected=5)
    plain = dataclasses.replace(c.before, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    for i in range(4):
        s, t = sessions[i], twins[i]
        assert s.n_rows == t.n_rows == np.asarray(c.rows.row_lhs).shape[0]
        _same_scores(s.score(plain, rank="device"), t.score(plain, rank="device"))
        _same_resident(s, t, bookkeeping=False)       # (a rejected append has grown the raw buffers and made the other set)
        assert s.guards_intact()
    assert all(s.guards_intact() for s in sessions) and group.guards_intact()
    # corrected, the same members go through
    rounds = [c.before, c.rnd, c.rnd, c.before]
    appends = [None, c.block, c.block, None]
    got = group.select_cuts(sessions[:4], rounds, max_selected=5, appends=appends)
    for g, t, rnd, a in zip(got, twins, rounds, appends):
        _same_selection(g, t.select_cuts(rnd, max_selected=5, append=a))
    for s, t in zip(sessions[:4], twins):
        _same_resident(s, t, bookkeeping=False)
        assert s._cur_set == t._cur_set and s._stale == t._stale == set()
    assert all(s.guards_intact() for s in sessions) and group.guards_intact()
    with pytest.raises(ValueError, match="once per call"):
        group.score([sessions[0], sessions[0]], [c.before, c.before])


def test_launch_list_and_upload(model, dev):  # noqa: F811
    """Same-shaped members give the same launch list at n = 2 and n = 8, as long as a solo call's; with appends, as long as the
    solo fused call's; one upload of the layout's size; a solo call afterwards launches what it always did."""
    seam, c = S.case("rows256"), A.case("seam_257_257")
    sessions = [LPSession(model, seam[0][1]) for _ in range(8)]
    rnd = seam[1][1]
    group = LPSessionGroup(dev)
    group.select_cuts(sessions, [rnd] * 8)
    with _lib.launch_profile() as solo:
        want = sessions[0].select_cuts(rnd)
    solo_names = [n for n, _ in solo.launches]
    lists = {}
    for n in (2, 8):
        timings = {}
        group.select_cuts(sessions[:n], [rnd] * n, timings=timings)
        with _lib.launch_profile() as prof:
            got = group.select_cuts(sessions[:n], [rnd] * n, timings=timings)
        lists[n] = [name for name, _ in prof.launches]
        for g in got:
            _same_selection(g, want)
        assert timings["upload_bytes"] == sum(-(-s.upload_bytes(rnd, EMPTY_FORCED) // 256) * 256 for s in sessions[:n])
    assert lists[2] == lists[8] and len(lists[2]) == len(solo_names), (lists, solo_names)
    assert all(n.startswith(("k_group_", "k_lprs_")) for n in lists[2])
    assert lists[2][:2] == ["k_lprs_round_stats", "k_lprs_round_emit"] and lists[2][-2:] == ["k_lprs_sel_pairs", "k_lprs_sel_filter"]
    # some members append: the appends' four launches in front, then a round's launches
    mixed = [LPSession(model, c.rows) for _ in range(4)]
    group.score(mixed, [c.before] * 4)
    fused = LPSession(model, c.rows)
    fused.score(c.before)
    with _lib.launch_profile() as solo_fused:
        fused.select_cuts(c.rnd, append=c.block)
    timings = {}
    appends = [c.block, None, c.block, None]
    rounds = [c.rnd, c.before, c.rnd, c.before]
    predicted = sum(-(-s.upload_bytes(r, EMPTY_FORCED, append=a) // 256) * 256 for s, r, a in zip(mixed, rounds, appends))
    with _lib.launch_profile() as prof:
        group.select_cuts(mixed, rounds, appends=appends, timings=timings)
    names = [n for n, _ in prof.launches]
    assert len(names) == len(solo_fused.launches), (names, solo_fused.launches)
    assert names[:4] == ["k_lprs_append_stats", "k_lprs_append_scan", "k_lprs_append_move", "k_lprs_append_order"]
    assert names[4:6] == ["k_lprs_round_stats", "k_lprs_round_emit"] and all(n.startswith(("k_group_", "k_lprs_")) for n in names)
    assert timings["upload_bytes"] == predicted
    with _lib.launch_profile() as prof:                              # a solo call of a member session: unchanged
        sessions[1].select_cuts(rnd)
    assert [n for n, _ in prof.launches] == solo_names
    assert solo_names[:2] == ["k_lpr_stats", "k_lpr_emit"] and solo_names[-2:] == ["k_sel_pairs", "k_sel_filter"]


def test_model_set_forwards_to_its_group(model, model2):
    """`ModelSet.score_rounds` / `select_cuts_rounds`: the keys name the sessions' models; one group serves both models' sessions."""
    from gcnn_cut_selector_amd.model import ModelSet
    mset = ModelSet({"a": model, "b": model2})
    seam = S.case("rows255")
    rows, rnd = seam[0][1], seam[1][1]
    sessions, twins = [model.open_lp(rows), model2.open_lp(rows)], [model.open_lp(rows), model2.open_lp(rows)]
    for g, t in zip(mset.select_cuts_rounds(["a", "b"], sessions, [rnd] * 2, max_selected=4), twins):
        _same_selection(g, t.select_cuts(rnd, max_selected=4))
    for g, t in zip(mset.score_rounds(["a", "b"], sessions, [rnd] * 2, rank="device"), twins):
        _same_scores(g, t.score(rnd, rank="device"))
    assert mset._lp_rounds.calls == 2 and mset._lp_rounds.max_sessions_per_call == 2
    with pytest.raises(ValueError, match="not opened"):
        mset.score_rounds(["b", "a"], sessions, [rnd] * 2)
    with pytest.raises(KeyError):
        mset.score_rounds(["a", "z"], sessions, [rnd] * 2)


def test_a_member_the_call_refuses_is_isolated(model, dev):  # noqa: F811
    """A call the library declines (None) or refuses (GcnnError) as a whole is halved until the member it is about stands alone:
    that one is answered by its own call, the others still share batched calls, and the counters say so."""
    seam = S.case("rows256")
    rows, rnd = seam[0][1], seam[1][1]
    sessions, twins = _pairs([model], [rows] * 5)

    class Picky(LPSessionGroup):
        refuse = None

        def _call(self, members, jobs, *args, **kw):
            if any(m is sessions[3] for m in members):
                if self.refuse == "raise":
                    raise _lib.GcnnError("gcnn_lp_rounds failed: bad argument")
                return None
            return super()._call(members, jobs, *args, **kw)

    for refuse in (None, "raise"):
        group = Picky(dev)
        group.refuse = refuse
        got = group.select_cuts(sessions, [rnd] * 5, max_selected=6, return_exceptions=True)
        for g, t in zip(got, twins):
            _same_selection(g, t.select_cuts(rnd, max_selected=6))
        # 5 -> (2, 3) -> 3 -> (1, 2) -> 2 -> (1, 1): members 0-1, then member 2, then member 4 batched; member 3 alone
        assert (group.calls, group.max_sessions_per_call, group.solo_rounds) == (3, 2, 1)
    for s, t in zip(sessions, twins):
        _same_resident(s, t)
