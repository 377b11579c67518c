"""Rounds of several resident LPs in one call where members remove rows (`infer.LPSessionGroup(batch_removes=True)`,
gcnn_lp_rounds_edit; csrc/k_lpedits.hpp) on the GPU.  The oracle of every member is a twin `LPSession` that gets the same sequence
through solo calls, plus the snapshot call on `assemble(rows_without(rows_with(...)))`: results, the resident state and the host's
bookkeeping are compared with `np.array_equal`.  The feature computes no floating-point value: no tolerance anywhere."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lpappendcases as A  # noqa: E402
import lpcases  # noqa: E402
import lpremovecases as D  # noqa: E402
import lpsessioncases as S  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate  # noqa: E402
from gcnn_cut_selector_amd.infer import LPSession, LPSessionGroup  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

SCALARS = ("l_max_deg", "v_max_deg", "n_rows", "n_state_rows", "n_state_edges")
ARRAYS = ("cons_feats", "row_place", "row_scale", "l_ptr", "edge_row", "edge_col", "edge_coef", "v_ptr", "v_oth", "v_coef")
EMPTY_FORCED = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
REMOVE_TWINS = ["k_lpes_mark", "k_lpes_rows", "k_lpes_vars"]
APPEND_TWINS = ["k_lprs_append_stats", "k_lprs_append_scan", "k_lprs_append_move", "k_lprs_append_order"]
SCORES, RANK, SELECT = "scores", "rank", "select"


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


def _same_resident(sess, other):
    """The resident state and everything the host keeps beside it: the sizes, the sets and their capacities, both raw sets, the
    transit set, the book, the kept and stale optional arrays, the longest segments."""
    a, b = sess.resident_state(), other.resident_state()
    for name in SCALARS:
        assert a[name] == b[name], name
    for name in ARRAYS:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name], equal_nan=True), name
    assert (sess.n_rows, sess._lhs, sess._max_deg, sess._cap, sess._cap_alt) == (other.n_rows, other._lhs, other._max_deg, other._cap, other._cap_alt)
    assert np.array_equal(sess._col_deg, other._col_deg)
    for x, y in zip(sess._book, other._book):
        assert np.array_equal(x, y)
    assert sess._cur_set == other._cur_set and sess._stale == other._stale and sorted(sess._kept) == sorted(other._kept)
    for name in sess._kept:
        assert np.array_equal(sess._kept[name], other._kept[name])
    caps = lambda slots: [None if s is None else s[1] for s in slots]  # noqa: E731
    assert caps(sess._sets) == caps(other._sets) and caps(sess._transit) == caps(other._transit)
    assert (sess._raw_alt is None) == (other._raw_alt is None)
    # the raw rows the session holds now (what the next removal reads)
    d = sess._dims
    used = (4 * (d["n_rows"] + 1), 4 * d["row_nnz"], 8 * d["row_nnz"], 8 * d["n_rows"], 8 * d["n_rows"])
    for x, y, n in zip(sess._raw, other._raw, used):
        assert np.array_equal(x[:n].cpu().numpy(), y[:n].cpu().numpy())


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


@dataclasses.dataclass
class Member:
    """One member of a call: the rows resident before, a round on them, the call's round, block and removed indices, and the
    snapshot the call's round stands for."""
    rows: object
    before: object
    rnd: object
    block: object = None
    idx: object = None
    snap: object = None


def plain(name="kinds"):
    c = A.case(name)
    return Member(c.rows, c.before, c.before, snap=lpstate.assemble(c.rows, c.before))


def appending(name="kinds"):
    c = A.case(name)
    return Member(c.rows, c.before, c.rnd, c.block, None, c.snap)


def removing(name="kinds"):
    c = D.case(name)
    return Member(c.rows, c.before, c.rnd, None, c.idx, c.snap)


def both(name="kinds", idx=(2, 44, 9, 49, 40), seed=31):
    """An append case with a removal on top; indices at or past the resident rows point into the member's own block."""
    c = A.case(name)
    after = lpstate.rows_without(lpstate.rows_with(c.rows, c.block), idx)
    rnd = A._round_for(np.random.default_rng(seed), after, c.snap)
    return Member(c.rows, c.before, rnd, c.block, np.asarray(idx), lpstate.assemble(after, rnd))


KINDS = (plain, appending, removing, both)


def _open(models, members, cls=LPSession, **kw):
    """(sessions, twins) of the members, each past one accepted round on its rows."""
    sessions = [cls(models[i % len(models)], m.rows, **kw) for i, m in enumerate(members)]
    twins = [LPSession(models[i % len(models)], m.rows, **kw) for i, m in enumerate(members)]
    for s, t, m in zip(sessions, twins, members):
        s.score(m.before)
        t.score(m.before)
    return sessions, twins


def _serve(group, mode, sessions, members, forced=None, **kw):
    rounds, appends, removes = [m.rnd for m in members], [m.block for m in members], [m.idx for m in members]
    if mode == SELECT:
        return group.select_cuts(sessions, rounds, forced, max_selected=5, appends=appends, removes=removes, **kw)
    return group.score(sessions, rounds, rank="device" if mode == RANK else False, appends=appends, removes=removes, **kw)


def _solo(mode, t, m, f=None):
    if mode == SELECT:
        return t.select_cuts(m.rnd, f, max_selected=5, append=m.block, remove=m.idx)
    return t.score(m.rnd, rank="device" if mode == RANK else False, append=m.block, remove=m.idx)


def _snapshot_call(mode, model, m, f=None):  # noqa: F811
    if mode == SELECT:
        return model.select_cuts_lp(m.snap, f, max_selected=5)
    return model.score_lp(m.snap, rank="device" if mode == RANK else False)


def _check(mode, got, want):
    if mode == SELECT:
        _same_selection(got, want)
    else:
        _same_scores(got, want, rank=mode == RANK)


def _one_call(models, dev, members, mode, group=None, cls=LPSession):  # noqa: F811
    """The members through one grouped call against their twins' solo calls and the snapshot call; returns (group, sessions, twins)."""
    sessions, twins = _open(models, members, cls)
    group = group or LPSessionGroup(dev, batch_removes=True)
    forced = [_forced(s.n_cols, seed=3 + i) if mode == SELECT and i % 2 == 0 else None for i, s in enumerate(sessions)]
    calls = group.calls
    got = _serve(group, mode, sessions, members, forced)
    assert group.calls == calls + -(-len(members) // group.MAX) and group.solo_rounds == 0
    for i, (g, s, t, m, f) in enumerate(zip(got, sessions, twins, members, forced)):
        _check(mode, g, _solo(mode, t, m, f))
        if m.snap is not None:
            _check(mode, g, _snapshot_call(mode, models[i % len(models)], m, f))
        _same_resident(s, t)
    return group, sessions, twins


@pytest.mark.parametrize("mode", [SCORES, RANK, SELECT])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_modes_with_mixed_edits(model, model2, dev, n, mode):  # noqa: F811
    """n members that mix plain, append, removal and both in one call, in the three modes (selection with forced rows on every
    other member), on two models; n = 1 is the member with both edits."""
    members = [KINDS[(i + 3) % 4]() for i in range(n)]
    group, sessions, _ = _one_call([model, model2], dev, members, mode)
    assert group.max_sessions_per_call == n and group.calls == 1
    # a second call on the edited sessions: plain rounds, which go out through gcnn_lp_rounds as before
    rounds = [m.rnd for m in members]
    for g, m, mdl in zip(group.score(sessions, rounds), members, [model, model2] * 4):
        _same_scores(g, mdl.score_lp(m.snap), rank=False)
    assert group.calls == 2 and group.solo_rounds == 0


CHUNKS = [D.CASES[i:i + 8] for i in range(0, len(D.CASES), 8)]


@pytest.mark.parametrize("names", CHUNKS, ids=[c[0] for c in CHUNKS])
def test_removal_seams_beside_other_shapes(model, dev, names):  # noqa: F811
    """Every case of `lpremovecases` as one member of a call beside members of other shapes: R0 = 255 / 256 / 257 / 513 with row
    0, the last row, rows 255 + 256, a whole first chunk and every other row; lists of 1 / 255 / 256 / 257 rows; only free rows;
    one row left; L = 0; emptied variable segments; the 300-row hub; V = 1 / 257 / past a trip over the chunk counters / 33,000."""
    members = [removing(n) for n in names]
    _, sessions, _ = _one_call([model], dev, members, SELECT, cls=GuardedSession)
    for s, m in zip(sessions, members):
        fresh = LPSession(model, lpstate.rows_without(m.rows, m.idx))
        a, b = s.resident_state(), fresh.resident_state()
        for name in ARRAYS + SCALARS:
            x, y = (a[name], b[name]) if name != "cons_feats" else (a[name][:, [0, 2]], b[name][:, [0, 2]])
            assert np.array_equal(x, y, equal_nan=True), name
        assert s.guards_intact()
        fresh.close()


def test_segment_that_stops_being_long_inside_the_grouped_call(model, dev):  # noqa: F811
    """V = 33,000 beside a small member: the last column falls from 33 to 32 entries through the grouped removal, so the next
    round's launch list must be the fresh session's (no long-segment blocks), with its bits."""
    big, small = removing("v33000"), removing("kinds")
    _, sessions, _ = _one_call([model], dev, [small, big], RANK)
    sess, fresh = sessions[1], LPSession(model, lpstate.rows_without(big.rows, big.idx))
    assert sess.resident_state()["v_max_deg"] == 32 == fresh.resident_state()["v_max_deg"]
    lists = []
    for s in (sess, fresh):
        s.score(big.rnd)
        with _lib.launch_profile() as prof:
            q = s.score(big.rnd, rank=True)
        lists.append(([n for n, _ in prof.launches], q))
    assert lists[0][0] == lists[1][0]
    _same_scores(lists[0][1], lists[1][1])


FUSED = {"resident_only": ("kinds", [3, 17, 22]), "block_only": ("kinds", [41, 45]), "both": ("kinds", [2, 44, 9, 49, 40]),
         "block_loses_all": ("kinds", [5] + list(range(40, 50))), "seam": ("seam_256_257", [0, 255, 256, 300, 400, 511, 512]),
         "every_resident_row": ("kinds", list(range(40)) + [47])}


def test_removal_and_append_with_indices_into_the_own_block(model, model2, dev):  # noqa: F811
    """Indices only in the resident rows, only in the block (no removal reaches the device), in both, a block that loses all its
    rows, an edit across the chunk seam, and every resident row removed with only rows of the block left: one call."""
    members = [both(case, idx, seed=40 + i) for i, (case, idx) in enumerate(FUSED.values())]
    group, sessions, _ = _one_call([model, model2], dev, members, SELECT, cls=GuardedSession)
    assert group.max_sessions_per_call == len(members)
    assert sessions[1]._transit == [None] and sessions[1]._raw_alt is None       # block_only: the plain fused member
    assert all(s.guards_intact() for s in sessions)


def test_lock_step_loops_that_append_and_clean_up(model, model2, dev):  # noqa: F811
    """Eight rounds over three sessions in lock step: each appends the cuts its last selection kept and removes three earlier cut
    rows (just-appended ones among them) in the same grouped call.  Every round equals the twins' and the snapshot call; the raw
    sets and the derived sets grow on the way, both parities are visited, and the transit set is allocated mid-loop."""
    scripts = [A.loop_script(8, seed=171 + 10 * i) for i in range(3)]
    models = [model, model2, model]
    rows = [lpstate.LPRows.from_snapshot(sc[1]) for sc in scripts]
    n_base = [np.asarray(r.row_lhs).shape[0] for r in rows]
    sessions = [GuardedSession(m, r) for m, r in zip(models, rows)]
    twins = [LPSession(m, r) for m, r in zip(models, rows)]
    group = GuardedGroup(dev, batch_removes=True)
    pick = np.random.default_rng(181)
    forced = [_forced(64, seed=9 + i) for i in range(3)]
    full = [dict(col_lb=sc[1].col_lb, col_ub=sc[1].col_ub, col_primal=sc[1].col_primal, col_primal_avg=sc[1].col_primal_avg) for sc in scripts]
    blocks = [None] * 3
    raw_caps, alt_caps = [{s._cap} for s in sessions], [set() for _ in sessions]
    parities, transit_at, removals = [set() for _ in sessions], [None] * 3, 0
    for r in range(8):
        rounds, removes = [], [None] * 3
        for i, (rng, base, pools) in enumerate(scripts):
            if blocks[i] is not None:
                rows[i] = lpstate.rows_with(rows[i], blocks[i])
                n = np.asarray(rows[i].row_lhs).shape[0]
                if n - n_base[i] >= 6 and not (i == 1 and r == 4):      # (one member skips a clean-up: a fused append beside removals)
                    removes[i] = n_base[i] + pick.choice(n - n_base[i], size=3, replace=False)
                    rows[i] = lpstate.rows_without(rows[i], removes[i])
                    removals += 1
            rounds.append(lpstate.LPRound(**A.S._solve(rng, rows[i], 64, col_lp=base.col_lp), **A.S._cuts_of(pools[r]),
                                          **(full[i] if r % 4 == 0 else {}), has_incumbent=True))
        got = group.select_cuts(sessions, rounds, forced, p_max=0.9, p_max_ub=0.95, max_selected=12, appends=blocks, removes=removes)
        for i, (g, twin) in enumerate(zip(got, twins)):
            _same_selection(g, twin.select_cuts(rounds[i], forced[i], p_max=0.9, p_max_ub=0.95, max_selected=12, append=blocks[i],
                                                remove=removes[i]))
            _same_selection(g, models[i].select_cuts_lp(lpstate.assemble(rows[i], rounds[i], full[i]), forced[i], p_max=0.9, p_max_ub=0.95,
                                                         max_selected=12))
            s = sessions[i]
            _same_resident(s, twin)
            assert s.n_rows == np.asarray(rows[i].row_lhs).shape[0]
            raw_caps[i].add(s._cap)
            alt_caps[i].add(s._cap_alt)
            if s._cur_set >= 0:
                parities[i].add(s._cur_set)
            if s._transit[0] is not None and transit_at[i] is None:
                transit_at[i] = r
            blocks[i] = A.cuts_as_rows(scripts[i][2][r], g.cut_index[g.order[:g.n_selected]])
            assert g.n_selected > 0
    assert group.solo_rounds == 0 and group.calls == 8 and group.max_sessions_per_call == 3
    assert removals >= 15 and all(p == {0, 1} for p in parities)
    assert all(t is not None and t >= 1 for t in transit_at), transit_at             # allocated by the first call with both edits
    assert all(len(c) >= 2 for c in raw_caps) and all(len(c) >= 2 for c in alt_caps), (raw_caps, alt_caps)     # both raw sets grew
    for s, r in zip(sessions, rows):
        fresh = LPSession(s.model, r)
        a, b = s.resident_state(), fresh.resident_state()
        for name in ARRAYS + SCALARS:
            x, y = (a[name], b[name]) if name != "cons_feats" else (a[name][:, [0, 2]], b[name][:, [0, 2]])
            assert np.array_equal(x, y, equal_nan=True), name
        assert s.guards_intact()
    assert group.guards_intact()


def test_none_rules_behind_a_zero_cut_member_with_a_removal(model, dev):  # noqa: F811
    """A round without cuts that removes rows is a member of the grouped call (its removal rides in the edit phase, its round's
    solo launches run behind the group's); a later member round without optional arrays reads what that one gave."""
    c, other = D.case("kinds"), removing("seam_257_seam")
    after = lpstate.rows_without(c.rows, c.idx)
    V = 64
    ub = np.where(np.arange(V) % 3 == 0, lpcases.INF, 2.0)
    none = dict(cut_ptr=np.zeros(1, np.int32), cut_col=np.zeros(0, np.int32), cut_val=np.zeros(0), cut_lhs=np.zeros(0), cut_rhs=np.zeros(0))
    empty = dataclasses.replace(c.rnd, col_ub=ub, **none)
    members = [Member(c.rows, c.before, empty, None, c.idx), other]
    group, sessions, twins = _one_call([model], dev, members, SELECT)
    assert sessions[0].n_rows == np.asarray(after.row_lhs).shape[0]
    bare = dataclasses.replace(c.rnd, col_lb=None, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    kept = dict(col_lb=c.rnd.col_lb, col_ub=ub, col_primal=c.rnd.col_primal, col_primal_avg=c.rnd.col_primal_avg)
    got = group.score(sessions, [bare, other.rnd], rank="device")
    _same_scores(got[0], twins[0].score(bare, rank="device"))
    _same_scores(got[0], model.score_lp(lpstate.assemble(after, bare, kept), rank="device"))
    for s, t in zip(sessions, twins):
        _same_resident(s, t)


class Miscounting(GuardedSession):
    """A session whose host account of a removal is off by one raw entry: the device's totals disagree and it flags the edit
    (every store of the removal is bounds-checked against the host's sizes, so the smaller count writes nothing out of place)."""

    def _removal_host(self, idx, append):
        e = super()._removal_host(idx, append)
        six = list(e.removed)
        six[1] += 1
        e.removed = tuple(six)
        assert e.mid["row_nnz"] >= 1
        e.mid = dict(e.mid, row_nnz=e.mid["row_nnz"] - 1)
        e.final = dict(e.final, row_nnz=e.final["row_nnz"] - 1)
        return e


def test_rejection_is_per_member_and_leaves_its_session_as_it_was(model, dev):  # noqa: F811
    """Guards on the sessions and the group.  One member's indices the host rejects (it stays out of the call), one member's
    removal the device flags because its totals disagree with the host's (it raises in its slot only and holds the rows it
    held): the others' results and resident states are their twins', and every guard byte is intact."""
    members = [removing("kinds"), removing("seam_513_n256"), both(), appending("kinds"), removing("var_edges")]
    sessions, twins = _open([model], members, GuardedSession)
    sessions[1].close()
    sessions[1] = Miscounting(model, members[1].rows)
    sessions[1].score(members[1].before)
    untouched = [LPSession(model, members[i].rows) for i in (0, 1)]
    for u, i in zip(untouched, (0, 1)):
        u.score(members[i].before)
    group = GuardedGroup(dev, batch_removes=True)
    rounds, appends = [m.rnd for m in members], [m.block for m in members]
    removes = [m.idx for m in members]
    removes[0] = [5, 6, 5]
    got = group.select_cuts(sessions, rounds, max_selected=5, appends=appends, removes=removes, return_exceptions=True)
    assert isinstance(got[0], ValueError) and "twice" in str(got[0])
    assert isinstance(got[1], ValueError) and "rejected by the device" in str(got[1])
    assert group.calls == 1 and group.max_sessions_per_call == 4 and group.solo_rounds == 0
    for i in (2, 3, 4):
        _same_selection(got[i], twins[i].select_cuts(rounds[i], max_selected=5, append=appends[i], remove=removes[i]))
        _same_selection(got[i], model.select_cuts_lp(members[i].snap, max_selected=5))
        _same_resident(sessions[i], twins[i])
    for i, u in zip((0, 1), untouched):
        s = sessions[i]
        assert s.n_rows == u.n_rows == np.asarray(members[i].rows.row_lhs).shape[0]
        a, b = s.resident_state(), u.resident_state()
        for name in ARRAYS + SCALARS:
            assert np.array_equal(a[name], b[name], equal_nan=True), name
        _same_scores(s.score(members[i].before, rank="device"), u.score(members[i].before, rank="device"))
    assert all(s.guards_intact() for s in sessions) and group.guards_intact()
    # corrected, member 0 goes through in a later call
    g = group.select_cuts(sessions[:1], rounds[:1], max_selected=5, removes=[members[0].idx])[0]
    _same_selection(g, twins[0].select_cuts(rounds[0], max_selected=5, remove=members[0].idx))
    _same_resident(sessions[0], twins[0])
    assert all(s.guards_intact() for s in sessions) and group.guards_intact()


def test_launch_list_upload_and_counters(model, dev):  # noqa: F811
    """Same-shaped members that append and remove: 3 + 4 + the plain round's launches whatever n, under the twins' names, behind
    one fill region; the upload is the sum of the solo uploads rounded up to 256 each; nothing goes solo."""
    m = both("seam_257_257", [0, 255, 256, 300, 513], seed=35)
    after = lpstate.rows_without(lpstate.rows_with(m.rows, m.block), m.idx)
    fresh = LPSession(model, after)
    fresh.score(m.rnd)
    with _lib.launch_profile() as prof:
        fresh.select_cuts(m.rnd)
    n_plain = len(prof.launches)
    lists = {}
    for n in (1, 2, 8):
        sessions, twins = _open([model], [m] * n)
        group = LPSessionGroup(dev, batch_removes=True)
        predicted = sum(-(-s.upload_bytes(m.rnd, EMPTY_FORCED, append=m.block, remove=m.idx) // 256) * 256 for s in sessions)
        solo = sum(s.upload_bytes(m.rnd, EMPTY_FORCED, append=m.block, remove=m.idx) for s in sessions)
        timings = {}
        with _lib.launch_profile() as prof:
            got = group.select_cuts(sessions, [m.rnd] * n, appends=[m.block] * n, removes=[m.idx] * n, timings=timings)
        lists[n] = [name for name, _ in prof.launches]
        assert solo <= timings["upload_bytes"] == predicted <= solo + 255 * n
        assert (group.calls, group.max_sessions_per_call, group.solo_rounds) == (1, n, 0)
        for g in got:
            _same_selection(g, model.select_cuts_lp(m.snap))
        (L, _, _), = group.layouts.values()
        assert isinstance(L, _lib.LpRoundsEditLayout)
        offs = sorted([L.remove_counts_off[i] for i in range(n)] + [L.counts_off[i] for i in range(n)])
        assert offs[0] == L.counts_base and offs[-1] < L.counts_base + L.counts_bytes <= L.out_base      # one region: one fill
    assert lists[1] == lists[2] == lists[8], lists
    names = lists[8]
    assert n_plain == 11 and len(names) == 3 + 4 + 11, names
    assert names[:3] == REMOVE_TWINS and names[3:7] == APPEND_TWINS and names[7:9] == ["k_lprs_round_stats", "k_lprs_round_emit"]
    assert all(x.startswith(("k_group_", "k_lprs_", "k_lpes_")) for x in names)
    # removal only: 3 + 11; and a chunk without a removal still goes out through gcnn_lp_rounds
    r = removing("seam_513_n257")
    sessions, _ = _open([model], [r] * 2)
    group = LPSessionGroup(dev, batch_removes=True)
    with _lib.launch_profile() as prof:
        group.select_cuts(sessions, [r.rnd] * 2, removes=[r.idx] * 2)
    names = [name for name, _ in prof.launches]
    assert len(names) == 3 + 11 and names[:3] == REMOVE_TWINS and names[3] == "k_lprs_round_stats"
    with _lib.launch_profile() as prof:
        group.select_cuts(sessions, [r.rnd] * 2)
    assert len(prof.launches) == 11 and isinstance(list(group.layouts.values())[-1][0], _lib.LpRoundsLayout)


def test_batch_removes_off_gives_the_same_answers(model, dev):  # noqa: F811
    """The default group on the same input: the removing members go solo (counted), the answers and resident states are the same."""
    members = [KINDS[i % 4]() for i in range(5)]
    on, s_on, _ = _one_call([model], dev, members, SELECT)
    sessions, _ = _open([model], members)
    off = LPSessionGroup(dev)
    forced = [_forced(s.n_cols, seed=3 + i) if i % 2 == 0 else None for i, s in enumerate(sessions)]
    got = _serve(off, SELECT, sessions, members, forced)
    assert off.solo_rounds == 2 and on.solo_rounds == 0
    for g, m, f, a, b in zip(got, members, forced, sessions, s_on):
        _same_selection(g, model.select_cuts_lp(m.snap, f, max_selected=5))
        _same_resident(a, b)


def test_model_set_forwards_removes(model, model2):
    """`ModelSet.select_cuts_rounds` / `score_rounds` with `removes=` and `batch_removes=`."""
    from gcnn_cut_selector_amd.model import ModelSet
    mset = ModelSet({"a": model, "b": model2})
    members = [removing("kinds"), both()]
    for batch, solo in ((True, 0), (False, 2)):
        sessions, twins = _open([model, model2], members)
        got = mset.select_cuts_rounds(["a", "b"], sessions, [m.rnd for m in members], max_selected=4, appends=[m.block for m in members],
                                      removes=[m.idx for m in members], batch_removes=batch)
        for g, t, m in zip(got, twins, members):
            _same_selection(g, t.select_cuts(m.rnd, max_selected=4, append=m.block, remove=m.idx))
        assert mset._lp_rounds.solo_rounds == solo
    sessions, twins = _open([model, model2], members)
    got = mset.score_rounds(["a", "b"], sessions, [m.rnd for m in members], rank="device", appends=[m.block for m in members],
                            removes=[m.idx for m in members], batch_removes=True)
    for g, t, m in zip(got, twins, members):
        _same_scores(g, t.score(m.rnd, rank="device", append=m.block, remove=m.idx))
    assert mset._lp_rounds.solo_rounds == 2
