"""The removal of rows from a resident LP (`LPSession.remove_rows`, the `remove=` of a round; csrc/k_lpremove.hpp) on the GPU.  Every
check is made against two independent answers with `np.array_equal` -- the full-snapshot call on the assembled snapshot of
`lpstate.rows_without(rows_with(rows, block), idx)`, and a FRESH session opened on those rows, whose resident state (static
constraint features, row places and scales, the six graph arrays, the longest segments) the edited session's must equal bit for
bit.  No tolerance anywhere."""
import dataclasses

import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

import lpappendcases as A  # noqa: E402
import lpcases  # noqa: E402
import lpremovecases as D  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate  # noqa: E402
from gcnn_cut_selector_amd.infer import LPSession, LPSessionGroup  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

NAMES = ["k_lpd_mark", "k_lpd_rows", "k_lpd_vars"]
APPEND_NAMES = ["k_lpa_stats", "k_lpa_scan", "k_lpa_move", "k_lpa_order"]
RESIDENT = ("row_place", "row_scale", "l_ptr", "edge_row", "edge_col", "edge_coef", "v_ptr", "v_oth", "v_coef", "l_max_deg", "v_max_deg",
            "n_rows", "n_state_rows", "n_state_edges")
NO_FORCED = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))


@pytest.fixture(scope="module")
def model(dev):  # noqa: F811
    return make_model(93, dev)[0]


class GuardedSession(LPSession):
    GUARD = 256


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _same_resident(sess, other):
    a, b = sess.resident_state(), other.resident_state()
    for name in RESIDENT:
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert np.array_equal(a["cons_feats"][:, [0, 2]], b["cons_feats"][:, [0, 2]], equal_nan=True)
    assert sess._lhs == other._lhs and sess._max_deg == other._max_deg and np.array_equal(sess._col_deg, other._col_deg)
    for x, y in zip(sess._book, other._book):
        assert np.array_equal(x, y)


def _same_selection(s, s0):
    assert np.array_equal(s.order, s0.order) and (s.n_kept, s.n_selected) == (s0.n_kept, s0.n_selected)
    assert np.array_equal(s.scores, s0.scores, equal_nan=True) and np.array_equal(s.cut_index, s0.cut_index)


def _same_scores(q, q0):
    assert q.shape == q0.shape and np.array_equal(q.numpy(), q0.numpy(), equal_nan=True)
    assert np.array_equal(q.rankings, q0.rankings) and np.array_equal(q.cut_index, q0.cut_index)


def _forced(n_cols, seed=5, n=3, per=2):
    rng = np.random.default_rng(seed)
    per = min(per, n_cols)
    cols = np.concatenate([np.sort(rng.choice(n_cols, size=per, replace=False)) for _ in range(n)])
    return (np.stack([np.repeat(np.arange(n), per), cols]).astype(np.int32), rng.standard_normal(n * per).astype(np.float32), n)


def _four_ways(model, rows, before, rnd, snap, after, block=None, idx=None):
    """The fused selection with forced rows, the fused state, the fused score and the edit alone: each against the snapshot call
    and a fresh session, on the results and on the resident state."""
    fresh = LPSession(model, after)
    forced = _forced(fresh.n_cols)
    want_sel = model.select_cuts_lp(snap, forced, max_selected=5)
    want_state, want_index = model.state_from_lp(snap)
    want_q = model.score_lp(snap, rank=True)
    fresh_sel = fresh.select_cuts(rnd, forced, max_selected=5)
    _same_selection(fresh_sel, want_sel)
    sess = GuardedSession(model, rows)
    sess.score(before)
    got = sess.select_cuts(rnd, forced, max_selected=5, append=block, remove=idx)
    _same_selection(got, want_sel)
    _same_selection(got, fresh_sel)
    assert sess.n_rows == fresh.n_rows
    _same_resident(sess, fresh)
    state, index = sess.state(rnd)
    assert _same(state, want_state) and np.array_equal(index, want_index)
    assert sess.guards_intact()
    sess.close()
    for call in ("state", "score"):
        sess = LPSession(model, rows)
        if call == "state":
            state, index = sess.state(rnd, append=block, remove=idx)
            assert _same(state, want_state) and np.array_equal(index, want_index)
        else:
            _same_scores(sess.score(rnd, rank=True, append=block, remove=idx), want_q)
        _same_resident(sess, fresh)
        sess.close()
    # the edit alone: the append, then the removal
    sess = GuardedSession(model, rows)
    if block is not None:
        sess.append_rows(*block.arrays(), incremental=True)
    sess.remove_rows(idx)
    assert sess.n_rows == fresh.n_rows
    _same_resident(sess, fresh)
    _same_scores(sess.score(rnd, rank=True), want_q)
    _same_scores(sess.score(rnd, rank=True), fresh.score(rnd, rank=True))
    assert sess.guards_intact()
    sess.close()
    fresh.close()


@pytest.mark.parametrize("name", D.CASES)
def test_remove_cases(model, name):
    """Kinds of removed row, only free rows removed, the side extremes (L = 0, no rhs side, only free rows left, one row left),
    the chunk seams and list sizes, the variables' segments (emptied, first / last / only entry, variable 0 and V - 1, V = 1 / 257 /
    past a trip over the chunk counters, a hub column) and V = 33,000."""
    c = D.case(name)
    _four_ways(model, c.rows, c.before, c.rnd, c.snap, lpstate.rows_without(c.rows, c.idx), idx=c.idx)


def test_segment_that_stops_being_long_through_the_removal(model):
    """V = 33,000: the last column falls from 33 to 32 entries only through the removal, so the by-variable edge pass drops its
    long-segment blocks -- the host's longest segments, the launch list and the bits equal the fresh session's."""
    c = D.case("v33000")
    fresh = LPSession(model, lpstate.rows_without(c.rows, c.idx))
    sess = LPSession(model, c.rows)
    before = sess.resident_state()["v_max_deg"]
    sess.remove_rows(c.idx)
    now = sess.resident_state()
    assert before == 33 and now["v_max_deg"] == 32 == fresh.resident_state()["v_max_deg"] and now["l_max_deg"] == fresh.resident_state()["l_max_deg"]
    lists = []
    for s in (sess, fresh):
        s.score(c.rnd)
        with _lib.launch_profile() as prof:
            q = s.score(c.rnd, rank=True)
        lists.append(([n for n, _ in prof.launches], q))
    assert lists[0][0] == lists[1][0]
    _same_scores(lists[0][1], lists[1][1])
    _same_scores(lists[0][1], model.score_lp(c.snap, rank=True))


def _fused_case(name, idx, seed):
    """An append case with a removal on top: (rows, block, idx, the round after the edit, its snapshot, a round before, the rows after)."""
    c = A.case(name)
    after = lpstate.rows_without(lpstate.rows_with(c.rows, c.block), idx)
    rnd = A._round_for(np.random.default_rng(seed), after, c.snap)
    return c.rows, c.block, np.asarray(idx), rnd, lpstate.assemble(after, rnd), c.before, after


FUSED = {"resident_only": ("kinds", [3, 17, 22]), "block_only": ("kinds", [41, 45]), "both": ("kinds", [2, 44, 9, 49, 40]),
         "block_loses_all": ("kinds", [5] + list(range(40, 50))), "dl0_lhs_removed": ("dl0", None), "seam": ("seam_256_257", None),
         "every_resident_row": ("kinds", list(range(40)) + [47])}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_append_and_removal_in_one_call(model, name):
    """Indices only in the resident rows, only in the block, in both, a block that loses all its rows, dL = 0 with removed lhs
    rows, an edit across the chunk seam, and every resident row removed with only rows of the block left."""
    case, idx = FUSED[name]
    if name == "dl0_lhs_removed":
        lhs_rows = np.flatnonzero(lpstate.finite(np.asarray(A.case(case).rows.row_lhs), 1e20))
        idx = lhs_rows[:4].tolist() + [41]
    if name == "seam":
        idx = [0, 255, 256, 300, 400, 511, 512]
    rows, block, idx, rnd, snap, before, after = _fused_case(case, idx, 31)
    _four_ways(model, rows, before, rnd, snap, after, block=block, idx=idx)


def test_block_only_indices_are_the_plain_fused_call(model):
    """Indices that point only into the block: the device sees no removal, and the launch list is the plain fused call's."""
    rows, block, idx, rnd, snap, before, after = _fused_case("kinds", [41, 45], 32)
    sess, twin = LPSession(model, rows), LPSession(model, rows)
    sess.score(before)
    twin.score(before)
    with _lib.launch_profile() as got:
        a = sess.select_cuts(rnd, append=block, remove=idx)
    with _lib.launch_profile() as want:
        b = twin.select_cuts(rnd, append=lpstate.block_without(block, np.asarray([1, 5])))
    names = [n for n, _ in got.launches]
    assert names == [n for n, _ in want.launches] and names[:4] == APPEND_NAMES and not [n for n in names if n.startswith("k_lpd_")]
    _same_selection(a, b)
    _same_selection(a, model.select_cuts_lp(snap))
    _same_resident(sess, twin)
    assert sess._transit == [None] and sess._raw_alt is None
    # a block that loses all its rows, with no resident row removed: a plain round
    with _lib.launch_profile() as got:
        sess.select_cuts(rnd, append=block, remove=sess.n_rows + np.arange(10))
    with _lib.launch_profile() as want:
        twin.select_cuts(rnd)
    assert [n for n, _ in got.launches] == [n for n, _ in want.launches]


def test_transit_set_and_both_parities(model):
    """Calls that carry both edits go current -> transit -> the other of `_sets`; the transit set is never the current one."""
    rows, block, idx, rnd, snap, before, after = _fused_case("kinds", [3, 44, 17], 33)
    sess = GuardedSession(model, rows)
    sess.score(before)
    parities, host = set(), rows
    for step in range(3):
        host = lpstate.rows_without(lpstate.rows_with(host, block), idx)
        rnd = A._round_for(np.random.default_rng(40 + step), host, snap)
        got = sess.select_cuts(rnd, append=block, remove=idx)
        _same_selection(got, model.select_cuts_lp(lpstate.assemble(host, rnd)))
        parities.add(sess._cur_set)
        transit = sess._transit[0]
        assert transit is not None and transit[0] is not sess._cur and all(transit[0] is not s[0] for s in sess._sets if s is not None)
        assert sess._raw_alt is not None and all(a is not b for a in sess._raw for b in sess._raw_alt)
    assert parities == {0, 1}
    fresh = LPSession(model, host)
    _same_resident(sess, fresh)
    assert sess.guards_intact()
    sess.close()
    assert sess._sets == [None, None] and sess._transit == [None] and sess._raw_alt is None and sess._cur is None


def test_separation_loop_with_clean_up(model):
    """Thirty rounds through one session: each appends the cuts the previous selection kept and removes three earlier cut rows
    picked by a seeded rng, in one call.  Both raw sets and all derived sets grow on the way; the state is compared with a fresh
    session's at rounds 10, 28 and 29."""
    rng, base, pools = A.loop_script()
    pick = np.random.default_rng(181)
    rows = lpstate.LPRows.from_snapshot(base)
    n_base = np.asarray(rows.row_lhs).shape[0]
    sess = GuardedSession(model, rows)
    forced = _forced(64, seed=9)
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    block, raw_caps, alt_caps, set_caps, transit_caps, parities, removals = None, {sess._cap}, set(), [set(), set()], set(), set(), 0
    for i, pool in enumerate(pools):
        idx = None
        if block is not None:
            rows = lpstate.rows_with(rows, block)
            n = np.asarray(rows.row_lhs).shape[0]
            if n - n_base >= 6:
                idx = n_base + pick.choice(n - n_base, size=3, replace=False)       # cut rows, just-appended ones among them
                rows = lpstate.rows_without(rows, idx)
                removals += 1
        rnd = lpstate.LPRound(**A.S._solve(rng, rows, 64, col_lp=base.col_lp), **A.S._cuts_of(pool), **(full if i % 4 == 0 else {}),
                              has_incumbent=True)
        got = sess.select_cuts(rnd, forced, max_selected=8, append=block, remove=idx)
        want = model.select_cuts_lp(lpstate.assemble(rows, rnd, full), forced, max_selected=8)
        _same_selection(got, want)
        assert sess.n_rows == np.asarray(rows.row_lhs).shape[0]
        raw_caps.add(sess._cap)
        alt_caps.add(sess._cap_alt)
        if sess._transit[0] is not None:
            transit_caps.add(sess._transit[0][1])
        if sess._cur_set >= 0:
            set_caps[sess._cur_set].add(sess._sets[sess._cur_set][1])
            parities.add(sess._cur_set)
        if i in (10, 28, 29):
            fresh = LPSession(model, rows)
            _same_resident(sess, fresh)
            _same_selection(got, fresh.select_cuts(dataclasses.replace(rnd, **full), forced, max_selected=8))
            fresh.close()
        block = A.cuts_as_rows(pool, got.cut_index[got.order[:got.n_selected]])
        assert np.asarray(block.row_lhs).shape[0] == got.n_selected > 0
    assert removals >= 25 and parities == {0, 1}
    assert len(raw_caps) >= 3 and len(alt_caps) >= 3 and all(len(s) >= 2 for s in set_caps) and len(transit_caps) >= 2     # every buffer grew
    assert sess.guards_intact()
    sess.close()
    assert sess._sets == [None, None] and sess._cur is None


def test_none_rules_behind_a_removal(model):
    """The optional column arrays of a round that carries a removal: None keeps what the last accepted round gave."""
    c = D.case("kinds")
    after = lpstate.rows_without(c.rows, c.idx)
    sess = LPSession(model, c.rows)
    sess.score(c.before)
    kept = {n: getattr(c.before, n) for n in lpstate.OPTIONAL}
    rnd = dataclasses.replace(c.rnd, col_lb=None, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    _same_selection(sess.select_cuts(rnd, remove=c.idx), model.select_cuts_lp(lpstate.assemble(after, rnd, kept)))
    sess = LPSession(model, c.rows)
    sess.score(c.before)
    V = sess.n_cols
    ub = np.where(np.arange(V) % 3 == 0, lpcases.INF, 2.0)
    rnd = dataclasses.replace(c.rnd, col_lb=None, col_ub=ub, col_primal=None, col_primal_avg=None, has_incumbent=False)
    _same_selection(sess.select_cuts(rnd, remove=c.idx), model.select_cuts_lp(lpstate.assemble(after, rnd, kept)))
    rnd = dataclasses.replace(c.rnd, col_lb=None, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    _same_selection(sess.select_cuts(rnd), model.select_cuts_lp(lpstate.assemble(after, rnd, dict(kept, col_ub=ub))))
    fresh = LPSession(model, c.rows)                                 # a first round must give the bounds, removal or not
    with pytest.raises(ValueError, match="first round"):
        fresh.select_cuts(rnd, remove=c.idx)
    assert fresh.n_rows == np.asarray(c.rows.row_lhs).shape[0]


def test_rejection_leaves_the_session_as_it_was(model):
    """deep=False: a round whose cut has a column out of range, in a call that carries both `append` and `remove` -- and the host
    checks, and a block the device flags behind a sound removal: each raises, leaves n_rows and the resident state as before and
    the guards intact.  The same edit with a sound round then succeeds and equals the fresh session."""
    rows, block, idx, rnd, snap, before, after = _fused_case("kinds", [2, 44, 9], 34)
    sess, twin = GuardedSession(model, rows, deep=False), LPSession(model, rows, deep=False)
    first = sess.score(before, rank=True)
    _same_scores(first, twin.score(before, rank=True))
    R0, V = sess.n_rows, sess.n_cols
    ub_bad = np.where(np.arange(V) % 2 == 0, lpcases.INF, 3.0)
    bad_round = dataclasses.replace(rnd, cut_col=np.where(np.arange(rnd.cut_col.size) == 3, V + 5, rnd.cut_col), col_ub=ub_bad,
                                    col_primal=np.asarray(rnd.col_primal) + 1.0)
    alone = A._round_for(np.random.default_rng(38), lpstate.rows_without(rows, [2, 9]), snap)
    bad_alone = dataclasses.replace(alone, cut_col=np.where(np.arange(alone.cut_col.size) == 3, V + 5, alone.cut_col))
    ptr, col, val, lhs, rhs = block.arrays()
    outside = col.copy()
    outside[ptr[3]] = V + 7
    plain = dataclasses.replace(before, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    attempts = (
        (ValueError, "outside", lambda: sess.select_cuts(bad_round, append=block, remove=idx)),
        (ValueError, "outside", lambda: sess.score(bad_alone, remove=[2, 9])),
        (ValueError, "outside", lambda: sess.select_cuts(rnd, append=lpstate.LPRowBlock(ptr, outside, val, lhs, rhs), remove=idx)),
        (ValueError, "integers", lambda: sess.select_cuts(rnd, append=block, remove=[2.0, 9.0])),
        (ValueError, r"outside \[0, 50\)", lambda: sess.select_cuts(rnd, append=block, remove=[50])),
        (ValueError, r"outside \[0, 40\)", lambda: sess.remove_rows([40])),
        (ValueError, "twice", lambda: sess.state(rnd, append=block, remove=[2, 44, 2])),
        (ValueError, "no row at all", lambda: sess.remove_rows(np.arange(R0))),
        (ValueError, "no row at all", lambda: sess.score(rnd, append=block, remove=np.arange(R0 + 10))),
        (ValueError, "row_dual", lambda: sess.select_cuts(before, append=block, remove=idx)))     # (the round must cover the kept rows)
    for exc, match, attempt in attempts:
        with pytest.raises(exc, match=match):
            attempt()
        assert sess.n_rows == R0
        _same_resident(sess, twin)
        _same_scores(sess.score(plain, rank=True), first)
        assert sess.guards_intact()
    assert "col_ub" not in sess._stale                               # (the plain rounds above brought the stale arrays up again)
    fresh = LPSession(model, after)
    _same_selection(sess.select_cuts(rnd, append=block, remove=idx), model.select_cuts_lp(snap))
    _same_resident(sess, fresh)
    assert sess.guards_intact()


def test_launches_and_upload_of_a_fused_removal(model):
    """The removal's three launches, then the append's four, then exactly a plain round's list; one upload whose size the
    layout predicts: the inner call's plus the list padded to 256 bytes."""
    c = D.case("seam_513_n257")
    after = lpstate.rows_without(c.rows, c.idx)
    sess, fresh = LPSession(model, c.rows), LPSession(model, after)
    sess.score(c.before)
    fresh.score(c.rnd)
    with _lib.launch_profile() as plain:
        fresh.select_cuts(c.rnd)
    predicted = sess.upload_bytes(c.rnd, NO_FORCED, remove=c.idx)
    assert predicted == fresh.upload_bytes(c.rnd, NO_FORCED) + (4 * 257 + 255) // 256 * 256
    timings = {}
    with _lib.launch_profile() as prof:
        sess.select_cuts(c.rnd, timings=timings, remove=c.idx)
    names = [n for n, _ in prof.launches]
    assert names[:3] == NAMES and names[3:] == [n for n, _ in plain.launches], names
    assert timings["upload_bytes"] == predicted
    with _lib.launch_profile() as prof:                              # a plain round of the edited session: unchanged
        sess.select_cuts(c.rnd)
    assert [n for n, _ in prof.launches] == [n for n, _ in plain.launches]
    # with an append behind the removal
    rows, block, idx, rnd, snap, before, after = _fused_case("seam_257_257", [0, 255, 256, 300, 513], 35)
    sess, fresh, twin = LPSession(model, rows), LPSession(model, after), LPSession(model, lpstate.rows_without(rows, [0, 255, 256]))
    sess.score(before)
    fresh.score(rnd)
    with _lib.launch_profile() as plain:
        fresh.select_cuts(rnd)
    filtered = lpstate.block_without(block, np.asarray([43, 256]))
    predicted = sess.upload_bytes(rnd, NO_FORCED, append=block, remove=idx)
    assert predicted == twin.upload_bytes(rnd, NO_FORCED, append=filtered) + 256
    timings = {}
    with _lib.launch_profile() as prof:
        got = sess.select_cuts(rnd, timings=timings, append=block, remove=idx)
    names = [n for n, _ in prof.launches]
    assert names[:3] == NAMES and names[3:7] == APPEND_NAMES and names[7:] == [n for n, _ in plain.launches], names
    assert timings["upload_bytes"] == predicted
    _same_selection(got, model.select_cuts_lp(snap))
    _same_resident(sess, fresh)


def test_group_answers_a_member_with_a_removal_through_its_solo_call(model, dev):  # noqa: F811
    """Three sessions, one of them with `removes=`: that one is answered solo (`solo_rounds == 1`), the others keep their batched
    call, and all three equal their solo twins."""
    c, d = A.case("kinds"), D.case("kinds")
    rows, block, idx, rnd, snap, before, after = _fused_case("kinds", [2, 44, 9], 36)
    jobs = [(c.rows, c.before, c.rnd, c.block, None), (rows, before, rnd, block, idx), (d.rows, d.before, d.before, None, None)]
    sessions = [LPSession(model, j[0]) for j in jobs]
    twins = [LPSession(model, j[0]) for j in jobs]
    for s, t, j in zip(sessions, twins, jobs):
        s.score(j[1])
        t.score(j[1])
    group = LPSessionGroup(dev)
    forced = [_forced(64, seed=11 + i) for i in range(3)]
    got = group.select_cuts(sessions, [j[2] for j in jobs], forced, max_selected=5, appends=[j[3] for j in jobs], removes=[j[4] for j in jobs])
    assert group.solo_rounds == 1 and group.calls == 1 and group.max_sessions_per_call == 2
    for s, t, j, f, g in zip(sessions, twins, jobs, forced, got):
        _same_selection(g, t.select_cuts(j[2], f, max_selected=5, append=j[3], remove=j[4]))
        _same_resident(s, t)
    _same_selection(got[1], model.select_cuts_lp(snap, forced[1], max_selected=5))
    # the scores, with a removal alone in one member and an empty list (no removal: the batched call) in another
    rnd2 = A._round_for(np.random.default_rng(37), lpstate.rows_without(d.rows, d.idx), d.snap)
    rounds = [c.rnd, rnd, rnd2]
    removes = [[], None, d.idx]
    got = group.score(sessions, rounds, rank="device", removes=removes)
    assert group.solo_rounds == 2 and group.calls == 2
    for s, t, r, m, g in zip(sessions, twins, rounds, removes, got):
        _same_scores(g, t.score(r, rank="device", remove=m))
        _same_resident(s, t)
    with pytest.raises(ValueError, match="one entry per session"):
        group.score(sessions, rounds, removes=[None])
