"""The incremental append to a resident LP (`LPSession.append_rows(incremental=True)`, the `append=` of a round; csrc/k_lpappend.hpp)
on the GPU.  Every check is made against two independent answers with `np.array_equal` -- the full-snapshot call on the assembled
snapshot, and a FRESH session opened on all rows, whose resident state (static constraint features, row places and scales, the six
graph arrays, the longest segments) the appended session's must equal bit for bit.  No tolerance anywhere."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lpappendcases as A  # noqa: E402
import lpcases  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate  # noqa: E402
from gcnn_cut_selector_amd.infer import LPSession  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

NAMES = ["k_lpa_stats", "k_lpa_scan", "k_lpa_move", "k_lpa_order"]
RESIDENT = ("row_place", "row_scale", "l_ptr", "edge_row", "edge_col", "edge_coef", "v_ptr", "v_oth", "v_coef", "l_max_deg", "v_max_deg",
            "n_rows", "n_state_rows", "n_state_edges")


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


@pytest.mark.parametrize("name", A.CASES)
def test_append_cases(model, name):
    """Kinds of appended row, dL = 0, L0 = 0, H0 = 0, the chunk seams, the variables' splits, a hub column, V = 1 / 257 / past a trip
    of the scan / 33,000 with a segment that becomes long only through the append: the fused selection, the fused state and
    score, and the incremental append alone, each against the snapshot call and a fresh session."""
    c = A.case(name)
    after = lpstate.rows_with(c.rows, c.block)
    fresh = LPSession(model, after)
    forced = _forced(fresh.n_cols)
    want_sel = model.select_cuts_lp(c.snap, forced, max_selected=5)
    want_state, want_index = model.state_from_lp(c.snap)
    want_q = model.score_lp(c.snap, rank=True)
    fresh_sel = fresh.select_cuts(c.rnd, forced, max_selected=5)
    _same_selection(fresh_sel, want_sel)
    # the selection with the append inside
    sess = GuardedSession(model, c.rows)
    sess.score(c.before)
    got = sess.select_cuts(c.rnd, forced, max_selected=5, append=c.block)
    _same_selection(got, want_sel)
    _same_selection(got, fresh_sel)
    assert sess.n_rows == fresh.n_rows
    _same_resident(sess, fresh)
    state, index = sess.state(c.rnd)
    assert _same(state, want_state) and np.array_equal(index, want_index)
    assert sess.guards_intact()
    sess.close()
    # the state and the scores with the append inside
    for call in ("state", "score"):
        sess = LPSession(model, c.rows)
        if call == "state":
            state, index = sess.state(c.rnd, append=c.block)
            assert _same(state, want_state) and np.array_equal(index, want_index)
        else:
            _same_scores(sess.score(c.rnd, rank=True, append=c.block), want_q)
        _same_resident(sess, fresh)
        sess.close()
    # the append alone
    sess = GuardedSession(model, c.rows)
    sess.append_rows(*c.block.arrays(), incremental=True)
    assert sess.n_rows == fresh.n_rows
    _same_resident(sess, fresh)
    _same_scores(sess.score(c.rnd, rank=True), want_q)
    _same_scores(sess.score(c.rnd, rank=True), fresh.score(c.rnd, rank=True))
    assert sess.guards_intact()


def test_segment_that_becomes_long_through_the_append(model):
    """V = 33,000: the last column passes 32 entries only through the append, so the by-variable edge pass needs its long-segment
    blocks from then on -- the host's longest segments, the launch list and the bits equal the fresh session's."""
    c = A.case("v33000")
    after = lpstate.rows_with(c.rows, c.block)
    fresh = LPSession(model, after)
    sess = LPSession(model, c.rows)
    before = sess.resident_state()["v_max_deg"]
    sess.append_rows(*c.block.arrays(), incremental=True)
    now = sess.resident_state()
    assert before <= 32 < now["v_max_deg"] == fresh.resident_state()["v_max_deg"] and now["l_max_deg"] == fresh.resident_state()["l_max_deg"]
    lists = []
    for s in (sess, fresh):
        s.score(c.rnd)
        with _lib.launch_profile() as prof:
            q = s.score(c.rnd, rank=True)
        lists.append(([n for n, _ in prof.launches], q))
    assert lists[0][0] == lists[1][0]
    _same_scores(lists[0][1], lists[1][1])
    _same_scores(lists[0][1], model.score_lp(c.snap, rank=True))


def test_separation_loop(model):
    """Thirty rounds through one session: each appends the cuts the previous selection kept and selects among new candidates with
    forced rows, in one call.  The raw buffers and both derived sets double on the way; the state is compared with a fresh
    session's on both parities of the ping-pong."""
    rng, base, pools = A.loop_script()
    rows = lpstate.LPRows.from_snapshot(base)
    sess = GuardedSession(model, rows)
    forced = _forced(64, seed=9)
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    block, raw_caps, set_caps, parities = None, {sess._cap}, [set(), set()], set()
    for i, pool in enumerate(pools):
        if block is not None:
            rows = lpstate.rows_with(rows, block)
        rnd = lpstate.LPRound(**A.S._solve(rng, rows, 64, col_lp=base.col_lp), **A.S._cuts_of(pool), **(full if i % 4 == 0 else {}),
                              has_incumbent=True)
        got = sess.select_cuts(rnd, forced, max_selected=5, append=block)
        want = model.select_cuts_lp(lpstate.assemble(rows, rnd, full), forced, max_selected=5)
        _same_selection(got, want)
        assert sess.n_rows == np.asarray(rows.row_lhs).shape[0]
        raw_caps.add(sess._cap)
        if sess._cur_set >= 0:
            set_caps[sess._cur_set].add(sess._sets[sess._cur_set][1])
            parities.add(sess._cur_set)
        if i >= len(pools) - 2 or i == 10:
            fresh = LPSession(model, rows)
            _same_resident(sess, fresh)
            _same_selection(got, fresh.select_cuts(dataclasses.replace(rnd, **full), forced, max_selected=5))
            fresh.close()
        block = A.cuts_as_rows(pool, got.cut_index[got.order[:got.n_selected]])
        assert np.asarray(block.row_lhs).shape[0] == got.n_selected > 0
    assert len(raw_caps) >= 3 and all(len(s) >= 2 for s in set_caps) and parities == {0, 1}      # every buffer doubled at least once
    assert sess._cur_set in (0, 1) and sess.guards_intact()
    sess.close()
    assert sess._sets == [None, None] and sess._cur is None


def test_none_rules_in_a_fused_round(model):
    """The optional column arrays of a round that carries an append: None keeps what the last accepted round gave; without an
    incumbent the kept incumbent arrays are not read."""
    c = A.case("kinds")
    after = lpstate.rows_with(c.rows, c.block)
    sess = LPSession(model, c.rows)
    sess.score(c.before)
    kept = {n: getattr(c.before, n) for n in lpstate.OPTIONAL}
    rnd = dataclasses.replace(c.rnd, col_lb=None, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    _same_selection(sess.select_cuts(rnd, append=c.block), model.select_cuts_lp(lpstate.assemble(after, rnd, kept)))
    sess = LPSession(model, c.rows)
    sess.score(c.before)
    V = sess.n_cols
    ub = np.where(np.arange(V) % 3 == 0, lpcases.INF, 2.0)
    rnd = dataclasses.replace(c.rnd, col_lb=None, col_ub=ub, col_primal=None, col_primal_avg=None, has_incumbent=False)
    _same_selection(sess.select_cuts(rnd, append=c.block), model.select_cuts_lp(lpstate.assemble(after, rnd, kept)))
    rnd = dataclasses.replace(c.rnd, col_lb=None, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    _same_selection(sess.select_cuts(rnd), model.select_cuts_lp(lpstate.assemble(after, rnd, dict(kept, col_ub=ub))))
    fresh = LPSession(model, c.rows)                                 # a first round must give the bounds, append or not
    with pytest.raises(ValueError, match="first round"):
        fresh.select_cuts(rnd, append=c.block)
    assert fresh.n_rows == np.asarray(c.rows.row_lhs).shape[0]


@pytest.mark.parametrize("name", ["kinds", "seam_256_257"])
def test_incremental_against_the_default(model, name):
    c = A.case(name)
    a, b = LPSession(model, c.rows), LPSession(model, c.rows)
    with _lib.launch_profile() as prof:
        a.append_rows(*c.block.arrays())
    assert [n for n, _ in prof.launches][:2] == ["k_lpr_rows_stats", "k_lpr_rows_emit"]          # the default is the rebuild
    with _lib.launch_profile() as prof:
        b.append_rows(*c.block.arrays(), incremental=True)
    assert [n for n, _ in prof.launches] == NAMES
    _same_resident(a, b)
    _same_scores(a.score(c.rnd, rank=True), b.score(c.rnd, rank=True))
    # and on from there: a rebuild behind an incremental append, an incremental append behind a rebuild
    a.append_rows(*c.block.arrays(), incremental=True)
    b.append_rows(*c.block.arrays())
    _same_resident(a, b)
    b.append_rows(*c.block.arrays()[:0] + (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0)),
                  incremental=True)                                  # zero rows: a no-op
    _same_resident(a, b)


def test_rejection_leaves_the_session_as_it_was(model):
    """deep=False: a block with unsorted columns, one with a column out of range, a valid block with a flagged round, the
    4,097-cut limit -- each raises, leaves n_rows and the next plain round identical to a session that never saw the call, and
    the guard bytes intact."""
    c = A.case("kinds")
    sess, twin = GuardedSession(model, c.rows, deep=False), LPSession(model, c.rows, deep=False)
    first = sess.score(c.before, rank=True)
    _same_scores(first, twin.score(c.before, rank=True))
    R0, V = sess.n_rows, sess.n_cols
    ptr, col, val, lhs, rhs = c.block.arrays()
    unsorted = col.copy()
    unsorted[ptr[2]], unsorted[ptr[2] + 1] = col[ptr[2] + 1], col[ptr[2]]
    outside = col.copy()
    outside[ptr[3]] = V + 7
    ub_bad = np.where(np.arange(V) % 2 == 0, lpcases.INF, 3.0)
    bad_round = dataclasses.replace(c.rnd, cut_col=np.where(np.arange(c.rnd.cut_col.size) == 3, V + 5, c.rnd.cut_col), col_ub=ub_bad,
                                    col_primal=np.asarray(c.rnd.col_primal) + 1.0)
    many = lpcases.snapshot("cuts4097")
    wide = dataclasses.replace(c.rnd, **{n: getattr(many, n) for n in ("cut_ptr", "cut_col", "cut_val", "cut_lhs", "cut_rhs")})
    plain = dataclasses.replace(c.before, col_ub=None, col_primal=None, col_primal_avg=None, has_incumbent=True)
    attempts = (
        (ValueError, "increasing", lambda: sess.select_cuts(c.rnd, append=lpstate.LPRowBlock(ptr, unsorted, val, lhs, rhs))),
        (ValueError, "outside", lambda: sess.score(c.rnd, append=lpstate.LPRowBlock(ptr, outside, val, lhs, rhs))),
        (ValueError, "outside", lambda: sess.select_cuts(bad_round, append=c.block)),
        (_lib.GcnnError, "4097 cuts", lambda: sess.select_cuts(wide, append=c.block)),
        (ValueError, "increasing", lambda: sess.append_rows(ptr, unsorted, val, lhs, rhs, incremental=True)),
        (ValueError, "outside", lambda: sess.append_rows(ptr, outside, val, lhs, rhs, incremental=True)),
        (ValueError, "row_dual", lambda: sess.select_cuts(c.before, append=c.block)))      # (the round must cover the new rows)
    for exc, match, attempt in attempts:
        with pytest.raises(exc, match=match):
            attempt()
        assert sess.n_rows == R0
        _same_resident(sess, twin)
        _same_scores(sess.score(plain, rank=True), first)
        assert sess.guards_intact()
    # and a good append goes through afterwards
    fresh = LPSession(model, lpstate.rows_with(c.rows, c.block))
    _same_selection(sess.select_cuts(c.rnd, append=c.block), model.select_cuts_lp(c.snap))
    _same_resident(sess, fresh)
    assert sess.guards_intact()


def test_launches_and_upload_of_a_fused_round(model):
    """The append's four launches, then exactly a plain round's list; one upload whose size the layout predicts."""
    c = A.case("seam_257_257")
    sess, fresh = LPSession(model, c.rows), LPSession(model, lpstate.rows_with(c.rows, c.block))
    sess.score(c.before)
    fresh.score(c.rnd)
    with _lib.launch_profile() as plain:
        fresh.select_cuts(c.rnd)
    predicted = sess.upload_bytes(c.rnd, (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)), append=c.block)
    timings = {}
    with _lib.launch_profile() as prof:
        sess.select_cuts(c.rnd, timings=timings, append=c.block)
    names = [n for n, _ in prof.launches]
    assert names[:4] == NAMES and names[4:] == [n for n, _ in plain.launches], names
    assert names[4:6] == ["k_lpr_stats", "k_lpr_emit"] and not [n for n in names[4:] if n.startswith("k_lpa_")]
    block_bytes = sum(a.nbytes for a in lpstate.check_row_block(*c.block.arrays(), sess.n_cols, 1e20)[0])
    assert timings["upload_bytes"] == predicted
    assert block_bytes <= predicted - fresh.upload_bytes(c.rnd, (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))) <= block_bytes + 256
    with _lib.launch_profile() as prof:                              # a plain round of the appended session: unchanged
        sess.select_cuts(c.rnd)
    assert [n for n, _ in prof.launches] == [n for n, _ in plain.launches]
