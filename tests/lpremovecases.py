"""Removals from a resident LP (`LPSession.remove_rows`, the `remove=` of a round; csrc/k_lpremove.hpp) at the places where the
compaction can go wrong.  A case is (rows resident before, the removed indices, the round that follows, the snapshot that round
stands for) plus the seam it is chosen for; built on tests/lpcases.py, tests/lpsessioncases.py and `lpappendcases.resident`.

`removed(state, rows, idx, defect)` restates the removal in NumPy by the layout
  rows          [ kept lhs | kept rhs, ids renumbered ]
  by-left edges [ kept lhs | kept rhs, at - removed edges in front, row id renumbered ]
  by-variable   per variable the kept entries of its old segment, in their old order, row ids renumbered; v_ptr = old v_ptr -
                exclusive prefix of the removed counts
and can apply one of DEFECTS.  Without a defect it equals `resident` of `lpstate.rows_without(rows, idx)`
(tests/test_lpremovecases.py asserts that and holds every case to the defects it is chosen against)."""
import dataclasses
import functools

import numpy as np

import lpappendcases as A
import lpcases
import lpsessioncases as S
from gcnn_cut_selector_amd import lpstate

INF = lpcases.INF
CHUNK = lpcases.CHUNK

DEFECTS = {
    "rhs_ids_not_renumbered": "rhs row ids not renumbered by the removed lhs rows",
    "places_not_renumbered": "row_place of the kept rhs sides not renumbered",
    "l_ptr_last_not_moved": "l_ptr's last entry not moved",
    "one_side_dropped": "only one side of a removed two-sided row dropped",
    "free_row_counted": "a removed free row counted as a state row",
    "next_row_dropped": "the row behind a removed one dropped as well (<= for < in the search)",
    "chunk_skipped": "a chunk without a kept row skipped in the prefix",
    "v_ptr_left": "a variable's segment compacted but v_ptr left",
    "reversed": "kept entries of a variable written in reversed order",
}
STATE_ARRAYS = A.STATE_ARRAYS


@dataclasses.dataclass
class Case:
    rows: lpstate.LPRows
    idx: np.ndarray               # the removed rows (any order)
    rnd: lpstate.LPRound          # the round after the removal
    snap: lpstate.LPSnapshot      # what it stands for
    before: lpstate.LPRound       # a round on the rows before it
    against: tuple


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def removed(old, rows, idx, defect=None):
    """The resident state after removing the rows `idx` from `old` = resident(rows), by the removal's layout."""
    lhs, rhs = np.asarray(rows.row_lhs, np.float64), np.asarray(rows.row_rhs, np.float64)
    has_l, has_r = A._sides(lhs, rhs, rows.infinity)
    R0 = lhs.shape[0]
    idx = np.sort(np.asarray(idx, np.int64))
    gone = np.zeros(R0, bool)
    gone[idx] = True
    if defect == "next_row_dropped":
        gone[idx[idx + 1 < R0] + 1] = True
    place = old["row_place"]
    C0, E0, L0 = old["cons_static"].shape[0], old["edge_row"].shape[0], old["n_lhs"]
    V = old["v_ptr"].shape[0] - 1
    keep = np.ones(C0, bool)
    for r in np.flatnonzero(gone):
        two = has_l[r] and has_r[r]
        if has_l[r]:
            keep[place[r, 0]] = False
        if has_r[r] and not (two and defect == "one_side_dropped"):
            keep[place[r, 1]] = False
        if defect == "free_row_counted" and not (has_l[r] or has_r[r]):
            p = L0 + int(has_r[:r].sum())            # the place a free row would take as an rhs side
            if p < C0:
                keep[p] = False
    new_id = np.where(keep, np.cumsum(keep) - 1, -1)
    ids = new_id.copy()
    if defect == "rhs_ids_not_renumbered":           # the rhs rows keep the old count of lhs rows in front
        rhs_rank = np.cumsum(keep[L0:]) - 1
        ids[L0:] = np.where(keep[L0:], L0 + rhs_rank, -1)
    out = {"cons_static": old["cons_static"][keep]}
    e_keep = keep[old["edge_row"]]
    out["edge_row"] = ids[old["edge_row"]][e_keep]
    out["edge_col"], out["edge_coef"] = old["edge_col"][e_keep], old["edge_coef"][e_keep]
    l_ptr = np.concatenate([[0], np.cumsum(np.diff(old["l_ptr"])[keep])]).astype(np.int64)
    if defect == "l_ptr_last_not_moved":
        l_ptr[-1] = E0
    out["l_ptr"] = l_ptr
    # by row: the new LP row of a kept row is the kept rows in front -- per chunk of 256 a prefix over the chunks, then a local rank
    stay = ~gone
    new_r = np.cumsum(stay) - 1
    if defect == "chunk_skipped":
        per_chunk = np.add.reduceat(stay.astype(np.int64), np.arange(0, R0, CHUNK))
        rank = np.cumsum(per_chunk > 0) - (per_chunk > 0)        # the chunk's index among the chunks with a kept row
        front = np.concatenate([[0], np.cumsum(per_chunk)])[rank]
        local = np.concatenate([np.cumsum(c) - 1 for c in np.split(stay.astype(np.int64), np.arange(CHUNK, R0, CHUNK))])
        new_r = np.repeat(front, np.minimum(CHUNK, R0 - np.arange(0, R0, CHUNK))) + local
    n_stay = int(stay.sum())
    place_new = np.where(place >= 0, new_id[np.maximum(place, 0)], -1)
    if defect == "places_not_renumbered":
        place_new[:, 1] = place[:, 1]
    row_place, row_scale = np.full((n_stay, 2), -1, np.int64), np.zeros(n_stay)
    at = new_r[stay]
    row_place[at], row_scale[at] = place_new[stay], old["row_scale"][stay]
    out["row_place"], out["row_scale"] = row_place, row_scale
    # by variable
    var = np.repeat(np.arange(V), np.diff(old["v_ptr"]))
    v_keep = keep[old["v_oth"]]
    order = np.flatnonzero(v_keep)
    if defect == "reversed":
        order = order[np.lexsort((-order, var[order]))]
    out["v_oth"], out["v_coef"] = ids[old["v_oth"]][order], old["v_coef"][order]
    out["v_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(var[v_keep], minlength=V))]).astype(np.int64)
    if defect == "v_ptr_left":
        out["v_ptr"] = old["v_ptr"].copy()
    left = keep[:L0]
    out["n_lhs"] = int(left.sum())
    out["n_lhs_edges"] = int(np.diff(old["l_ptr"])[:L0][left].sum())
    deg_l, deg_v = np.diff(out["l_ptr"]), np.bincount(var[v_keep], minlength=V)
    out["l_max_deg"] = int(deg_l.max()) if deg_l.size and out["edge_row"].size else 0
    out["v_max_deg"] = int(deg_v.max()) if V and out["edge_row"].size else 0
    return out


def moved(a, b):
    """The named arrays in which two resident states differ."""
    return [n for n in STATE_ARRAYS if a[n].shape != b[n].shape or not np.array_equal(a[n], b[n], equal_nan=True)]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _case(rng, base, rows, idx, against):
    idx = np.asarray(idx, np.int64)
    after = lpstate.rows_without(rows, idx)
    rnd = A._round_for(rng, after, base)
    return Case(rows, idx, rnd, lpstate.assemble(after, rnd), A._round_for(rng, rows, base), tuple(against))


def _with_column_in(block, column, where, value=1.5):
    """`block` with `column` in exactly the rows `where` (columns stay increasing)."""
    ptr, col, val, lhs, rhs = A._without_columns(block, [column])
    rows = []
    for i in range(len(ptr) - 1):
        c, x = col[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
        if i in where:
            at = int(np.searchsorted(c, column))
            c, x = np.insert(c, at, column), np.insert(x, at, value)
        rows.append((c, x))
    lens = np.array([r[0].size for r in rows])
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate([r[0] for r in rows]).astype(np.int32),
            np.concatenate([r[1] for r in rows]), lhs, rhs)


def _block_of(rows):
    return tuple(np.asarray(getattr(rows, n)) for n in ("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs"))


KINDS_40 = (0, 1, 2, 3, 4) * 8        # 0 rhs-only, 1 lhs-only, 2 equality, 3 ranged, 4 free
SHIFTS = ("rhs_ids_not_renumbered", "places_not_renumbered", "l_ptr_last_not_moved")
BY_VAR = ("v_ptr_left", "reversed")
SEAM_R0 = (255, 256, 257, 513)
SEAM_PICKS = ("first", "last", "seam", "chunk0", "alternate", "n1", "n255", "n256", "n257")


def _kinds_rows(rng, base, kinds=KINDS_40, empty=7):
    """Rows of every kind over `base`'s columns; row `empty` (ranged) has no entries."""
    ptr, col, val, lhs, rhs = S._row_block(rng, kinds, 64, np.asarray(base.col_lp))
    if empty is not None:
        keep = np.ones(col.size, bool)
        keep[ptr[empty]:ptr[empty + 1]] = False
        lens = np.diff(ptr); lens[empty] = 0
        ptr, col, val = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), col[keep], val[keep]
    return A._rows_of(base, (ptr, col, val, lhs, rhs))


def _seam_idx(rng, r0, pick):
    if pick == "first":
        return [0]
    if pick == "last":
        return [r0 - 1]
    if pick == "seam":
        return [255, 256] if r0 > 256 else [r0 - 2, r0 - 1]
    if pick == "chunk0":
        return list(range(min(CHUNK, r0 - 1)))
    if pick == "alternate":
        return list(range(0, r0, 2))
    return sorted(rng.choice(r0, size=min(int(pick[1:]), r0 - 1), replace=False).tolist())


def _make_case(name):
    if name in ("kinds", "free_only", "all_lhs", "all_rhs", "free_left", "one_left"):
        rng = np.random.default_rng(201)
        base = lpcases._make(seed=202, R=8, V=64, K=12, short_rows=False)
        rows = _kinds_rows(rng, base)
        k = np.asarray(KINDS_40)
        idx, against = {
            "kinds": ([5, 6, 7, 8, 9], SHIFTS + BY_VAR + ("one_side_dropped", "free_row_counted", "next_row_dropped")),
            "free_only": (np.flatnonzero(k == 4)[:5], ("free_row_counted", "next_row_dropped")),
            "all_lhs": (np.flatnonzero(np.isin(k, (1, 2, 3))), ("one_side_dropped", "l_ptr_last_not_moved", "places_not_renumbered")),
            "all_rhs": (np.flatnonzero(np.isin(k, (0, 2, 3))), ("one_side_dropped", "l_ptr_last_not_moved")),
            "free_left": (np.flatnonzero(k != 4), ("one_side_dropped", "l_ptr_last_not_moved")),
            "one_left": (np.delete(np.arange(40), 3), ("one_side_dropped", "l_ptr_last_not_moved")),
        }[name]
        return _case(rng, base, rows, idx, against)
    if name.startswith("seam_"):
        _, r0, pick = name.split("_")
        r0 = int(r0)
        rng = np.random.default_rng(1000 * r0 + SEAM_PICKS.index(pick))
        base = lpcases._make(seed=230 + r0, R=r0, V=64, K=12, short_rows=False)
        rows, idx = lpstate.LPRows.from_snapshot(base), np.asarray(_seam_idx(rng, r0, pick))
        # (the first and last row of every chunk of these rows is free or empty: what a removal can move depends on the rows' kinds)
        has_l, has_r = A._sides(np.asarray(rows.row_lhs), np.asarray(rows.row_rhs), rows.infinity)
        entries = np.diff(rows.row_ptr)[idx]
        against = ("reversed",) if r0 - idx.size >= 20 else ()     # (a column needs two kept entries for an order to show)
        if has_l[idx].any() and np.delete(has_r, idx).any():        # (a kept rhs side behind a removed lhs side)
            against += ("places_not_renumbered",)
        if has_l[idx].any() and np.delete(has_r & (np.diff(rows.row_ptr) > 0), idx).any():     # (and it has an edge to carry its id)
            against += ("rhs_ids_not_renumbered",)
        if ((has_l | has_r)[idx] & (entries > 0)).any():
            against += ("l_ptr_last_not_moved", "v_ptr_left")
        if (~(has_l | has_r))[idx].any() and pick in ("first", "last", "seam"):
            against += ("free_row_counted",)
        if pick == "chunk0" and r0 > 2 * CHUNK:                     # (a chunk with kept rows behind the one without)
            against += ("chunk_skipped",)
        return _case(rng, base, rows, idx, against)
    if name == "var_edges":      # column 0: its only entry goes; column 1: its first; column 2: its last; column 63: one of two
        rng = np.random.default_rng(241)
        base = lpcases._make(seed=242, R=8, V=64, K=12, short_rows=False)
        block = S._row_block(rng, (1, 0, 3) * 10, 64, np.asarray(base.col_lp))
        for column, where in ((0, {3}), (1, {2, 10, 20}), (2, {5, 15, 25}), (63, {3, 29})):
            block = _with_column_in(block, column, where)
        return _case(rng, base, A._rows_of(base, block), [25, 2, 3], SHIFTS + BY_VAR)
    if name == "hub300":         # one column that 300 rows all hit, 150 of them removed, alternating
        rng = np.random.default_rng(251)
        base = lpcases._make(seed=252, R=40, V=64, K=12, short_rows=False)
        hub = A._with_column(rng, S._row_block(rng, A._kinds(300, rng, (0, 1, 3)), 64, np.asarray(base.col_lp)), 5, 64)
        rows = lpstate.rows_with(lpstate.LPRows.from_snapshot(base), lpstate.LPRowBlock(*hub))
        return _case(rng, base, rows, 40 + np.arange(0, 300, 2), SHIFTS + BY_VAR)
    if name == "v33000":         # the last column holds 33 entries, one of which goes: its segment stops being long
        V = 33000
        rng = np.random.default_rng(261)
        base = lpcases._make(seed=262, R=300, V=V, K=6, short_rows=True)
        rows = lpstate.LPRows.from_snapshot(base)
        rows = dataclasses.replace(rows, **dict(zip(("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs"),
                                                    A._without_columns(_block_of(rows), [V - 1]))))
        extra = lpstate.LPRowBlock(np.arange(0, 67, 2, dtype=np.int32), np.stack([100 + np.arange(33), np.full(33, V - 1)], 1).ravel().astype(np.int32),
                                   np.round(rng.uniform(0.5, 3.0, 66), 3), np.full(33, -INF), np.full(33, 5.0))
        return _case(rng, base, lpstate.rows_with(rows, extra), [300 + 16, 4, 250], SHIFTS + BY_VAR)
    if name.startswith("v"):     # V = 1, 257, one past a trip over the chunk counters
        V = int(name[1:])
        rng = np.random.default_rng(270 + V % 97)
        if V == 1:
            base = A._one_column(rng)
            return _case(rng, base, lpstate.LPRows.from_snapshot(base), [1, 2, 7, 19], SHIFTS + BY_VAR)
        base = lpcases._make(seed=271 + V % 89, R=300, V=V, K=6, short_rows=V > 1000)
        ends = lpstate.LPRowBlock(np.arange(0, 7, 2, dtype=np.int32), np.array([0, V - 1] * 3, np.int32), np.round(rng.uniform(0.5, 3.0, 6), 3),
                                  np.array([-1.0, -INF, -2.0]), np.array([INF, 4.0, 3.0]))
        rows = lpstate.rows_with(lpstate.LPRows.from_snapshot(base), ends)
        idx = np.concatenate([rng.choice(300, size=30, replace=False), [301]])
        return _case(rng, base, rows, idx, SHIFTS + BY_VAR)
    raise KeyError(name)


SIDE_CASES = ("all_lhs", "all_rhs", "free_left", "one_left")
SEAM_CASES = tuple(f"seam_{r0}_{pick}" for r0 in SEAM_R0 for pick in SEAM_PICKS if not (pick == "n257" and r0 <= 257))
V_CASES = ("v1", "v257", f"v{A.SCAN_TRIP + 464}")
CASES = ("kinds", "free_only") + SIDE_CASES + SEAM_CASES + ("var_edges", "hub300") + V_CASES + ("v33000",)
CPU_CASES = tuple(n for n in CASES if n not in (V_CASES[2], "v33000"))     # (the two largest V: GPU only, as lpappendcases)


@functools.lru_cache(maxsize=None)
def case(name):
    return _make_case(name)
