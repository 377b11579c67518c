"""Appends to a resident LP (`LPSession.append_rows(incremental=True)`, the `append=` of a round; csrc/k_lpappend.hpp) at the places
where the incremental merge can go wrong.  A case is (rows resident before, the appended block, the round that follows, the
snapshot that round stands for) plus the seam it is chosen for; built on tests/lpcases.py and tests/lpsessioncases.py.

`resident(rows)` restates in NumPy what a session holds of its rows -- the static constraint features, the edge list, both CSR
orders, the row places and scales, the longest segments -- from scratch; `merged(state, rows, block, defect)` restates the
incremental append: the block's own rows derived alone, everything old copied, shifted and merged by the layout
  rows          [ old lhs (L0) | new lhs (dL) | old rhs, ids + dL | new rhs ]
  by-left edges [ old lhs (EL0) | new lhs (dEL) | old rhs, at + dEL, row id + dL | new rhs ]
  by-variable   per variable [ old entries of rows < L0 | new lhs | old entries of rows >= L0, id + dL | new rhs ], new ascending by row
and can apply one of DEFECTS.  Without a defect it equals `resident` of the joined rows (tests/test_lpappendcases.py asserts that
and holds every case to the defects it is chosen against)."""
import dataclasses
import functools

import numpy as np

import lpcases
import lpsessioncases as S
from gcnn_cut_selector_amd import lpstate

INF = lpcases.INF
CHUNK = lpcases.CHUNK
SCAN_TRIP = CHUNK * CHUNK          # variables one trip of k_lpa_scan's loop over the chunk counters in front covers

DEFECTS = {
    "rhs_ids_not_shifted": "no + dL on the row ids of old rhs-sided edges",
    "places_not_shifted": "no + dL on old row_place entries of the rhs side",
    "new_lhs_at_end": "new lhs entries put at the end of a variable's segment",
    "placement_order": "new entries of a variable left in placement order",
    "split_after_new": "the split of a variable's old segment taken at L0 + dL",
    "free_row_counted": "a free row of the block takes a state place",
    "l_ptr_last_not_moved": "l_ptr's last entry not moved",
}
STATE_ARRAYS = ("cons_static", "edge_row", "edge_col", "edge_coef", "l_ptr", "v_ptr", "v_oth", "v_coef", "row_place", "row_scale")


@dataclasses.dataclass
class Case:
    rows: lpstate.LPRows
    block: lpstate.LPRowBlock
    rnd: lpstate.LPRound          # the round after the append
    snap: lpstate.LPSnapshot      # what it stands for
    before: lpstate.LPRound       # a round on the rows before it
    against: tuple


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _sides(lhs, rhs, inf, free_counts=False):
    has_l, has_r = lpstate.finite(lhs, inf), lpstate.finite(rhs, inf)
    if free_counts:
        has_r = has_r | ~(has_l | has_r)
    return has_l, has_r


def resident(rows, free_counts=False):
    """What a session holds of `rows` (fp64 values; int64 indices), built from scratch."""
    ptr, col, val = (np.asarray(getattr(rows, n)) for n in ("row_ptr", "row_col", "row_val"))
    lhs, rhs = np.asarray(rows.row_lhs, np.float64), np.asarray(rows.row_rhs, np.float64)
    inf, _, _, obj_norm = rows.scalars()
    obj = np.asarray(rows.col_obj, np.float64)
    n, V = lhs.shape[0], obj.shape[0]
    lens = np.diff(ptr).astype(np.int64)
    rid = np.repeat(np.arange(n), lens)
    norm = np.sqrt(np.bincount(rid, weights=val * val, minlength=n))
    norm[norm == 0] = 1.0
    den = norm * obj_norm
    cosine = np.bincount(rid, weights=val * obj[col], minlength=n) / den
    has_l, has_r = _sides(lhs, rhs, inf, free_counts)
    il, ir = np.flatnonzero(has_l), np.flatnonzero(has_r)
    place = np.full((n, 2), -1, np.int64)
    place[il, 0] = np.arange(il.size)
    place[ir, 1] = il.size + np.arange(ir.size)
    with np.errstate(invalid="ignore", over="ignore"):
        static = np.concatenate([np.stack([-(lhs / norm)[il], -cosine[il]], 1), np.stack([(rhs / norm)[ir], cosine[ir]], 1)], 0)
    e_row, e_col, e_coef = [], [], []
    for side, sign in ((0, -1.0), (1, 1.0)):
        keep = place[rid, side] >= 0
        e_row.append(place[rid, side][keep]); e_col.append(col[keep].astype(np.int64)); e_coef.append(sign * (val / norm[rid])[keep])
    e_row, e_col, e_coef = np.concatenate(e_row), np.concatenate(e_col), np.concatenate(e_coef)
    C = il.size + ir.size
    l_ptr = np.concatenate([[0], np.cumsum(np.bincount(e_row, minlength=C))]).astype(np.int64)
    perm = np.argsort(e_col, kind="stable")
    v_ptr = np.concatenate([[0], np.cumsum(np.bincount(e_col, minlength=V))]).astype(np.int64)
    return dict(cons_static=static, edge_row=e_row, edge_col=e_col, edge_coef=e_coef, l_ptr=l_ptr, v_ptr=v_ptr, v_oth=e_row[perm],
                v_coef=e_coef[perm], row_place=place, row_scale=den, n_lhs=int(il.size), n_lhs_edges=int(lens[il].sum()),
                l_max_deg=int(np.diff(l_ptr).max()) if C and e_row.size else 0, v_max_deg=int(np.diff(v_ptr).max()) if V and e_row.size else 0)


def block_rows(rows, block):
    """The block as an LP of its own over the same columns."""
    return lpstate.LPRows(*block.arrays(), rows.col_type, rows.col_obj, infinity=rows.infinity, sum_epsilon=rows.sum_epsilon,
                          n_model_vars=rows.n_model_vars, obj_norm=rows.scalars()[3])


def merged(old, rows, block, defect=None):
    """The resident state after appending `block` to `old` = resident(rows), by the incremental layout."""
    rows = dataclasses.replace(rows, obj_norm=rows.scalars()[3])
    new = resident(block_rows(rows, block), free_counts=defect == "free_row_counted")
    L0, EL0, dL, dEL = old["n_lhs"], old["n_lhs_edges"], new["n_lhs"], new["n_lhs_edges"]
    C0, E0 = old["cons_static"].shape[0], old["edge_row"].shape[0]
    dC, dE = new["cons_static"].shape[0], new["edge_row"].shape[0]
    V = old["v_ptr"].shape[0] - 1
    # where a new state row / by-left edge goes: its lhs part behind the old lhs part, its rhs part behind everything
    new_row = lambda p: np.where(p < dL, L0 + p, C0 + p)          # noqa: E731
    old_row = lambda p, shift=dL: np.where(p < L0, p, p + shift)   # noqa: E731
    out = {}
    static = np.zeros((C0 + dC, 2))
    static[old_row(np.arange(C0))] = old["cons_static"]
    static[new_row(np.arange(dC))] = new["cons_static"]
    out["cons_static"] = static
    at_old = np.where(np.arange(E0) < EL0, np.arange(E0), np.arange(E0) + dEL)
    at_new = np.where(np.arange(dE) < dEL, EL0 + np.arange(dE), E0 + np.arange(dE))
    ids_old = old_row(old["edge_row"], 0 if defect == "rhs_ids_not_shifted" else dL)
    for name, a_old, a_new in (("edge_row", ids_old, new_row(new["edge_row"])), ("edge_col", old["edge_col"], new["edge_col"]),
                               ("edge_coef", old["edge_coef"], new["edge_coef"])):
        a = np.zeros(E0 + dE, a_old.dtype)
        a[at_old], a[at_new] = a_old, a_new
        out[name] = a
    l_ptr = np.zeros(C0 + dC + 1, np.int64)
    l_ptr[old_row(np.arange(C0))] = np.where(np.arange(C0) < L0, old["l_ptr"][:C0], old["l_ptr"][:C0] + dEL)
    l_ptr[new_row(np.arange(dC))] = np.where(np.arange(dC) < dL, EL0 + new["l_ptr"][:dC], E0 + new["l_ptr"][:dC])
    l_ptr[C0 + dC] = E0 + dE if defect != "l_ptr_last_not_moved" else E0
    out["l_ptr"] = l_ptr
    place_old = old["row_place"].copy()
    if defect != "places_not_shifted":
        place_old[:, 1] = np.where(place_old[:, 1] >= 0, place_old[:, 1] + dL, -1)
    place_new = np.where(new["row_place"] >= 0, new_row(new["row_place"]), -1)
    out["row_place"] = np.concatenate([place_old, place_new])
    out["row_scale"] = np.concatenate([old["row_scale"], new["row_scale"]])
    # by variable: the four parts of every segment
    rng = np.random.default_rng(3)
    v_ptr = old["v_ptr"] + new["v_ptr"]
    v_oth, v_coef = np.zeros(E0 + dE, np.int64), np.zeros(E0 + dE)
    split_at = L0 + dL if defect == "split_after_new" else L0
    for v in range(V):
        ob, oe, nb, ne = old["v_ptr"][v], old["v_ptr"][v + 1], new["v_ptr"][v], new["v_ptr"][v + 1]
        if ob == oe and nb == ne:
            continue
        o_row, o_coef, n_row, n_coef = old["v_oth"][ob:oe], old["v_coef"][ob:oe], new["v_oth"][nb:ne], new["v_coef"][nb:ne]
        sp = int(np.searchsorted(o_row, split_at))
        is_l = n_row < dL
        parts = [(o_row[:sp], o_coef[:sp]), (L0 + n_row[is_l], n_coef[is_l]), (o_row[sp:] + dL, o_coef[sp:]),
                 (C0 + n_row[~is_l], n_coef[~is_l])]
        if defect == "placement_order":
            for k in (1, 3):
                p = rng.permutation(parts[k][0].size)[::-1] if parts[k][0].size > 1 else np.arange(parts[k][0].size)
                if parts[k][0].size > 1 and np.array_equal(p, np.arange(p.size)):
                    p = p[::-1]
                parts[k] = (parts[k][0][p], parts[k][1][p])
        if defect == "new_lhs_at_end":
            parts = [parts[0], parts[2], parts[3], parts[1]]
        v_oth[v_ptr[v]:v_ptr[v + 1]] = np.concatenate([p[0] for p in parts])
        v_coef[v_ptr[v]:v_ptr[v + 1]] = np.concatenate([p[1] for p in parts])
    out.update(v_ptr=v_ptr, v_oth=v_oth, v_coef=v_coef, n_lhs=L0 + dL, n_lhs_edges=EL0 + dEL)
    # the longest segments as the host keeps them: a running maximum over the rows, a per-column count
    out["l_max_deg"] = max(old["l_max_deg"], new["l_max_deg"])
    deg = np.diff(old["v_ptr"]) + np.diff(new["v_ptr"])
    out["v_max_deg"] = int(deg.max()) if V and deg.size and (E0 + dE) else 0
    return out


def same_resident(a, b):
    return all(a[n].shape == b[n].shape and np.array_equal(a[n], b[n], equal_nan=True) for n in STATE_ARRAYS) and all(
        a[n] == b[n] for n in ("n_lhs", "n_lhs_edges", "l_max_deg", "v_max_deg"))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _round_for(rng, rows, base, **over):
    V = np.asarray(rows.col_type).shape[0]
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    full.update(over)
    return lpstate.LPRound(**S._solve(rng, rows, V, col_lp=base.col_lp), **S._cuts_of(base), **full, has_incumbent=True)


def _case(rng, base, rows, block, against):
    block = lpstate.LPRowBlock(*block)
    after = lpstate.rows_with(rows, block)
    rnd = _round_for(rng, after, base)
    return Case(rows, block, rnd, lpstate.assemble(after, rnd), _round_for(rng, rows, base), tuple(against))


def _rows_of(base, block):
    """`base`'s columns with `block` as the only rows."""
    ptr, col, val, lhs, rhs = block
    return lpstate.LPRows(np.asarray(ptr, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64), np.asarray(lhs, np.float64),
                          np.asarray(rhs, np.float64), base.col_type, base.col_obj)


def _with_column(rng, block, column, V):
    """`block` with `column` added to every row that does not have it (columns stay increasing)."""
    ptr, col, val, lhs, rhs = block
    rows = []
    for i in range(len(ptr) - 1):
        c, x = col[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
        if column not in c:
            at = int(np.searchsorted(c, column))
            c, x = np.insert(c, at, column), np.insert(x, at, np.round(rng.uniform(0.5, 3.0), 3))
        rows.append((c, x))
    lens = np.array([r[0].size for r in rows])
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate([r[0] for r in rows]).astype(np.int32),
            np.concatenate([r[1] for r in rows]), lhs, rhs)


def _without_columns(block, columns):
    ptr, col, val, lhs, rhs = block
    keep = ~np.isin(col, columns)
    rid = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    lens = np.bincount(rid[keep], minlength=len(ptr) - 1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), col[keep], val[keep], lhs, rhs


def _one_column(rng):
    """A snapshot over a single column: 20 rows (every third empty) and 3 cuts of one entry each."""
    n = 20
    lens = (np.arange(n) % 3 != 0).astype(np.int64)
    nnz = int(lens.sum())
    one = lambda x: np.array([x])      # noqa: E731
    return lpstate.LPSnapshot(
        row_ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), row_col=np.zeros(nnz, np.int32),
        row_val=np.round(rng.uniform(0.5, 3.0, nnz), 3), row_lhs=np.where(np.arange(n) % 2 == 0, -2.0, -INF),
        row_rhs=np.where(np.arange(n) % 5 == 0, INF, 3.0), row_dual=rng.standard_normal(n), row_basis=rng.integers(0, 4, n).astype(np.int8),
        col_type=one(1).astype(np.int8), col_obj=one(1.5), col_lb=one(0.0), col_ub=one(1.0), col_basis=one(1).astype(np.int8),
        col_lp=one(0.5), col_redcost=one(0.0), cut_ptr=np.arange(4, dtype=np.int32), cut_col=np.zeros(3, np.int32),
        cut_val=np.array([1.0, -2.0, 0.5]), cut_lhs=np.array([-INF, -INF, 0.4]), cut_rhs=np.array([0.3, -1.2, INF]),
        col_primal=one(1.0), col_primal_avg=one(0.75))


SEAM_SIZES = [(r0, dr) for r0 in (255, 256, 257) for dr in (1, 255, 256, 257)]
ALL_SHIFTS = ("rhs_ids_not_shifted", "places_not_shifted", "l_ptr_last_not_moved")
ALL_MERGE = ("new_lhs_at_end", "placement_order", "split_after_new")


def _kinds(n, rng, allowed=(0, 1, 2, 3, 4)):
    k = rng.choice(allowed, n)
    k[:min(n, len(allowed))] = allowed[:min(n, len(allowed))]      # every allowed kind at least once where there is room
    return tuple(int(x) for x in k)


def _make_case(name):
    if name == "kinds":          # lhs only, rhs only, ranged, free, an empty row and a row of zero norm
        rng = np.random.default_rng(101)
        base = lpcases._make(seed=102, R=40, V=64, K=12, short_rows=False)
        ptr, col, val, lhs, rhs = S._row_block(rng, (1, 0, 3, 4, 3, 2, 3, 1, 0, 3), 64, np.asarray(base.col_lp))
        val = val.copy()
        val[ptr[5]:ptr[6]] = 0.0                                    # row 5 (an equality): zero norm
        keep = np.ones(col.size, bool)
        keep[ptr[6]:ptr[7]] = False                                 # row 6 (ranged): empty
        lens = np.diff(ptr); lens[6] = 0
        block = (np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), col[keep], val[keep], lhs, rhs)
        return _case(rng, base, lpstate.LPRows.from_snapshot(base), block, ALL_SHIFTS + ALL_MERGE + ("free_row_counted",))
    if name == "dl0":            # rhs-only rows: nothing shifts
        rng = np.random.default_rng(111)
        base = lpcases._make(seed=112, R=40, V=64, K=12, short_rows=False)
        block = S._row_block(rng, (0,) * 9 + (4,), 64, np.asarray(base.col_lp))
        return _case(rng, base, lpstate.LPRows.from_snapshot(base), block, ("free_row_counted", "l_ptr_last_not_moved"))
    if name in ("l0_zero", "h0_zero"):      # lhs rows onto a session without lhs rows / without rhs rows
        rng = np.random.default_rng(121 if name == "l0_zero" else 122)
        base = lpcases._make(seed=123, R=8, V=64, K=12, short_rows=False)
        rows = _rows_of(base, S._row_block(rng, (0,) * 30 if name == "l0_zero" else (1,) * 30, 64, np.asarray(base.col_lp)))
        block = S._row_block(rng, (1, 3, 0, 1, 3, 3, 1, 0, 3, 1, 1, 3), 64, np.asarray(base.col_lp))
        against = ALL_SHIFTS + ALL_MERGE if name == "l0_zero" else ("new_lhs_at_end", "placement_order", "l_ptr_last_not_moved")
        return _case(rng, base, rows, block, against)
    if name.startswith("seam_"):            # dR onto R0 around the 256 rows of a chunk
        r0, dr = (int(x) for x in name[5:].split("_"))
        rng = np.random.default_rng(1000 * r0 + dr)
        base = lpcases._make(seed=130 + r0, R=r0, V=64, K=12, short_rows=False)
        block = S._row_block(rng, (3,) if dr == 1 else _kinds(dr, rng), 64, np.asarray(base.col_lp))
        against = ALL_SHIFTS + ALL_MERGE if dr > 1 else ALL_SHIFTS + ("new_lhs_at_end", "split_after_new")   # (one row: no order)
        return _case(rng, base, lpstate.LPRows.from_snapshot(base), block, against)
    if name == "var_splits":     # column 0 has no old entries, column 1 only lhs-sided ones, column 2 only rhs-sided ones
        rng = np.random.default_rng(141)
        base = lpcases._make(seed=142, R=8, V=64, K=12, short_rows=False)
        lp = np.asarray(base.col_lp)
        kinds = (1,) * 10 + (0,) * 10 + (3,) * 10
        old = _without_columns(S._row_block(rng, kinds, 64, lp), [0, 1, 2])
        ptr, col, val, lhs, rhs = old
        # rebuild with column 1 in the lhs-only rows and column 2 in the rhs-only rows
        rows = []
        for i in range(30):
            c, x = col[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
            extra = 1 if i < 10 else (2 if i < 20 else None)
            if extra is not None:
                c, x = np.insert(c, 0, extra), np.insert(x, 0, 1.5)
            rows.append((c, x))
        lens = np.array([r[0].size for r in rows])
        old = (np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate([r[0] for r in rows]).astype(np.int32),
               np.concatenate([r[1] for r in rows]), lhs, rhs)
        block = S._row_block(rng, (3, 1, 0, 3, 3, 1, 0, 3), 64, lp)
        for c in (0, 1, 2):
            block = _with_column(rng, block, c, 64)
        return _case(rng, base, _rows_of(base, old), block, ALL_SHIFTS + ALL_MERGE)
    if name == "hub300":         # one column that 300 new rows all hit: more new entries than a block has threads
        rng = np.random.default_rng(151)
        base = lpcases._make(seed=152, R=40, V=64, K=12, short_rows=False)
        block = _with_column(rng, S._row_block(rng, _kinds(300, rng, (0, 1, 3)), 64, np.asarray(base.col_lp)), 5, 64)
        return _case(rng, base, lpstate.LPRows.from_snapshot(base), block, ALL_SHIFTS + ALL_MERGE)
    if name.startswith("v"):     # V = 1, 257, one past a trip of the scan's chunk loop, 33,000 (past the single call's limit)
        V = int(name[1:])
        rng = np.random.default_rng(160 + V % 97)
        base = _one_column(rng) if V == 1 else lpcases._make(seed=161 + V % 89, R=300, V=V, K=6, short_rows=True)
        lp = np.asarray(base.col_lp)
        if V == 1:
            n = 7
            block = (np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), np.round(rng.uniform(0.5, 3.0, n), 3),
                     np.where(np.arange(n) % 2 == 0, -1.0, -INF), np.where(np.arange(n) % 3 == 0, INF, 4.0))
        else:
            kinds = _kinds(40, rng, (0, 1, 3))
            lens = rng.integers(1, 4, 40)
            ptr, col = lpcases._columns(rng, lens, V)
            val = np.round(rng.uniform(0.5, 3.0, col.size), 3)
            act = np.bincount(np.repeat(np.arange(40), lens), weights=val * lp[col], minlength=40)
            k = np.asarray(kinds)
            block = (ptr, col, val, np.where(k == 0, -INF, act - 1.0), np.where(k == 1, INF, act + 1.0))
            # a segment that becomes long for the list's mean degree (over 32 entries at one lane group a segment) only through
            # the append: the last column, which also closes the by-variable scan
            block = _with_column(rng, block, V - 1, V)
        return _case(rng, base, lpstate.LPRows.from_snapshot(base), block, ALL_SHIFTS + ALL_MERGE)
    raise KeyError(name)


V_CASES = ("v1", "v257", f"v{SCAN_TRIP + 464}", "v33000")
SEAM_CASES = tuple(f"seam_{r0}_{dr}" for r0, dr in SEAM_SIZES)
CASES = ("kinds", "dl0", "l0_zero", "h0_zero", "var_splits", "hub300") + SEAM_CASES + V_CASES
CPU_CASES = tuple(n for n in CASES if n not in V_CASES[2:])     # (the two largest V: a per-variable Python loop is slow; GPU only)


@functools.lru_cache(maxsize=None)
def case(name):
    return _make_case(name)


def counts(c):
    """(R0, L0, H0, dR, dL, dH, free rows of the block) of a case."""
    inf = c.rows.infinity
    l0, h0 = _sides(np.asarray(c.rows.row_lhs), np.asarray(c.rows.row_rhs), inf)
    dl, dh = _sides(np.asarray(c.block.row_lhs), np.asarray(c.block.row_rhs), inf)
    return (l0.shape[0], int(l0.sum()), int(h0.sum()), dl.shape[0], int(dl.sum()), int(dh.sum()), int((~(dl | dh)).sum()))


# ---- the separation loop ---------------------------------------------------------------------------------------------------------------
def loop_script(n_rounds=30, seed=171):
    """A base LP (30 rows, 64 columns) and per round the candidate cuts (14 to 16 of them) and a solve generator: the loop appends
    the cuts the previous selection kept, as rhs- or lhs-sided rows, so what a round appends depends on the model's answers."""
    rng = np.random.default_rng(seed)
    base = lpcases._make(seed=seed + 1, R=30, V=64, K=16, short_rows=False)
    pools = [lpcases._make(seed=seed + 2 + i, R=1, V=64, K=14 + i % 3, short_rows=False) for i in range(n_rounds)]
    return rng, base, pools


def cuts_as_rows(pool, picked):
    """The cuts `picked` (input indices) of a pool snapshot as a block of rows."""
    ptr, col, val = np.asarray(pool.cut_ptr), np.asarray(pool.cut_col), np.asarray(pool.cut_val)
    picked = np.asarray(picked, np.int64)
    lens = (ptr[picked + 1] - ptr[picked]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in picked] + [np.zeros(0, np.int64)]).astype(np.int64)
    return lpstate.LPRowBlock(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), col[take].astype(np.int32), val[take],
                              np.asarray(pool.cut_lhs)[picked], np.asarray(pool.cut_rhs)[picked])
