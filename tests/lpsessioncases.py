"""Sessions of a resident LP (`GCNN.open_lp`, csrc/k_lpres.hpp) at the places where they can go wrong, as sequences of steps
  ("open", LPRows) | ("round", LPRound, assembled LPSnapshot) | ("append", (row_ptr, row_col, row_val, row_lhs, row_rhs))
where the assembled snapshot is what the round stands for by definition (`lpstate.assemble` of all rows so far, the round, and the
optional column arrays as the last rounds gave them).  Built on tests/lpcases.py (the seam snapshots and their generator) and the
hand-worked `small_lp()` variants.

`restated(steps, defect)` restates a session in NumPy (tests/lpstate_restate.py) -- the state of every round -- and can apply one
of DEFECTS, the mistakes an implementation of a session can make; tests/test_lpsessioncases.py holds every case to the defects it
is chosen against."""
import functools

import numpy as np

import lpcases
import lpstate_restate as R
from gcnn_cut_selector_amd import lpstate

INF = lpcases.INF
CHUNK = lpcases.CHUNK
K_SEQUENCE = (600, 5, 0, 513, 1100)
ROW_CASES = ("rows255", "rows256", "rows257", "rows600")


def split(snap):
    return lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)


def _single(snap):
    rows, rnd = split(snap)
    return [("open", rows), ("round", rnd, snap)]


def _solve(rng, snap_rows, V, **over):
    """A fresh solve for R rows and V columns: the per-round fields without cuts."""
    R_ = np.asarray(snap_rows.row_lhs).shape[0]
    row_basis = rng.integers(0, 4, R_).astype(np.int8)
    col_basis = rng.integers(0, 4, V).astype(np.int8)
    f = dict(row_dual=rng.standard_normal(R_) * (row_basis != 1), row_basis=row_basis, col_basis=col_basis,
             col_lp=np.where(rng.random(V) < 0.5, rng.integers(0, 2, V).astype(np.float64), rng.random(V)),
             col_redcost=rng.standard_normal(V) * (col_basis != 1))
    f.update(over)
    return f


def _cuts_of(snap):
    return {n: getattr(snap, n) for n in ("cut_ptr", "cut_col", "cut_val", "cut_lhs", "cut_rhs")}


def _row_block(rng, kinds, V, col_lp):
    """Rows of the given kinds (0 rhs-only, 1 lhs-only, 2 equality, 3 ranged, 4 free) with lengths around the 16 lanes of a row."""
    n = len(kinds)
    lens = rng.choice((1, 2, 15, 16, 17, 33), n)
    ptr, col = lpcases._columns(rng, lens, V)
    val = np.round(rng.uniform(0.5, 3.0, col.size), 3) * rng.choice([-1.0, 1.0], col.size)
    act = np.bincount(np.repeat(np.arange(n), lens), weights=val * col_lp[col], minlength=n)
    kinds = np.asarray(kinds)
    rhs = np.where((kinds == 1) | (kinds == 4), INF, act + rng.uniform(0.0, 2.0, n))
    lhs = np.where(kinds == 2, rhs, np.where((kinds == 0) | (kinds == 4), -INF, act - rng.uniform(0.1, 2.0, n)))
    return ptr, col, val, lhs, rhs


def _joined(rows, block):
    ptr, col, val, lhs, rhs = block
    base = int(np.asarray(rows.row_ptr)[-1])
    return lpstate.LPRows(row_ptr=np.concatenate([rows.row_ptr, np.asarray(ptr[1:]) + base]).astype(np.int32),
                          row_col=np.concatenate([rows.row_col, col]).astype(np.int32), row_val=np.concatenate([rows.row_val, val]),
                          row_lhs=np.concatenate([rows.row_lhs, lhs]), row_rhs=np.concatenate([rows.row_rhs, rhs]),
                          col_type=rows.col_type, col_obj=rows.col_obj, infinity=rows.infinity, sum_epsilon=rows.sum_epsilon,
                          n_model_vars=rows.n_model_vars, obj_norm=rows.obj_norm)


def _steps(rows, script):
    """script: ("round", LPRound) | ("append", block) -> steps with the assembled snapshots, tracking rows and kept arrays."""
    steps, kept = [("open", rows)], {}
    for item in script:
        if item[0] == "append":
            steps.append(item)
            if np.asarray(item[1][3]).shape[0]:
                rows = _joined(rows, item[1])
            continue
        rnd = item[1]
        snap = lpstate.assemble(rows, rnd, kept)
        steps.append(("round", rnd, snap))
        for name in lpstate.OPTIONAL:
            if getattr(rnd, name) is not None and not (name.startswith("col_primal") and not rnd.incumbent()):
                kept[name] = getattr(rnd, name)
    return steps


def _k_sequence():
    """Case 2: K = 600 -> 5 -> 0 -> 513 -> 1,100 through one session; every round has its own solve.  (lpcases._make draws the
    columns and rows before the cuts: the same seed, R and V give the same LP for every K.)"""
    snaps = [lpcases._make(seed=15, R=8, V=300, K=k, short_rows=False) for k in K_SEQUENCE]
    rows = lpstate.LPRows.from_snapshot(snaps[0])
    return _steps(rows, [("round", lpstate.LPRound.from_snapshot(s)) for s in snaps])


def _appends():
    """Case 3: 249 rows; + 3 rhs-only; + 2 ranged and 1 lhs-only (every rhs-sided place shifts); + 0; + 2 (R 255 -> 257: a second
    chunk).  The first append outgrows the raw buffers, which are sized exactly at open."""
    rng = np.random.default_rng(71)
    base = lpcases._make(seed=72, R=249, V=64, K=12, short_rows=False)
    rows, V = lpstate.LPRows.from_snapshot(base), 64
    cuts = _cuts_of(base)
    full = dict(col_lb=base.col_lb, col_ub=base.col_ub, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg)
    script, cur = [("round", lpstate.LPRound.from_snapshot(base))], rows
    for kinds in ((0, 0, 0), (3, 3, 1), (), (3, 0)):
        block = _row_block(rng, kinds, V, np.asarray(base.col_lp))
        script.append(("append", block))
        if kinds:
            cur = _joined(cur, block)
        script.append(("round", lpstate.LPRound(**_solve(rng, cur, V, col_lp=base.col_lp), **cuts, **(full if not kinds else {}),
                                                has_incumbent=True)))
    return _steps(rows, script)


def _none_rules():
    """Case 4: `None` keeps the last value -- col_ub flips has_ub on some columns, is then left out, then given again; the
    incumbent arrays likewise; has_incumbent goes False -> True -> False."""
    rng = np.random.default_rng(81)
    base = lpcases._make(seed=82, R=40, V=300, K=30, short_rows=False)
    rows, V, cuts = lpstate.LPRows.from_snapshot(base), 300, _cuts_of(base)
    ub2 = np.where(np.arange(V) % 3 == 0, INF, base.col_ub)
    ub3 = np.where(np.arange(V) % 5 == 0, 7.0, ub2)
    primal2 = np.where(base.col_type == 3, rng.random(V), rng.integers(0, 2, V).astype(np.float64))
    mk = lambda **kw: ("round", lpstate.LPRound(**_solve(rng, rows, V), **cuts, **kw))  # noqa: E731
    return _steps(rows, [
        mk(col_lb=base.col_lb, col_ub=base.col_ub, has_incumbent=False),                                    # no incumbent yet
        mk(col_ub=ub2, col_primal=base.col_primal, col_primal_avg=base.col_primal_avg),                     # has_ub flips; incumbent
        mk(has_incumbent=True),                                                                             # everything kept
        mk(col_ub=ub3, has_incumbent=False),                                                                # no incumbent again
        mk(col_primal=primal2, has_incumbent=True),                                                         # primal new, avg kept
        mk(col_lb=np.where(np.arange(V) % 7 == 0, -INF, 0.0), has_incumbent=True)])


def _big_v():
    """Case 6: 33,000 columns (past the single call's plan), 300 short rows, 40 cuts."""
    return _single(lpcases._make(seed=61, R=300, V=33000, K=40, short_rows=True))


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ROW_CASES:
        return _single(lpcases.snapshot(name))
    if name.startswith("hand:"):
        return _single(lpcases.hand_cases()[name[5:]][0])
    return {"k_sequence": _k_sequence, "appends": _appends, "none_rules": _none_rules, "big_v": _big_v}[name]()


def hand_names():
    return ["hand:" + n for n in lpcases.hand_cases()]


CPU_CASES = ROW_CASES + ("k_sequence", "appends", "none_rules")      # (big_v and the hand cases: covered by their own checks)

# ---- the restated session, with the defects an implementation can have -----------------------------------------------------------------
DEFECTS = {
    "dual_at_lp_row": "the round writes is_tight / dual at the LP row index instead of the state place",
    "free_row_counted": "a free row takes a state place",
    "global_prefix": "the global instead of the chunk-local row index behind the chunk prefix",
    "stale_cuts": "a smaller round keeps the cut rows of a larger earlier round behind its own",
    "ptr_not_shifted": "an appended block's row_ptr is not shifted by the resident entries",
    "places_not_rebuilt": "row places are not rebuilt after an append",
    "static_clobbered": "a round overwrites columns 0 and 2 of cons_feats",
    "growth_lost": "resident entries are lost in the growth copy",
    "absent_slot_read": "an absent optional array is read from the upload (zeros) instead of the resident buffer",
    "primal_without_incumbent": "a round without an incumbent still reads the kept incumbent arrays",
}
# which defects each case is chosen against
AGAINST = {"rows255": ("dual_at_lp_row", "free_row_counted"), "rows256": ("dual_at_lp_row", "free_row_counted"),
           "rows257": ("dual_at_lp_row", "free_row_counted", "global_prefix"), "rows600": ("dual_at_lp_row", "free_row_counted", "global_prefix"),
           "k_sequence": ("stale_cuts",),
           "appends": ("ptr_not_shifted", "places_not_rebuilt", "static_clobbered", "growth_lost"),
           "none_rules": ("absent_slot_read", "primal_without_incumbent")}


def _places(lhs, rhs, inf, defect=None):
    """row_place [R][2] as the rebuild records it: chunk prefix + chunk-local exclusive scan, lhs sides before rhs sides."""
    has_l, has_r = lpstate.finite(lhs, inf), lpstate.finite(rhs, inf)
    if defect == "free_row_counted":
        has_r = has_r | ~(has_l | has_r)
    n = lhs.shape[0]
    place = np.full((n, 2), -1, np.int64)
    for side, has, base in ((0, has_l, 0), (1, has_r, int(has_l.sum()))):
        pre, whole = 0, np.cumsum(has) - has
        for b in range(0, n, CHUNK):
            h = has[b:b + CHUNK]
            local = whole[b:b + CHUNK] if defect == "global_prefix" else np.cumsum(h) - h     # (the defect counts the chunks in front twice)
            place[b:b + CHUNK, side] = np.where(h, base + pre + local, -1)
            pre += int(h.sum())
    return place


def restated(steps, defect=None):
    """The state (the model's 10-tuple as fp64 / int64 arrays, cut_index) of every round of `steps`, from a session restated
    with NumPy the way the device one is built: a static constraint half + row places rebuilt per row set, a dynamic half per
    round.  Without a defect each equals `R.restate` of the assembled snapshot (the CPU test asserts that)."""
    out, rows, kept, place, prev, grown = [], None, {}, None, None, False
    for step in steps:
        if step[0] == "open":
            rows = step[1]
            place = _places(np.asarray(rows.row_lhs), np.asarray(rows.row_rhs), rows.infinity, defect)
        elif step[0] == "append":
            block = step[1]
            if not np.asarray(block[3]).shape[0]:
                continue
            if defect == "ptr_not_shifted":            # the new rows' offsets point at the first resident entries: their values
                n_new = int(np.diff(block[0]).sum())     # (the columns alias too; the values alone keep the restatement's input valid)
                block = (block[0], block[1], np.asarray(rows.row_val)[:n_new], block[3], block[4])
            if defect == "growth_lost" and not grown:   # the copy into the larger buffers drops the resident values
                rows = lpstate.LPRows(**{**rows.__dict__, "row_val": np.zeros_like(np.asarray(rows.row_val, np.float64))})
                grown = True
            rows = _joined(rows, block)
            if defect == "places_not_rebuilt":
                place = np.concatenate([place, np.full((np.asarray(block[3]).shape[0], 2), -1, np.int64)])
            else:
                place = _places(np.asarray(rows.row_lhs), np.asarray(rows.row_rhs), rows.infinity, defect)
        else:
            rnd = step[1]
            use = dict(kept)
            if defect == "absent_slot_read":
                use = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in kept.items()}
            if defect == "primal_without_incumbent" and not rnd.incumbent() and "col_primal" in kept and "col_primal_avg" in kept:
                rnd = lpstate.LPRound(**{**rnd.__dict__, "has_incumbent": True, "col_primal": None, "col_primal_avg": None})
            ref = R.restate(lpstate.assemble(rows, rnd, use))
            inputs = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in ref["inputs"]]
            cons = inputs[0]
            # the static half is the rebuild's; the round places is_tight and dual through row_place
            was = cons.copy()
            true_place = _places(np.asarray(rows.row_lhs), np.asarray(rows.row_rhs), rows.infinity)
            cons[:] = 0.0
            for side in (0, 1):
                src = true_place[:, side]
                for cols, dst in (((0, 2), place[:, side]), ((1, 3), np.arange(src.shape[0]) if defect == "dual_at_lp_row" else place[:, side])):
                    ok = (src >= 0) & (dst >= 0) & (dst < cons.shape[0])
                    for c in cols:
                        cons[dst[ok], c] = was[src[ok], c]
            if defect == "static_clobbered":
                cons[:, [0, 2]] = 0.0
            index = ref["cut_index"]
            if defect == "stale_cuts" and prev is not None and prev[4].shape[0] > inputs[4].shape[0]:
                inputs[4] = np.concatenate([inputs[4], prev[4][inputs[4].shape[0]:]])
            for name in lpstate.OPTIONAL:
                if getattr(step[1], name) is not None and not (name.startswith("col_primal") and not step[1].incumbent()):
                    kept[name] = getattr(step[1], name)
            prev = inputs
            out.append((tuple(inputs), index))
    return out


def same_state(a, b):
    return all((np.asarray(x).shape == np.asarray(y).shape and np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True))
               if isinstance(x, np.ndarray) else x == y for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])
