"""A raw LP snapshot as the input of the cut scorer: what a solver binding fills in instead of re-implementing get_state.

`LPSnapshot` holds the LP rows and the candidate cuts as CSR over LP column positions plus per-row, per-column and per-cut vectors
in the solver's own float64 (include/gcnn_hip.h: gcnn_lp_state).  This module is the host side only -- the checks, the five sizes
the entry points need on the host, and the packer of the one upload; the arithmetic that turns a snapshot into the model's ten
inputs runs on the device (csrc/k_lpstate.hpp) behind `GCNN.state_from_lp`, `GCNN.score_lp` and `GCNN.select_cuts_lp`.
It imports NumPy only (the library binding is loaded inside `lp_layout`), so the scoring server's torch-free clients use it too."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

# the packed order: GCNN_LP_* of include/gcnn_hip.h (index 0 is the reserved header)
FIELDS = (("row_ptr", np.int32), ("row_col", np.int32), ("row_val", np.float64), ("row_lhs", np.float64), ("row_rhs", np.float64),
          ("row_dual", np.float64), ("row_basis", np.int8), ("col_type", np.int8), ("col_obj", np.float64), ("col_lb", np.float64),
          ("col_ub", np.float64), ("col_basis", np.int8), ("col_lp", np.float64), ("col_redcost", np.float64),
          ("col_primal", np.float64), ("col_primal_avg", np.float64), ("cut_ptr", np.int32), ("cut_col", np.int32),
          ("cut_val", np.float64), ("cut_lhs", np.float64), ("cut_rhs", np.float64))
BASIS_LOWER, BASIS_BASIC, BASIS_UPPER, BASIS_ZERO = 0, 1, 2, 3
TYPE_BINARY, TYPE_INTEGER, TYPE_IMPLINT, TYPE_CONTINUOUS = 0, 1, 2, 3
FLAG_TEXT = ("a column position outside [0, n_cols)", "columns of a row or cut are not strictly increasing",
             "row_ptr / cut_ptr is not monotone inside [0, nnz]", "the state's sizes differ from the host's count")


@dataclass
class LPSnapshot:
    """Host arrays: values float64, indices int32, codes int8 (other dtypes are cast while packing).
    rows: CSR `row_ptr [R+1]`, `row_col` (LP column positions), `row_val`; `row_lhs`, `row_rhs`, `row_dual`; `row_basis` with
    0 lower, 1 basic, 2 upper, 3 zero.  columns: `col_type` (0 binary, 1 integer, 2 implicit integer, 3 continuous), `col_obj`,
    `col_lb`, `col_ub`, `col_basis`, `col_lp`, `col_redcost`; with an incumbent also `col_primal` and `col_primal_avg`.
    cuts: CSR `cut_ptr`, `cut_col`, `cut_val`; `cut_lhs`, `cut_rhs`.
    Within a row or cut the columns are strictly increasing, every cut has an entry, constants are already in lhs / rhs.
    `obj_norm` None: the norm of `col_obj`; a value <= 0 counts as 1.  `n_model_vars` None: the number of columns.
    `has_incumbent` None: whether `col_primal` is given."""
    row_ptr: np.ndarray
    row_col: np.ndarray
    row_val: np.ndarray
    row_lhs: np.ndarray
    row_rhs: np.ndarray
    row_dual: np.ndarray
    row_basis: np.ndarray
    col_type: np.ndarray
    col_obj: np.ndarray
    col_lb: np.ndarray
    col_ub: np.ndarray
    col_basis: np.ndarray
    col_lp: np.ndarray
    col_redcost: np.ndarray
    cut_ptr: np.ndarray
    cut_col: np.ndarray
    cut_val: np.ndarray
    cut_lhs: np.ndarray
    cut_rhs: np.ndarray
    col_primal: np.ndarray | None = None
    col_primal_avg: np.ndarray | None = None
    infinity: float = 1e20
    sum_epsilon: float = 1e-6
    n_model_vars: int | None = None
    obj_norm: float | None = None
    has_incumbent: bool | None = None

    def scalars(self):
        """(infinity, sum_epsilon, n_model_vars, obj_norm, has_incumbent) with the defaults filled in."""
        inc = self.col_primal is not None if self.has_incumbent is None else bool(self.has_incumbent)
        norm = float(np.linalg.norm(np.asarray(self.col_obj, np.float64))) if self.obj_norm is None else float(self.obj_norm)
        nmv = int(np.asarray(self.col_type).shape[0]) if self.n_model_vars is None else int(self.n_model_vars)
        return float(self.infinity), float(self.sum_epsilon), nmv, (1.0 if norm <= 0 else norm), inc


def finite(x, infinity):
    """The snapshot's notion of a finite side or bound: not |x| >= infinity."""
    return ~(np.abs(x) >= infinity)


def _check_csr(name, ptr, col, val, n, n_cols, deep):
    if ptr.ndim != 1 or ptr.shape[0] != n + 1:
        raise ValueError(f"{name}_ptr must hold {n + 1} offsets, got shape {tuple(ptr.shape)}")
    if col.ndim != 1 or val.ndim != 1 or col.shape != val.shape:
        raise ValueError(f"{name}_col and {name}_val must be vectors of one length")
    nnz = col.shape[0]
    if ptr[0] != 0 or ptr[-1] != nnz or (n and np.any(ptr[1:] < ptr[:-1])):
        raise ValueError(f"{name}_ptr must rise from 0 to the {nnz} entries of {name}_col")
    if deep and nnz:
        if int(col.min()) < 0 or int(col.max()) >= n_cols:
            raise ValueError(f"{name}_col: a column position outside [0, {n_cols})")
        inner = np.ones(nnz, bool)
        inner[ptr[:-1][ptr[:-1] < nnz]] = False            # the first entry of a row has no predecessor in it
        if np.any((col[1:] <= col[:-1]) & inner[1:]):
            raise ValueError(f"{name}_col: columns within a {name} must be strictly increasing")
    return nnz


def check_snapshot(snap: LPSnapshot, deep: bool = True):
    """Validate a snapshot on the host -> (the 21 arrays in packed order with their packed dtypes, dims) where dims is the dict
    of `_lib.LpDims` fields, the state's sizes C and E1 included (the size computation: masks and sums over `row_ptr`, O(R)).
    Always: shapes, codes, offsets, no empty cut, representable sizes.  `deep`: also the O(nnz) facts -- columns in range and
    strictly increasing; without it the device finds those and the call raises after the download."""
    arrays = []
    for name, dt in FIELDS:
        a = getattr(snap, name)
        a = np.zeros(0, dt) if a is None else np.asarray(a)
        if a.dtype != dt:
            if dt != np.float64 and a.size and a.dtype.kind in "iu" and (int(a.max()) > np.iinfo(dt).max or int(a.min()) < np.iinfo(dt).min):
                raise ValueError(f"{name}: a value does not fit {np.dtype(dt).name}")
            a = a.astype(dt)
        arrays.append(np.ascontiguousarray(a))
    (row_ptr, row_col, row_val, row_lhs, row_rhs, row_dual, row_basis, col_type, col_obj, col_lb, col_ub, col_basis, col_lp,
     col_redcost, col_primal, col_avg, cut_ptr, cut_col, cut_val, cut_lhs, cut_rhs) = arrays
    infinity, eps, nmv, obj_norm, inc = snap.scalars()
    if not (infinity > 0 and eps > 0 and np.isfinite(obj_norm)) or nmv < 1:
        raise ValueError("infinity and sum_epsilon must be positive, obj_norm finite, n_model_vars at least 1")
    R, V, K = row_lhs.shape[0], col_type.shape[0], cut_lhs.shape[0]
    for name, a, n in (("row_rhs", row_rhs, R), ("row_dual", row_dual, R), ("row_basis", row_basis, R), ("col_obj", col_obj, V),
                       ("col_lb", col_lb, V), ("col_ub", col_ub, V), ("col_basis", col_basis, V), ("col_lp", col_lp, V),
                       ("col_redcost", col_redcost, V), ("cut_rhs", cut_rhs, K), ("col_primal", col_primal, V if inc else 0),
                       ("col_primal_avg", col_avg, V if inc else 0)):
        if name.startswith("col_primal") and not inc:
            continue
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"{name} must be a vector of {n} values, got shape {tuple(a.shape)}")
    for name, a in (("row_basis", row_basis), ("col_basis", col_basis), ("col_type", col_type)):
        if a.size and (int(a.min()) < 0 or int(a.max()) > 3):
            raise ValueError(f"{name}: codes are 0..3")
    nnz_r = _check_csr("row", row_ptr, row_col, row_val, R, V, deep)
    nnz_k = _check_csr("cut", cut_ptr, cut_col, cut_val, K, V, deep)
    if K and np.any(cut_ptr[1:] == cut_ptr[:-1]):
        raise ValueError("every cut must have at least one entry")
    if not inc:
        arrays[14] = arrays[15] = np.zeros(0, np.float64)
    lens = np.diff(row_ptr)
    has_lhs, has_rhs = finite(row_lhs, infinity), finite(row_rhs, infinity)
    C = int(has_lhs.sum()) + int(has_rhs.sum())
    E1 = int(lens[has_lhs].sum(dtype=np.int64)) + int(lens[has_rhs].sum(dtype=np.int64))
    if E1 > 2 ** 31 - 1:
        raise ValueError("the state's constraint edges do not fit int32")
    dims = dict(n_rows=R, n_cols=V, n_cuts=K, row_nnz=nnz_r, cut_nnz=nnz_k, has_incumbent=int(inc), n_model_vars=nmv,
                n_state_rows=C, n_state_edges=E1, reserved=0, infinity=infinity, sum_epsilon=eps, obj_norm=obj_norm)
    return arrays, dims


# ---- the cuts alone: what the hybrid selection reads (hybrid.py, csrc/k_hybrid.hpp) ------------------------------------------------
CUT_FIELDS = (("cut_ptr", np.int32), ("cut_col", np.int32), ("cut_val", np.float64), ("cut_lhs", np.float64), ("cut_rhs", np.float64),
              ("col_type", np.int8), ("col_obj", np.float64), ("col_lp", np.float64))      # GCNN_HYBRID_* order


@dataclass
class CutSnapshot:
    """The eight arrays of an `LPSnapshot` that SCIP's hybrid cut quality and the parallelism filter need, under the same contract:
    the cuts as CSR over LP column positions (`cut_ptr`, `cut_col`, `cut_val`, `cut_lhs`, `cut_rhs`; columns strictly increasing
    within a cut, every cut has an entry, constants already in lhs / rhs) and per column `col_type`, `col_obj`, `col_lp`.
    An `LPSnapshot` is accepted wherever a `CutSnapshot` is."""
    cut_ptr: np.ndarray
    cut_col: np.ndarray
    cut_val: np.ndarray
    cut_lhs: np.ndarray
    cut_rhs: np.ndarray
    col_type: np.ndarray
    col_obj: np.ndarray
    col_lp: np.ndarray
    infinity: float = 1e20


def check_cut_snapshot(snap, deep: bool = True):
    """`check_snapshot` for the fields of a `CutSnapshot` (or of an `LPSnapshot`: its other fields are not looked at) -> (the
    eight arrays in packed order with their packed dtypes, dims) where dims is the dict of `_lib.HybridDims` fields."""
    arrays = []
    for name, dt in CUT_FIELDS:
        a = np.asarray(getattr(snap, name))
        if a.dtype != dt:
            if dt != np.float64 and a.size and a.dtype.kind in "iu" and (int(a.max()) > np.iinfo(dt).max or int(a.min()) < np.iinfo(dt).min):
                raise ValueError(f"{name}: a value does not fit {np.dtype(dt).name}")
            a = a.astype(dt)
        arrays.append(np.ascontiguousarray(a))
    cut_ptr, cut_col, cut_val, cut_lhs, cut_rhs, col_type, col_obj, col_lp = arrays
    infinity = float(snap.infinity)
    if not infinity > 0:
        raise ValueError("infinity must be positive")
    V, K = col_type.shape[0], cut_lhs.shape[0]
    for name, a, n in (("cut_lhs", cut_lhs, K), ("cut_rhs", cut_rhs, K), ("col_type", col_type, V), ("col_obj", col_obj, V), ("col_lp", col_lp, V)):
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"{name} must be a vector of {n} values, got shape {tuple(a.shape)}")
    if col_type.size and (int(col_type.min()) < 0 or int(col_type.max()) > 3):
        raise ValueError("col_type: codes are 0..3")
    nnz = _check_csr("cut", cut_ptr, cut_col, cut_val, K, V, deep)
    if K and np.any(cut_ptr[1:] == cut_ptr[:-1]):
        raise ValueError("every cut must have at least one entry")
    return arrays, dict(n_cols=V, n_cuts=K, cut_nnz=nnz, reserved=0, infinity=infinity)


def state_key(dims):
    """(n_cons, n_vars, n_cuts, E1, E2) of the state a snapshot of these dims builds."""
    return dims["n_state_rows"], dims["n_cols"], dims["n_cuts"], dims["n_state_edges"], dims["cut_nnz"]


def pack_snapshot(buf, snap_off, arrays):
    """Write the checked arrays into a staging buffer (`buf`: writable uint8 array) at the library's offsets (the reserved header is zeroed)."""
    buf[snap_off[0]:snap_off[0] + 16] = 0
    for off, a in zip(snap_off[1:], arrays):
        if a.size:
            buf[off:off + a.nbytes] = a.view(np.uint8)


def raise_for_flags(flags):
    """The four LP flag words of a download -> ValueError naming the first violation."""
    for f, text in zip(flags, FLAG_TEXT):
        if f:
            raise ValueError(f"LP snapshot rejected by the device: {text}")


# ---- an LP that stays on the device across separation rounds (GCNN.open_lp, csrc/k_lpres.hpp) ------------------------------------------
ROW_FIELDS = FIELDS[:5] + FIELDS[7:9]        # what stays: the rows, col_type, col_obj
OPTIONAL = ("col_lb", "col_ub", "col_primal", "col_primal_avg")      # bit q of a round's presence mask (GCNN_LPR_*)
ROUND_FIELDS = (("row_dual", np.float64), ("row_basis", np.int8), ("col_basis", np.int8), ("col_lp", np.float64),
                ("col_redcost", np.float64), ("col_lb", np.float64), ("col_ub", np.float64), ("col_primal", np.float64),
                ("col_primal_avg", np.float64)) + FIELDS[16:]          # the packed order behind the header (gcnn_lp_round)


@dataclass
class LPRows:
    """The part of an `LPSnapshot` that does not change between the separation rounds of one LP: the rows, `col_type`, `col_obj`
    and the scalars (defaults as `LPSnapshot`'s)."""
    row_ptr: np.ndarray
    row_col: np.ndarray
    row_val: np.ndarray
    row_lhs: np.ndarray
    row_rhs: np.ndarray
    col_type: np.ndarray
    col_obj: np.ndarray
    infinity: float = 1e20
    sum_epsilon: float = 1e-6
    n_model_vars: int | None = None
    obj_norm: float | None = None

    @classmethod
    def from_snapshot(cls, snap):
        return cls(**{name: getattr(snap, name) for name, _ in ROW_FIELDS}, infinity=snap.infinity, sum_epsilon=snap.sum_epsilon,
                   n_model_vars=snap.n_model_vars, obj_norm=snap.obj_norm)

    def scalars(self):
        """(infinity, sum_epsilon, n_model_vars, obj_norm) with the defaults filled in as `LPSnapshot.scalars` fills them."""
        norm = float(np.linalg.norm(np.asarray(self.col_obj, np.float64))) if self.obj_norm is None else float(self.obj_norm)
        nmv = int(np.asarray(self.col_type).shape[0]) if self.n_model_vars is None else int(self.n_model_vars)
        return float(self.infinity), float(self.sum_epsilon), nmv, (1.0 if norm <= 0 else norm)


@dataclass
class LPRound:
    """What one separation round adds to an `LPRows`: the solve (`row_dual`, `row_basis`, `col_basis`, `col_lp`, `col_redcost`, the
    bounds) and the candidate cuts.  In a round after the first `col_lb`, `col_ub`, `col_primal` and `col_primal_avg` may each be
    None: unchanged since the last round that gave it.  `has_incumbent` None: whether `col_primal` is given -- so a round that
    keeps the last incumbent arrays says `has_incumbent=True`; without an incumbent the two arrays are not looked at."""
    row_dual: np.ndarray
    row_basis: np.ndarray
    col_basis: np.ndarray
    col_lp: np.ndarray
    col_redcost: np.ndarray
    cut_ptr: np.ndarray
    cut_col: np.ndarray
    cut_val: np.ndarray
    cut_lhs: np.ndarray
    cut_rhs: np.ndarray
    col_lb: np.ndarray | None = None
    col_ub: np.ndarray | None = None
    col_primal: np.ndarray | None = None
    col_primal_avg: np.ndarray | None = None
    has_incumbent: bool | None = None

    @classmethod
    def from_snapshot(cls, snap):
        return cls(**{name: getattr(snap, name) for name, _ in ROUND_FIELDS}, has_incumbent=snap.has_incumbent)

    def incumbent(self):
        return self.col_primal is not None if self.has_incumbent is None else bool(self.has_incumbent)


@dataclass
class LPRowBlock:
    """Rows to append behind the resident ones of an `LPSession`: CSR over the same columns with `row_ptr` from 0, under the
    rows' contract of `LPSnapshot` (checked by `check_row_block`)."""
    row_ptr: np.ndarray
    row_col: np.ndarray
    row_val: np.ndarray
    row_lhs: np.ndarray
    row_rhs: np.ndarray

    def arrays(self):
        return self.row_ptr, self.row_col, self.row_val, self.row_lhs, self.row_rhs


def rows_with(rows: LPRows, *blocks: LPRowBlock) -> LPRows:
    """`rows` with the blocks appended: what a session holds after appending them."""
    ptr, col, val, lhs, rhs = ([np.asarray(getattr(rows, n))] for n in ("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs"))
    at = int(ptr[0][-1])
    for b in blocks:
        bp = np.asarray(b.row_ptr)
        ptr.append(bp[1:].astype(np.int64) + at)
        at += int(bp[-1])
        for dst, a in zip((col, val, lhs, rhs), (b.row_col, b.row_val, b.row_lhs, b.row_rhs)):
            dst.append(np.asarray(a))
    return LPRows(np.concatenate(ptr).astype(np.int32), np.concatenate(col).astype(np.int32), np.concatenate(val).astype(np.float64),
                  np.concatenate(lhs).astype(np.float64), np.concatenate(rhs).astype(np.float64), rows.col_type, rows.col_obj,
                  infinity=rows.infinity, sum_epsilon=rows.sum_epsilon, n_model_vars=rows.n_model_vars, obj_norm=rows.obj_norm)


def check_remove(remove, n_rows):
    """The row indices of a removal, checked against `n_rows` rows -> ascending int64 (empty for None or no index).  Any order is
    accepted; ValueError for an index that is not an integer, lies outside [0, n_rows) or is given twice."""
    if remove is None:
        return np.zeros(0, np.int64)
    a = np.asarray(remove)
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"remove: row indices must be integers, got {a.dtype}")
    a = np.sort(a.astype(np.int64).ravel())
    if a[0] < 0 or a[-1] >= n_rows:
        raise ValueError(f"remove: a row index outside [0, {n_rows})")
    if np.any(a[1:] == a[:-1]):
        raise ValueError("remove: a row index is given twice")
    return a


def _csr_without(arrays, idx):
    """The five row arrays (row_ptr from 0) without the rows `idx` (ascending, checked); the order of the kept rows unchanged."""
    ptr, col, val, lhs, rhs = (np.asarray(a) for a in arrays)
    keep = np.ones(lhs.shape[0], bool)
    keep[idx] = False
    lens = np.diff(ptr).astype(np.int64)
    entries = np.repeat(keep, lens)
    new_ptr = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int32)
    return new_ptr, col[entries], val[entries], lhs[keep], rhs[keep]


def rows_without(rows: LPRows, remove) -> LPRows:
    """`rows` without the rows at the indices `remove` (any order), the order of the kept rows unchanged: what a session holds
    after removing them."""
    idx = check_remove(remove, np.asarray(rows.row_lhs).shape[0])
    ptr, col, val, lhs, rhs = _csr_without((rows.row_ptr, rows.row_col, rows.row_val, rows.row_lhs, rows.row_rhs), idx)
    return LPRows(ptr, col.astype(np.int32), val.astype(np.float64), lhs.astype(np.float64), rhs.astype(np.float64), rows.col_type,
                  rows.col_obj, infinity=rows.infinity, sum_epsilon=rows.sum_epsilon, n_model_vars=rows.n_model_vars, obj_norm=rows.obj_norm)


def block_without(block: LPRowBlock, idx) -> LPRowBlock:
    """`block` without its rows `idx` (ascending indices into the block, checked)."""
    return LPRowBlock(*_csr_without(block.arrays(), idx))


def split_remove(remove, n_resident, block=None):
    """A removal's indices, which number the rows AFTER the append of `block` in the same call -> (the ascending indices of
    resident rows, the block without the rows the others name -- None where no row of it is left).  Empty indices: (empty,
    block).  ValueError as `check_remove`, and where the removal would leave no row at all."""
    n_block = 0 if block is None else int(np.asarray(block.row_lhs).shape[0])
    idx = check_remove(remove, n_resident + n_block)
    if idx.size and idx.size == n_resident + n_block:
        raise ValueError("remove: the removal would leave no row at all; open a new session instead")
    inside = idx[idx >= n_resident] - n_resident
    if inside.size:
        block = block_without(block, inside) if inside.size < n_block else None
    return idx[idx < n_resident], block


def row_book(arrays, infinity):
    """What a session keeps on the host per resident row to stay exact through a removal without a device read: (entry counts
    int64 [R], side bits int8 [R] -- 1: the lhs side is listed, 2: the rhs side --, a copy of row_col int32 [N])."""
    row_ptr, row_col, _, row_lhs, row_rhs = arrays
    sides = finite(row_lhs, infinity).astype(np.int8) + 2 * finite(row_rhs, infinity).astype(np.int8)
    return np.diff(row_ptr).astype(np.int64), sides, np.array(row_col, np.int32)


def removal_counts(book, col_deg, lhs, idx):
    """The host's exact account of removing the resident rows `idx` (ascending) -> (the removed rows' six counts: rows, raw
    entries, state rows, state edges, lhs state rows, lhs edges; the book without them; `col_deg` after the decrement; (lhs rows,
    lhs entries) after; (l_max_deg, v_max_deg) after: the maximum over the kept listed rows, the maximum of the new `col_deg`)."""
    lens, sides, cols = book
    keep = np.ones(lens.shape[0], bool)
    keep[idx] = False
    has_l, has_r = (sides[idx] & 1).astype(bool), (sides[idx] & 2).astype(bool)
    gone = lens[idx]
    m_lhs, m_lhs_edges = int(has_l.sum()), int(gone[has_l].sum())
    counts = (int(idx.size), int(gone.sum()), m_lhs + int(has_r.sum()), m_lhs_edges + int(gone[has_r].sum()), m_lhs, m_lhs_edges)
    weight = np.repeat(has_l.astype(np.int64) + has_r, gone)
    if idx.size <= 64:                                  # a few rows: slices between them, O(rows) + a copy of the entries
        ends = np.cumsum(lens)[idx]
        starts = ends - gone
        hit = np.concatenate([cols[a:b] for a, b in zip(starts, ends)])
        new_cols = np.concatenate([cols[a:b] for a, b in zip([0] + ends.tolist(), starts.tolist() + [cols.shape[0]])])
    else:
        entries = np.repeat(keep, lens)
        hit, new_cols = cols[~entries], cols[entries]
    ok = (hit >= 0) & (hit < col_deg.shape[0])
    deg = col_deg.copy()
    if col_deg.shape[0] <= max(8 * hit.size, 1 << 14):
        deg -= np.bincount(hit[ok], weights=weight[ok], minlength=col_deg.shape[0]).astype(np.int64)
    else:
        which, inverse = np.unique(hit[ok], return_inverse=True)
        deg[which] -= np.bincount(inverse, weights=weight[ok], minlength=which.size).astype(np.int64)
    new_book = (lens[keep], sides[keep], new_cols)
    listed = new_book[0][new_book[1] > 0]
    longest = int(listed.max()) if listed.size else 0
    return counts, new_book, deg, (lhs[0] - m_lhs, lhs[1] - m_lhs_edges), (longest, int(deg.max()) if deg.size else 0)


def lp_remove_layout(dims, removed, block, present, n_forced=-1, n_entries=0):
    """(LpDims, LpRemoveDims, LpAppendDims | None, LpRemoveLayout) of the library for the dims BEFORE the edit, the removed rows'
    eight counts and, with an append behind the removal, the block's eight counts (its resident lhs counts: after the removal);
    raises `_lib.GcnnError` where it declines the sizes."""
    import ctypes as C

    from . import _lib
    d, m, L = _lib.LpDims(**dims), _lib.LpRemoveDims(*removed), _lib.LpRemoveLayout()
    b = None if block is None else _lib.LpAppendDims(*block)
    _lib.check(_lib.lib().gcnn_lp_remove_layout_for(C.byref(d), C.byref(m), None if b is None else C.byref(b), present, n_forced, n_entries,
                                                    C.byref(L)), "gcnn_lp_remove_layout_for")
    return d, m, b, L


def assemble(rows: LPRows, rnd: LPRound, kept=None) -> LPSnapshot:
    """The `LPSnapshot` a round stands for: the definition of what a session answers.  `kept`: {name: array} of the optional column
    arrays as the last rounds gave them, for the ones this round leaves None."""
    inc = rnd.incumbent()
    opt = {}
    for name in OPTIONAL:
        a = getattr(rnd, name)
        if name.startswith("col_primal") and not inc:
            a = None
        elif a is None:
            a = (kept or {}).get(name)
            if a is None:
                raise ValueError(f"{name} is None and no earlier round gave it")
        opt[name] = a
    return LPSnapshot(**{name: getattr(rows, name) for name, _ in ROW_FIELDS},
                      **{name: getattr(rnd, name) for name, _ in ROUND_FIELDS if name not in OPTIONAL}, **opt,
                      infinity=rows.infinity, sum_epsilon=rows.sum_epsilon, n_model_vars=rows.n_model_vars, obj_norm=rows.obj_norm,
                      has_incumbent=inc)


def _cast(name, a, dt):
    """`check_snapshot`'s cast of one array to its packed dtype."""
    a = np.zeros(0, dt) if a is None else np.asarray(a)
    if a.dtype != dt:
        if dt != np.float64 and a.size and a.dtype.kind in "iu" and (int(a.max()) > np.iinfo(dt).max or int(a.min()) < np.iinfo(dt).min):
            raise ValueError(f"{name}: a value does not fit {np.dtype(dt).name}")
        a = a.astype(dt)
    return np.ascontiguousarray(a)


def _vector(name, a, n):
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError(f"{name} must be a vector of {n} values, got shape {tuple(a.shape)}")


def check_row_block(row_ptr, row_col, row_val, row_lhs, row_rhs, n_cols, infinity, deep=True):
    """The checks `check_snapshot` applies to the rows, on a block of rows (all of them at open, the new ones of an append) ->
    (the five arrays with their packed dtypes, (R, nnz, C, E1) of the block)."""
    arrays = [_cast(name, a, dt) for (name, dt), a in zip(FIELDS[:5], (row_ptr, row_col, row_val, row_lhs, row_rhs))]
    row_ptr, row_col, row_val, row_lhs, row_rhs = arrays
    if row_lhs.ndim != 1:
        raise ValueError(f"row_lhs must be a vector, got shape {tuple(row_lhs.shape)}")
    R = row_lhs.shape[0]
    _vector("row_rhs", row_rhs, R)
    nnz = _check_csr("row", row_ptr, row_col, row_val, R, n_cols, deep)
    lens = np.diff(row_ptr)
    has_lhs, has_rhs = finite(row_lhs, infinity), finite(row_rhs, infinity)
    C = int(has_lhs.sum()) + int(has_rhs.sum())
    E1 = int(lens[has_lhs].sum(dtype=np.int64)) + int(lens[has_rhs].sum(dtype=np.int64))
    return arrays, (R, nnz, C, E1)


def check_rows(rows: LPRows, deep: bool = True):
    """`check_snapshot` for the resident half -> (the seven arrays in ROW_FIELDS order, dims) where dims is the dict of
    `_lib.LpDims` fields with no cuts and no incumbent."""
    infinity, eps, nmv, obj_norm = rows.scalars()
    if not (infinity > 0 and eps > 0 and np.isfinite(obj_norm)) or nmv < 1:
        raise ValueError("infinity and sum_epsilon must be positive, obj_norm finite, n_model_vars at least 1")
    col_type, col_obj = _cast("col_type", rows.col_type, np.int8), _cast("col_obj", rows.col_obj, np.float64)
    if col_type.ndim != 1:
        raise ValueError(f"col_type must be a vector, got shape {tuple(col_type.shape)}")
    V = col_type.shape[0]
    _vector("col_obj", col_obj, V)
    if col_type.size and (int(col_type.min()) < 0 or int(col_type.max()) > 3):
        raise ValueError("col_type: codes are 0..3")
    arrays, (R, nnz, C, E1) = check_row_block(rows.row_ptr, rows.row_col, rows.row_val, rows.row_lhs, rows.row_rhs, V, infinity, deep)
    if E1 > 2 ** 31 - 1:
        raise ValueError("the state's constraint edges do not fit int32")
    dims = dict(n_rows=R, n_cols=V, n_cuts=0, row_nnz=nnz, cut_nnz=0, has_incumbent=0, n_model_vars=nmv, n_state_rows=C,
                n_state_edges=E1, reserved=0, infinity=infinity, sum_epsilon=eps, obj_norm=obj_norm)
    return arrays + [col_type, col_obj], dims


def check_round(rnd: LPRound, row_dims, have=(), deep: bool = True):
    """`check_snapshot` for a round against the resident rows' dims -> (the 14 arrays in ROUND_FIELDS order, None for an optional
    one that does not travel; the presence mask; the round's dims: `row_dims` with the cuts and the incumbent filled in).
    `have`: the optional arrays an earlier round gave -- one that is neither given nor held is a ValueError."""
    R, V = row_dims["n_rows"], row_dims["n_cols"]
    inc = rnd.incumbent()
    arrays, present = [], 0
    for name, dt in ROUND_FIELDS:
        a = getattr(rnd, name)
        if name in OPTIONAL:
            if name.startswith("col_primal") and not inc:
                arrays.append(None)
                continue
            if a is None:
                if name not in have:
                    raise ValueError(f"{name}: the first round must give it" if name in OPTIONAL[:2]
                                     else f"{name}: has_incumbent is set and no round has given it")
                arrays.append(None)
                continue
            present |= 1 << OPTIONAL.index(name)
        arrays.append(_cast(name, a, dt))
    by_name = dict(zip((n for n, _ in ROUND_FIELDS), arrays))
    K = by_name["cut_lhs"].shape[0] if by_name["cut_lhs"].ndim == 1 else -1
    if K < 0:
        raise ValueError(f"cut_lhs must be a vector, got shape {tuple(by_name['cut_lhs'].shape)}")
    for name, n in (("row_dual", R), ("row_basis", R), ("col_basis", V), ("col_lp", V), ("col_redcost", V), ("col_lb", V),
                    ("col_ub", V), ("col_primal", V), ("col_primal_avg", V), ("cut_rhs", K)):
        if by_name[name] is not None:
            _vector(name, by_name[name], n)
    for name in ("row_basis", "col_basis"):
        a = by_name[name]
        if a.size and (int(a.min()) < 0 or int(a.max()) > 3):
            raise ValueError(f"{name}: codes are 0..3")
    cut_ptr = by_name["cut_ptr"]
    nnz_k = _check_csr("cut", cut_ptr, by_name["cut_col"], by_name["cut_val"], K, V, deep)
    if K and np.any(cut_ptr[1:] == cut_ptr[:-1]):
        raise ValueError("every cut must have at least one entry")
    return arrays, present, dict(row_dims, n_cuts=K, cut_nnz=nnz_k, has_incumbent=int(inc))


def pack_round(buf, in_off, arrays, present):
    """Write a checked round into a staging buffer at gcnn_lp_round_layout_for's offsets: the header with the presence mask, then
    every array that travels."""
    buf[in_off[0]:in_off[0] + 16] = 0
    buf[in_off[0]:in_off[0] + 4].view(np.int32)[0] = present
    for off, a in zip(in_off[1:], arrays):
        if a is not None and a.size:
            buf[off:off + a.nbytes] = a.view(np.uint8)


def rows_upload_layout(n_rows, nnz, first):
    """Byte offsets of (row_ptr, row_col, row_val, row_lhs, row_rhs) in the staging buffer of a block of rows and the total.  The
    first block carries all R + 1 offsets, an appended one only the R behind the resident closing offset."""
    sizes = (4 * (n_rows + (1 if first else 0)), 4 * nnz, 8 * nnz, 8 * n_rows, 8 * n_rows)
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += (s + 15) & ~15
    return offs, at


def pack_row_block(buf, arrays, entry_base, first):
    """Write a checked block of rows into a staging buffer at `rows_upload_layout`'s offsets; its offsets are shifted by
    `entry_base`, the entries already resident.  Returns the five (offset, bytes) pairs."""
    row_ptr, row_col, row_val, row_lhs, row_rhs = arrays
    ptr = (row_ptr if first else row_ptr[1:]).astype(np.int64) + entry_base
    if ptr.size and int(ptr[-1]) > 2 ** 31 - 1:
        raise ValueError("the rows' entries do not fit int32")
    offs, _ = rows_upload_layout(row_lhs.shape[0], row_col.shape[0], first)
    out = []
    for off, a in zip(offs, (ptr.astype(np.int32), row_col, row_val, row_lhs, row_rhs)):
        if a.size:
            buf[off:off + a.nbytes] = a.view(np.uint8)
        out.append((off, a.nbytes))
    return out


def block_sides(arrays, n_cols, infinity):
    """What the host keeps of a checked block of rows beside `check_row_block`'s counts: (lhs-sided rows, their entries, the
    longest row that lists a side, per-column count of listed entries as (columns, counts)).  O(entries of the block); a block
    that is not small against the columns is counted densely, O(columns), which is cheaper then."""
    row_ptr, row_col, _, row_lhs, row_rhs = arrays
    lens = row_ptr[1:] - row_ptr[:-1]
    has_lhs, has_rhs = finite(row_lhs, infinity), finite(row_rhs, infinity)
    sides = has_lhs.view(np.int8) + has_rhs.view(np.int8)
    listed = lens[sides > 0]
    longest = int(listed.max()) if listed.size else 0
    weight = np.repeat(sides, lens)
    in_range = not row_col.size or (int(row_col.min()) >= 0 and int(row_col.max()) < n_cols)     # (without the deep check: anything)
    if in_range and n_cols <= 8 * row_col.size:
        dense = np.bincount(row_col, weights=weight, minlength=n_cols).astype(np.int64)
        cols = np.flatnonzero(dense)
        counts = dense[cols]
    else:
        cols, inverse = np.unique(row_col, return_inverse=True)
        counts = np.bincount(inverse, weights=weight, minlength=cols.size).astype(np.int64)
        ok = (cols >= 0) & (cols < n_cols) & (counts > 0)
        cols, counts = cols[ok], counts[ok]
    return int(np.count_nonzero(has_lhs)), int(lens[has_lhs].sum()), longest, (cols, counts)


def lp_append_layout(dims, block, present, n_forced=-1, n_entries=0):
    """(LpDims, LpAppendDims, LpAppendLayout) of the library for the dims BEFORE an append (a round's cut fields filled in) and
    the block's eight counts; raises `_lib.GcnnError` where it declines the sizes."""
    import ctypes as C

    from . import _lib
    d, b, L = _lib.LpDims(**dims), _lib.LpAppendDims(*block), _lib.LpAppendLayout()
    _lib.check(_lib.lib().gcnn_lp_append_layout_for(C.byref(d), C.byref(b), present, n_forced, n_entries, C.byref(L)),
               "gcnn_lp_append_layout_for")
    return d, b, L


def pack_append(buf, L, block_arrays, round_arrays, present):
    """Write a checked block and a checked round into a staging buffer at gcnn_lp_append_layout_for's offsets: the block (its
    `row_ptr` from 0, all n + 1 offsets) in front, then the round as `pack_round` writes it, at `L.block_bytes`."""
    for off, a in zip(L.block_off, block_arrays):
        if a.size:
            buf[off:off + a.nbytes] = a.view(np.uint8)
    pack_round(buf[L.block_bytes:], list(L.round.in_off), round_arrays, present)


def unpack_append(buf, L, counts, round_dims, present):
    """The inverse of `pack_append` for a block of `counts` = (rows, entries) and a round of `round_dims` (after the append) ->
    (the block's five arrays, the round's 14 arrays with None where one does not travel)."""
    n, nnz = counts
    shapes = ((n + 1, np.int32), (nnz, np.int32), (nnz, np.float64), (n, np.float64), (n, np.float64))
    block = [buf[off:off + k * np.dtype(dt).itemsize].view(dt).copy() for off, (k, dt) in zip(L.block_off, shapes)]
    R, V, K, NK = round_dims["n_rows"], round_dims["n_cols"], round_dims["n_cuts"], round_dims["cut_nnz"]
    sizes = [R, R, V, V, V] + [V if present >> q & 1 else None for q in range(4)] + [K + 1, NK, NK, K, K]
    base, rnd = L.block_bytes, []
    for off, (name, dt), k in zip(list(L.round.in_off)[1:], ROUND_FIELDS, sizes):
        rnd.append(None if k is None else buf[base + off:base + off + k * np.dtype(dt).itemsize].view(dt).copy())
    return block, rnd


def lp_round_layout(dims, present, n_forced=-1, n_entries=0):
    """(LpDims, LpRoundLayout) of the library for a round's dims; raises `_lib.GcnnError` where it declines the sizes."""
    import ctypes as C

    from . import _lib
    d, L = _lib.LpDims(**dims), _lib.LpRoundLayout()
    _lib.check(_lib.lib().gcnn_lp_round_layout_for(C.byref(d), present, n_forced, n_entries, C.byref(L)), "gcnn_lp_round_layout_for")
    return d, L


def lp_layout(dims, n_forced=-1, n_entries=0):
    """(LpDims, LpLayout) of the library for these dims."""
    import ctypes as C

    from . import _lib
    d, L = _lib.LpDims(**dims), _lib.LpLayout()
    _lib.check(_lib.lib().gcnn_lp_layout_for(C.byref(d), n_forced, n_entries, C.byref(L)), "gcnn_lp_layout_for")
    return d, L


# ---- the data collector's expert round (collect.py, csrc/gcnn_collect.hpp): what both the in-process call and the server's client use ----
class CollectResult:
    """What `collect_lp` answers for an expert round of data_collector.SamplingAgent.cutselselect (data_collector.py:101-195).
    `state`: the 10-tuple of host arrays `GCNN.state_from_lp(snapshot)` returns; `cut_index` [K] int32: state position -> input
    cut; `improvements` = quality[cut_index], float64: the labels ALIGNED with `state` -- what a sample writer stores
    (`utils.save_sample(path, utils.inputs_to_state(res.state), res.improvements)`).
    `order` [K] int32 (kept cuts first, best first, then the removed ones), `n_kept`, `n_selected` = min(n_kept, max_selected):
    the plugin's ranking and parallelism filter over `quality`, in INPUT cut indices.
    `hybrid_quality` [K] float64 and `features` [K, 3] float64 (efficacy, integer support, objective parallelism), input cut
    order: the plugin's fallback ranking (data_collector.py:145-148) without a second call."""

    def __init__(self, state, cut_index, improvements, order, n_kept, n_selected, hybrid_quality, features):
        self.state, self.cut_index, self.improvements = state, cut_index, improvements
        self.order, self.n_kept, self.n_selected = order, n_kept, n_selected
        self.hybrid_quality, self.features = hybrid_quality, features

    def __repr__(self):
        return f"CollectResult(n_cuts={self.order.shape[0]}, n_kept={self.n_kept}, n_selected={self.n_selected})"


def check_quality(quality, n_cuts):
    """The expert's quality of an expert round -> a contiguous float64 vector of `n_cuts` finite values, or ValueError.  Integer and
    float arrays are accepted (cast to float64); anything else, a wrong length or a value that is not finite is refused: the
    reference records a sample only when every dive solved (data_collector.py:119-133), so -inf and NaN never belong to one."""
    q = np.asarray(quality)
    if q.dtype.kind not in "fiu":
        raise ValueError(f"quality must be a float64 vector, got dtype {q.dtype}")
    if q.ndim != 1 or q.shape[0] != n_cuts:
        raise ValueError(f"quality must hold one value per cut ({n_cuts}), got shape {tuple(q.shape)}")
    q = np.ascontiguousarray(q, dtype=np.float64)
    if not np.isfinite(q).all():
        raise ValueError("quality: every value must be finite (a round with an unsolved dive is not recorded)")
    return q
