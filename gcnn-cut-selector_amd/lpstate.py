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


def lp_layout(dims, n_forced=-1, n_entries=0):
    """(LpDims, LpLayout) of the library for these dims."""
    import ctypes as C

    from . import _lib
    d, L = _lib.LpDims(**dims), _lib.LpLayout()
    _lib.check(_lib.lib().gcnn_lp_layout_for(C.byref(d), n_forced, n_entries, C.byref(L)), "gcnn_lp_layout_for")
    return d, L
