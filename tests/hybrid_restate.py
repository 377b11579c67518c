"""NumPy float64 restatement of the hybrid cut selection from cut rows (include/gcnn_hip.h: gcnn_hybrid_select), written from the
semantics listed there.  A checker, not a product path: the library computes all of this on the device (csrc/k_hybrid.hpp).

`restate(snap)` returns the three features and the quality in the association the reference's line has under Python's evaluation,
    quality = (efficacy + (0.1 * nint) / nnz) + 0.1 * parallelism,
every operation a NumPy float64 operation of its own, plus what a comparison needs to be derived rather than measured:
  bounds   per element, how far a float64 evaluation that adds the same terms in another order may land from this one, in the
           manner of `lpstate_restate.restate`: a sum of n terms carries n * 2^-52 * sum|terms|, a norm of n squares a relative
           (n + 2) * 2^-52, |col_obj| (V + 2) * 2^-52, every further operation 2^-52 relative.  Where every sum is exact (the
           dyadic cases of hybridcases.py) the device must give these very bits.
  rows     the filter's rows, cut_val / norm rounded to float32, as dense float64 [K, V] (what `cutsel_restate.dense_rows` builds).
`select` is the selection with a float64 key (`cutsel_restate.select` narrows its scores to float32).

Variants, for the host proofs of tests/test_hybridcases.py -- each must fail a planted case:
  quality_fused          the last step as one fused multiply-add (exact arithmetic via `fractions`, rounded once)
  quality_other_assoc    0.1 * (nint / nnz) in place of (0.1 * nint) / nnz
  select(key=np.float32) float32 keys, the threshold taken as float32(0.9 * float64(q0)) as `cutsel_restate.threshold` does
  select(tie_rank=...)   ties in another order than input order (the LP path's state order: lhs-sided cuts first)"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from gcnn_cut_selector_amd import lpstate

U = 2.0 ** -52


def _row_ids(ptr):
    return np.repeat(np.arange(ptr.shape[0] - 1), np.diff(ptr))


def _row_sum(ptr, terms):
    return np.bincount(_row_ids(ptr), weights=terms, minlength=ptr.shape[0] - 1).astype(np.float64)


def quality_of(eff, nint, nnz, par):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (eff + (0.1 * nint) / nnz) + 0.1 * par


def quality_other_assoc(eff, nint, nnz, par):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (eff + 0.1 * (nint / nnz)) + 0.1 * par


def quality_fused(eff, nint, nnz, par):
    """x + 0.1 * p with the product kept exact and the sum rounded once: what a fused multiply-add gives."""
    with np.errstate(invalid="ignore", divide="ignore"):
        x = eff + (0.1 * nint) / nnz
    out = np.empty_like(x)
    for i, (a, p) in enumerate(zip(x, par)):
        out[i] = float(Fraction(float(a)) + Fraction(0.1) * Fraction(float(p))) if np.isfinite(a) and np.isfinite(p) else a + 0.1 * p
    return out


def restate(snap):
    arrays, dims = lpstate.check_cut_snapshot(snap, deep=True)
    cut_ptr, cut_col, cut_val, cut_lhs, cut_rhs, col_type, col_obj, col_lp = arrays
    inf = dims["infinity"]
    V, K = dims["n_cols"], dims["n_cuts"]
    n_k = np.diff(cut_ptr).astype(np.float64)
    kid = _row_ids(cut_ptr)
    raw = np.sqrt(_row_sum(cut_ptr, cut_val * cut_val))
    norm = np.where(raw == 0, 1.0, raw)
    act = _row_sum(cut_ptr, cut_val * col_lp[cut_col])
    act_b = n_k * U * _row_sum(cut_ptr, np.abs(cut_val * col_lp[cut_col]))
    dob = _row_sum(cut_ptr, cut_val * col_obj[cut_col])
    dob_b = n_k * U * _row_sum(cut_ptr, np.abs(cut_val * col_obj[cut_col]))
    nint = np.bincount(kid, weights=(col_type[cut_col] != 3).astype(np.float64), minlength=K)
    rel_k, rel_v = (n_k + 2) * U, (V + 2) * U
    feas = np.minimum(cut_rhs - act, act - cut_lhs)
    eff = -feas / norm
    eff_b = act_b / norm + np.abs(eff) * rel_k + 4 * U * np.abs(eff)
    with np.errstate(invalid="ignore", divide="ignore"):
        isup = nint / n_k
    objn = float(np.sqrt(np.sum(col_obj * col_obj)))
    prod = raw * objn
    with np.errstate(invalid="ignore", divide="ignore"):
        par = np.where(prod == 0, 0.0, np.abs(dob) / prod)
        par_b = np.where(prod == 0, 0.0, dob_b / prod + par * (rel_k + rel_v + 4 * U))
    quality = quality_of(eff, nint, n_k, par)
    quality_b = eff_b + 0.1 * par_b + 4 * U * (np.abs(eff) + 0.1 * isup + 0.1 * par)
    lhs_fin = lpstate.finite(cut_lhs, inf)
    with np.errstate(invalid="ignore"):
        side_l = lhs_fin & ((cut_lhs - act) > (act - cut_rhs))        # the LP path's state order: these cuts first
    state_rank = np.empty(K, np.int64)
    state_rank[np.concatenate([np.flatnonzero(side_l), np.flatnonzero(~side_l)])] = np.arange(K)
    row32 = (cut_val / norm[kid]).astype(np.float32)
    dense = np.zeros((K, V), np.float64)
    dense[kid, cut_col] = row32.astype(np.float64)
    return dict(features=np.stack([eff, isup, par], 1), bounds=np.stack([eff_b, np.zeros(K), par_b], 1), quality=quality,
                quality_bound=quality_b, nint=nint, nnz=n_k, rows=dense, row32=row32, norm=norm, state_rank=state_rank, dims=dims)


def ranking(q, tie_rank=None):
    """Descending stable ranking, NaN as -inf, ties in input order (or by `tie_rank`)."""
    key = np.where(np.isnan(q), -np.inf, q)
    if tie_rank is None:
        return np.argsort(-key.astype(np.float64), kind="stable").astype(np.int64)
    return np.lexsort((tie_rank, -key.astype(np.float64))).astype(np.int64)


def select(q, cut_dense, forced_dense=None, p_max=0.1, p_max_ub=0.5, key=np.float64, tie_rank=None, record=None):
    """-> (order int32 [K], n_kept): `cutsel_restate.select` with the key type as a parameter.  key=np.float64: the threshold is
    0.9 * Q[0] and the comparison is in float64.  `record` receives 'P' (every parallelism consulted), 'Q' and 't'."""
    q = np.asarray(q, np.float64).astype(key)
    K = q.size
    order = ranking(q, tie_rank)
    if K == 0:
        if record is not None:
            record.update(P=np.zeros(0), Q=q, t=key(np.nan))
        return order.astype(np.int32), 0
    if forced_dense is None:
        forced_dense = np.zeros((0, cut_dense.shape[1]))
    P_cc, P_fc = np.abs(cut_dense @ cut_dense.T), np.abs(forced_dense @ cut_dense.T)
    Q = q[order]
    t = key(0.9 * float(Q[0]))
    with np.errstate(invalid="ignore"):
        low = Q < t
    consulted = []

    def move(rm):
        nonlocal order
        order = np.concatenate([order[~rm], order[rm]])
        return int(rm.sum())

    n = K
    for r in range(P_fc.shape[0]):
        P = P_fc[r, order[:n]]
        consulted.append(P)
        rm = np.zeros(K, bool)
        rm[:n] = (P > p_max) & (low[:n] | (P > p_max_ub))
        n -= move(rm)
    i = 0
    while i < n - 1:
        P = P_cc[order[i], order[i + 1:n]]
        consulted.append(P)
        rm = np.zeros(K, bool)
        rm[i + 1:n] = (P > p_max) & (low[i + 1:n] | (P > p_max_ub))
        n -= move(rm)
        i += 1
    if record is not None:
        record.update(P=np.concatenate(consulted) if consulted else np.zeros(0), Q=Q, t=t, order=order.copy())
    return order.astype(np.int32), n


def margins(ref, record, p_max, p_max_ub):
    """The three distances that decide whether the integers of a selection may be compared with `==`: the smallest gap between
    adjacent ranked qualities net of both bounds, the smallest distance of a quality from the threshold net of its bound and the
    threshold's, and the smallest distance of a consulted non-zero parallelism from either threshold."""
    rank = ranking(ref["quality"])
    Q, B = ref["quality"][rank], ref["quality_bound"][rank]
    gap = np.inf if Q.size < 2 else float(np.min((Q[:-1] - Q[1:]) - (B[:-1] + B[1:])))
    t = 0.9 * Q[0] if Q.size else np.nan
    thr = np.inf if not Q.size else float(np.min(np.abs(Q - t) - (B + 0.9 * B[0] + U * abs(t))))
    P = record["P"][record["P"] != 0.0]
    par = np.inf if not P.size else float(min(np.abs(P - p_max).min(), np.abs(P - p_max_ub).min()))
    return gap, thr, par
