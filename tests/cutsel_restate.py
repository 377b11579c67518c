"""NumPy restatement of the cut selection (the parallelism filter of the SCIP plugin's cutselselect, model_evaluator.py:109-154),
written from the semantics in include/gcnn_hip.h, in state order.  Dense fp64 rows, P = |A B^T|, the threshold computed explicitly.

Threshold: the reference pins NumPy 1.22.  There `0.9 * quality[0]` multiplies a Python float by a float32 SCALAR, and with scalars
only the ordinary promotion applies: the product is a float64.  `quality < that` compares a float32 ARRAY with a float64 scalar of
the same kind, so value-based casting keeps the array's float32 and rounds the scalar: t = float32(0.9 * float64(Q[0])), compared
in float32.  (NumPy >= 2 would round 0.9 to float32 first and multiply in float32.)  This is the form implemented."""
from __future__ import annotations

import numpy as np


def dense_rows(rows, cols, vals, n_rows, n_vars):
    """Edge list -> dense fp64 [n_rows, n_vars]; duplicate (row, col) entries add."""
    a = np.zeros((n_rows, n_vars), np.float64)
    np.add.at(a, (np.asarray(rows, np.int64), np.asarray(cols, np.int64)), np.asarray(vals, np.float32).astype(np.float64))
    return a


def ranking(q):
    """Descending stable ranking, NaN as -inf (what k_rank_scores / score_state's rankings give)."""
    key = np.where(np.isnan(q), -np.inf, q).astype(np.float64)
    return np.argsort(-key, kind="stable").astype(np.int64)


def threshold(q0):
    return np.float32(0.9 * float(np.float32(q0)))


def select(q, cut_dense, forced_dense=None, p_max=0.1, p_max_ub=0.5, record=None, P=None):
    """-> (order int32 [K], n_kept).  `record` (optional dict) receives 'P' (every parallelism the filter consulted), 'Q' and 't'.
    `P` (optional): the precomputed (|A A^T|, |B A^T|) -- the dense rows are then not read."""
    q = np.asarray(q, np.float32)
    K = q.size
    if forced_dense is None and P is None:
        forced_dense = np.zeros((0, cut_dense.shape[1]))
    order = ranking(q)
    if K == 0:
        if record is not None:
            record.update(P=np.zeros(0), Q=q, t=np.float32(np.nan))
        return order.astype(np.int32), 0
    P_cc, P_fc = P if P is not None else (np.abs(cut_dense @ cut_dense.T), np.abs(forced_dense @ cut_dense.T))
    Q = q[order]                      # fixed by position
    t = threshold(Q[0])
    low = Q < t                       # float32 comparison
    consulted = []

    def move(rm):
        nonlocal order
        rm = np.asarray(rm, bool)
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
        record.update(P=np.concatenate(consulted) if consulted else np.zeros(0), Q=Q, t=t)
    return order.astype(np.int32), n


def margins_ok(record, p_max, p_max_ub, eps=1e-9):
    """True when no consulted P lies within eps of a threshold and no finite Q within one float32 ulp of t: the only places where
    a restatement and the device may legitimately disagree.  A P of exactly 0 (rows without a common column) is 0 on every path."""
    P, Q, t = record["P"], record["Q"], record["t"]
    P = P[P != 0.0]
    if P.size and (np.abs(P - p_max).min() <= eps or np.abs(P - p_max_ub).min() <= eps):
        return False
    if np.isfinite(t):
        fin = Q[np.isfinite(Q)]
        if fin.size and np.abs(fin.astype(np.float64) - np.float64(t)).min() <= np.float64(np.spacing(np.abs(t))):
            return False
    return True
