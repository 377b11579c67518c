"""Thin torch-facing wrappers over the per-op C ABI (include/gcnn_hip.h).  Each wrapper only checks shapes, allocates
outputs and forwards device pointers; all arithmetic is in libgcnn_hip.so.  These are the unfused building blocks of
`PartialGraphConvolution.call` (/root/reference/model.py:533-575) and double as the unit-test surface."""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .graph import BipartiteGraph, _ptr, _stream

EMB = 64


def _chk(t, shape_tail=(EMB,), dtype=torch.float32, name="tensor"):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name}: expected contiguous {dtype} device tensor [N,{','.join(map(str, shape_tail))}], "
                         f"got {t.dtype} {tuple(t.shape)} cuda={t.is_cuda}")


def linear_fwd(xa, wa, bias=None, relu=False, xb=None, wb=None, sa=None, bd=None, seg_ptr=None):
    """y = act((sa*xa) @ wa [+ xb @ wb] [+ bias] [+ deg (x) bd]) on the fp32 MFMA (gcnn_linear_fwd)."""
    _chk(xa, name="xa"); _chk(xb, name="xb")
    y = torch.empty_like(xa)
    with torch.cuda.device(xa.device):
        _lib.check(_lib.lib().gcnn_linear_fwd(_ptr(xa), _ptr(sa), _ptr(wa), _ptr(xb), _ptr(wb), _ptr(bias), _ptr(bd),
                                              _ptr(seg_ptr), int(relu), _ptr(y), xa.shape[0], _stream(xa.device)),
                   "gcnn_linear_fwd")
    return y


def linear_bwd(dy, wa, ymask=None, so=None, dx=None, beta=0, wb=None, dx2=None, beta2=0):
    """dy <- dy*(ymask>0) in place; dx (=|+=) so*(dy @ wa^T); optionally dx2 (=|+=) dy @ wb^T (gcnn_linear_bwd)."""
    _chk(dy, name="dy"); _chk(ymask, name="ymask")
    if dx is None:
        dx = torch.empty_like(dy)
        beta = 0
    if wb is not None and dx2 is None:
        dx2 = torch.empty_like(dy)
        beta2 = 0
    with torch.cuda.device(dy.device):
        _lib.check(_lib.lib().gcnn_linear_bwd(_ptr(dy), _ptr(ymask), _ptr(wa), _ptr(so), _ptr(dx), int(beta), _ptr(wb),
                                              _ptr(dx2), int(beta2), dy.shape[0], _stream(dy.device)), "gcnn_linear_bwd")
    return dx, dx2


def _edge_side(graph: BipartiteGraph, by_left: bool):
    return (graph.l_ptr, graph.l_oth, graph.l_coef, graph.n_left) if by_left else \
           (graph.v_ptr, graph.v_oth, graph.v_coef, graph.n_var)


def conv_edge_fwd(graph: BipartiteGraph, recv_is_left: bool, pl, pr, w_edge, e_shift, e_scale, s1, save=False):
    """S[r] = sum_e relu(s1*(PL[l_e] + c_e*w + PR[v_e])) over the receiver's segment (gcnn_conv_edge_fwd).
    With save=True returns (S, N) where N[R,64] (active edges per receiver and channel) is what conv_edge_bwd consumes."""
    ptr, oth, coef, n_recv = _edge_side(graph, recv_is_left)
    p_recv, p_oth = (pl, pr) if recv_is_left else (pr, pl)
    dev = pl.device
    out = torch.empty((n_recv, EMB), dtype=torch.float32, device=dev)
    nrows = torch.empty((n_recv, EMB), dtype=torch.float32, device=dev) if save else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gcnn_conv_edge_fwd(_ptr(ptr), _ptr(oth), _ptr(coef), n_recv, graph.n_edges, _ptr(p_recv),
                                                 _ptr(p_oth), _ptr(w_edge), _ptr(e_shift), _ptr(e_scale), _ptr(s1),
                                                 _ptr(out), _ptr(nrows), graph.l_max_deg if recv_is_left else graph.v_max_deg,
                                                 _stream(dev)), "gcnn_conv_edge_fwd")
    return (out, nrows) if save else out


def conv_edge_bwd(graph: BipartiteGraph, recv_is_left: bool, nrows, pl, pr, w_edge, e_shift, e_scale, s1, d_s):
    """Gradients of the edge pass: (d_PL, d_PR, d_w_edge[64]).  The receiver side uses the N rows of the forward; the sender
    side recomputes the ReLU pattern from the projected tables PL / PR (nothing per edge was stored)."""
    lib = _lib.lib()
    dev = d_s.device
    n_recv = graph.n_left if recv_is_left else graph.n_var
    d_recv = torch.empty((n_recv, EMB), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gcnn_conv_edge_bwd_recv(_ptr(d_s), _ptr(nrows), _ptr(s1), n_recv, _ptr(d_recv), _stream(dev)),
                   "gcnn_conv_edge_bwd_recv")
        sptr, soth, scoef, n_send = _edge_side(graph, not recv_is_left)
        p_send, p_recv = (pr, pl) if recv_is_left else (pl, pr)
        d_send = torch.empty((n_send, EMB), dtype=torch.float32, device=dev)
        rows = torch.empty((16384, EMB), dtype=torch.float32, device=dev)  # per-block partials of d w_edge (GCNN_EDGE_DW_PARTS)
        n_parts = C.c_int32(0)
        _lib.check(lib.gcnn_conv_edge_bwd_send(_ptr(sptr), _ptr(soth), _ptr(scoef), n_send, graph.n_edges, _ptr(p_send),
                                               _ptr(p_recv), _ptr(w_edge), _ptr(e_shift), _ptr(e_scale), _ptr(s1), _ptr(d_s),
                                               _ptr(d_send), _ptr(rows), C.byref(n_parts),
                                               graph.v_max_deg if recv_is_left else graph.l_max_deg, _stream(dev)),
                   "gcnn_conv_edge_bwd_send")
    d_pl, d_pr = (d_recv, d_send) if recv_is_left else (d_send, d_recv)
    return d_pl, d_pr, rows[:n_parts.value].sum(0)


class SegmentPlan:
    """Receiver-sorted view of an index vector: the plan behind the standalone scatter-sum pass."""

    def __init__(self, index: torch.Tensor, out_size: int, validate=True):
        index = index.to(torch.int32).contiguous()
        e = index.numel()
        g = BipartiteGraph(torch.stack([index, torch.zeros_like(index)]), torch.zeros(e, dtype=torch.float32,
                           device=index.device), out_size, 1, validate, keep_perm=True)
        self.seg_ptr, self.perm, self.n_recv, self.n_edges = g.l_ptr, g.l_perm, int(out_size), e
        srt = bool((index[1:] >= index[:-1]).all()) if e > 1 else True
        self.sorted = srt  # messages already receiver-sorted: stream them without the permutation


class _ScatterSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, messages, plan):
        out = torch.empty((plan.n_recv, EMB), dtype=torch.float32, device=messages.device)
        with torch.cuda.device(messages.device):
            _lib.check(_lib.lib().gcnn_seg_sum_f32(_ptr(messages), _ptr(plan.seg_ptr), None if plan.sorted else _ptr(plan.perm),
                                                   plan.n_recv, _ptr(out), _stream(messages.device)), "gcnn_seg_sum_f32")
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, d_out):
        plan = ctx.plan
        d_out = d_out.contiguous()
        d_msg = torch.empty((plan.n_edges, EMB), dtype=torch.float32, device=d_out.device)
        with torch.cuda.device(d_out.device):
            _lib.check(_lib.lib().gcnn_seg_bcast_f32(_ptr(d_out), _ptr(plan.seg_ptr), None if plan.sorted else _ptr(plan.perm),
                                                     plan.n_recv, _ptr(d_msg), _stream(d_out.device)), "gcnn_seg_bcast_f32")
        return d_msg, None


def scatter_sum(messages: torch.Tensor, index, out_size: int):
    """`tf.scatter_nd(indices=index[:,None], updates=messages, shape=[out_size,64])` (model.py:568-569): duplicates are
    summed, untouched rows are zero.  `index` may be a tensor or a prebuilt SegmentPlan.  Atomic-free and deterministic."""
    _chk(messages, name="messages")
    plan = index if isinstance(index, SegmentPlan) else SegmentPlan(index, out_size)
    if plan.n_edges != messages.shape[0]:
        raise ValueError("one index per message row expected")
    return _ScatterSum.apply(messages, plan)


# ---- cut selection (gcnn_select_cuts): the parallelism filter of the SCIP plugin's cutselselect, model_evaluator.py:109-154 ----
SELECT_MAX_CUTS = 4096


def check_thresholds(p_max, p_max_ub):
    import math
    for name, x in (("p_max", p_max), ("p_max_ub", p_max_ub)):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(float(x)):
            raise ValueError(f"{name} must be a finite number, got {x!r}")


def pack_rows(edge_inds, edge_vals, n_rows, n_vars):
    """Host edge list of rows (row 0 = row id, row 1 = variable id, as get_state builds the cut edges) -> host CSR
    (ptr [n_rows+1], col, val): int32 / int32 / float32, entries of a row in their input order."""
    import numpy as np
    ei = np.asarray(edge_inds)
    ev = np.asarray(edge_vals, dtype=np.float32).reshape(-1)
    if ei.ndim != 2 or ei.shape[0] != 2 or ei.dtype.kind not in "iu" or ev.size != ei.shape[1]:
        raise ValueError(f"forced rows: expected an integer [2,E] index array and E values, got {ei.dtype} {tuple(ei.shape)} and "
                         f"{ev.size} values")
    rows, cols = ei[0].astype(np.int64), ei[1].astype(np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows or cols.min() < 0 or cols.max() >= n_vars):
        raise ValueError(f"forced rows: row ids must be in [0,{n_rows}), variable ids in [0,{n_vars})")
    perm = np.argsort(rows, kind="stable")
    ptr = np.zeros(n_rows + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=ptr[1:])
    return ptr, cols[perm].astype(np.int32), np.ascontiguousarray(ev[perm])


def select_cuts(quality, cut_graph: BipartiteGraph, cut_offsets=None, forced=None, forced_offsets=None, *, p_max=0.1,
                p_max_ub=0.5, max_cuts=None):
    """Parallelism filter of cutselselect on the device, one workgroup per sample (gcnn_select_cuts); nothing is synchronised.

    quality: [total_cuts] fp32 device scores (state order); cut_graph: the cut edge set (its by-left CSR holds the rows);
    cut_offsets: [n_samples+1] int32 device tensor, None = one sample; forced: None or (ptr, col, val) device CSR of the forced
    rows (pack_rows), with forced_offsets [n_samples+1] for more than one sample; max_cuts: the largest sample, None = derived
    (from the total without a host read when that is <= 4,096).  Returns (order [total_cuts] int32, n_kept [n_samples] int32)
    device tensors: order holds sample-local cut indices at each sample's offset; n_kept[s] = -1 flags a sample above max_cuts."""
    check_thresholds(p_max, p_max_ub)
    if not quality.is_cuda or quality.dtype != torch.float32 or quality.dim() != 1:
        raise ValueError("quality must be a 1-D fp32 device tensor")
    quality = quality.contiguous()
    total = quality.numel()
    if cut_graph.n_left != total:
        raise ValueError(f"quality has {total} entries, the cut graph {cut_graph.n_left} rows")
    dev = quality.device
    if cut_offsets is not None:
        cut_offsets = cut_offsets.to(device=dev, dtype=torch.int32).contiguous()
        n_samples = cut_offsets.numel() - 1
        if n_samples < 1:
            raise ValueError("cut_offsets needs n_samples + 1 >= 2 entries")
    else:
        n_samples = 1
    if max_cuts is None:
        max_cuts = total if (cut_offsets is None or total <= SELECT_MAX_CUTS) else \
            int((cut_offsets[1:] - cut_offsets[:-1]).max())
    if max_cuts > SELECT_MAX_CUTS:
        raise _lib.GcnnError(f"select_cuts: a state with {max_cuts} cuts; the device selection handles at most "
                             f"{SELECT_MAX_CUTS} per state and there is no CPU fallback")
    f_ptr = f_col = f_val = None
    n_forced = 0
    if forced is not None:
        f_ptr, f_col, f_val = (t.to(dev).contiguous() for t in forced)
        n_forced = f_ptr.numel() - 1
        if n_samples > 1 and n_forced > 0:
            if forced_offsets is None:
                raise ValueError("forced_offsets is required with forced rows and more than one sample")
            forced_offsets = forced_offsets.to(device=dev, dtype=torch.int32).contiguous()
    order = torch.empty(total, dtype=torch.int32, device=dev)
    n_kept = torch.empty(n_samples, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    ws_bytes = lib.gcnn_select_workspace_bytes(total, n_forced, max_cuts)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gcnn_select_cuts(_ptr(quality), _ptr(cut_graph.l_ptr), _ptr(cut_graph.l_oth), _ptr(cut_graph.l_coef),
                                        _ptr(cut_offsets), n_samples, total, int(max_cuts), cut_graph.n_var, _ptr(f_ptr),
                                        _ptr(f_col), _ptr(f_val), _ptr(forced_offsets) if n_forced else None, n_forced,
                                        float(p_max), float(p_max_ub), _ptr(order), _ptr(n_kept), _ptr(ws), ws_bytes,
                                        _stream(dev)), "gcnn_select_cuts")
    return order, n_kept


# ---- ensembles (gcnn_ensemble_mean): the mean of several models' scores of one state, model_trainer.py:38-49's five seeds --------
ENSEMBLE_MAX = _lib.GROUP_MAX


def ensemble_mean(member_scores):
    """Mean of 1..8 score rows on the device (k_ens_mean); nothing is synchronised.  member_scores: a list of 1-D fp32 device
    tensors of one length, in the ensemble's order.  acc = row[0], acc = acc + row[m] in that order, acc / float(M): fp32,
    round-to-nearest, nothing contracted, so a float32 loop on the host gives the same bits; one row comes back as its copy."""
    rows = list(member_scores)
    if not 1 <= len(rows) <= ENSEMBLE_MAX:
        raise ValueError(f"ensemble_mean: 1..{ENSEMBLE_MAX} score rows expected, got {len(rows)}")
    first = rows[0]
    for r in rows:
        if not isinstance(r, torch.Tensor) or not r.is_cuda or r.dtype != torch.float32 or r.dim() != 1:
            raise ValueError("ensemble_mean: every row must be a 1-D fp32 device tensor")
        if r.device != first.device or r.numel() != first.numel():
            raise ValueError("ensemble_mean: the rows must have one length and live on one device")
    rows = [r.contiguous() for r in rows]
    n = first.numel()
    if n >= 2 ** 31:
        raise ValueError("ensemble_mean: at most 2^31 - 1 scores per row")
    mean = torch.empty(n, dtype=torch.float32, device=first.device)
    ptrs = (C.c_void_p * len(rows))(*(r.data_ptr() for r in rows))
    with torch.cuda.device(first.device):
        _lib.check(_lib.lib().gcnn_ensemble_mean(ptrs, len(rows), n, _ptr(mean), _stream(first.device)), "gcnn_ensemble_mean")
    return mean
