"""Host arrays in, one C call, host arrays out: the host side of gcnn_infer, gcnn_infer_select, gcnn_infer_batch, the LP-snapshot
calls, gcnn_lp_batch, gcnn_infer_models and gcnn_lp_models (include/gcnn_hip.h).  What `GCNN.score_state`, `select_cuts` and their many-state forms (model.py) are composed of: the checks
of a host state, the one packer of the upload, the forced rows, and the two sessions that own the staging buffers.  `LPSession`
(`GCNN.open_lp`) is the host side of gcnn_lp_rows_build and gcnn_lp_round: an LP that stays on the device across separation rounds;
`LPSessionGroup` is the host side of gcnn_lp_rounds: the rounds of several such sessions in one call.  `_EnsembleSession` and
`_LPEnsembleSession` are the host side of gcnn_infer_ensemble and gcnn_lp_ensemble: ONE state scored by several models, their mean
ranked or selected (`ModelSet.score_ensemble` and its siblings); `_EnsembleBatchSession` and `_LPEnsembleBatchSession` are the host
side of gcnn_infer_ensemble_batch and gcnn_lp_ensemble_batch: up to 64 states scored by one ensemble in one call
(`ModelSet.score_ensemble_many` and its siblings)."""

from __future__ import annotations

import ctypes as C
import time
import weakref
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops

BAD_INDEX = "edge index out of range (left ids must be in [0,n_left), variable ids in [0,n_vars))"


class ScoreArray(np.ndarray):
    """Host-side scores of the single-state inference path: an ndarray that also answers `.numpy()` (the reference's call sites do
    `get_improvements(state, False).numpy()`, model_evaluator.py:103).  `rankings` (optional): indices in descending score
    order, equal scores in index order -- `sorted(range(n), key=lambda x: quality[x], reverse=True)` of model_evaluator.py:110."""
    rankings = None
    cut_index = None      # calls that start from an LP snapshot: state position -> input cut (scores are in STATE order)
    members = None        # `ModelSet.score_ensemble`: float32 [M, K], every member's own scores (the array itself is their mean)

    def numpy(self):
        return np.asarray(self)


class SelectResult:
    """What `GCNN.select_cuts` returns: `order` (int32 cut indices in STATE order: the kept cuts first, best first, then the
    removed ones), `n_selected` = min(n_kept, max_selected) -- the reference's 'nselectedcuts' --, `n_kept` and the `scores`."""

    features = None       # `HybridSelector` (hybrid.py): [K, 3] float64 efficacy, integer support, objective parallelism
    members = None        # `ModelSet.select_cuts_ensemble`: float32 [M, K], every member's own scores (`scores` is their mean)

    def __init__(self, order, n_kept, n_selected, scores, cut_index=None):
        self.order, self.n_kept, self.n_selected, self.scores = order, n_kept, n_selected, scores
        self.cut_index = cut_index     # `select_cuts_lp`: state position -> input cut, so cut_index[order[:n_selected]] are the inputs

    def __repr__(self):
        return f"SelectResult(n_selected={self.n_selected}, n_kept={self.n_kept}, order={self.order!r})"


class _UseGeneralPath(Exception):
    """The specialised single-state path declined (unsorted edge list, very long segment, too many variables)."""


def is_host_state(state):
    """True for a tuple of host arrays; False for a prepared `Batch` (it has `dims`) and for a tuple that holds a torch tensor."""
    return not (hasattr(state, "dims") or any(isinstance(x, torch.Tensor) for x in state[:7]))


def n_selected(n_kept, max_selected):
    return n_kept if max_selected is None else min(n_kept, int(max_selected))


def stable_ranking(scores):
    """Cut indices in descending score order, equal scores in index order."""
    return np.argsort(-np.asarray(scores), kind="stable").astype(np.int32)


def check_feature_shapes(c, v, k, n_cons, n_vars, n_cuts):
    """Feature matrices (NumPy arrays or torch tensors) against their widths and the state's three counts."""
    for name, t, f in (("cons_feats", c, 4), ("var_feats", v, 14), ("cut_feats", k, 6)):
        if t.ndim != 2 or t.shape[1] != f:
            raise ValueError(f"{name} must have shape [N,{f}], got {tuple(t.shape)}")
    for name, total, t in (("n_cons", n_cons, c), ("n_vars", n_vars, v), ("n_cuts", n_cuts, k)):
        if int(total) != t.shape[0]:
            raise ValueError(f"{name}={int(total)} does not match the {t.shape[0]} feature rows")


def check_state(inputs):
    """The model's 10-tuple of host arrays -> (the seven arrays, key = (n_cons, n_vars, n_cuts, E1, E2))."""
    c, cei, cef, v, k, kei, kef, n_cons, n_vars, n_cuts = inputs
    c, v, k = np.asarray(c), np.asarray(v), np.asarray(k)
    cei, kei, cef, kef = np.asarray(cei), np.asarray(kei), np.asarray(cef), np.asarray(kef)
    check_feature_shapes(c, v, k, n_cons, n_vars, n_cuts)
    for name, ei, ef in (("cons_edge_inds", cei, cef), ("cut_edge_inds", kei, kef)):
        if ei.ndim != 2 or ei.shape[0] != 2 or ei.dtype.kind not in "iu":
            raise ValueError(f"{name} must be an integer array of shape [2,E], got {ei.dtype} {tuple(ei.shape)}")
        if ef.size != ei.shape[1]:
            raise ValueError("edge features must hold one value per edge")
        # the upload packs indices as int32 with an unchecked cast: an int64 / uint index of 2**31 or more would wrap, possibly
        # into range, and score another graph -- such lists are rejected here (int32 input cannot overflow; the device
        # flags catch everything that is out of range but representable)
        if ei.dtype != np.int32 and ei.size and (int(ei.max()) > 2 ** 31 - 1 or int(ei.min()) < -2 ** 31):
            raise ValueError(BAD_INDEX)
    key = (c.shape[0], v.shape[0], k.shape[0], cei.shape[1], kei.shape[1])
    return (c, cei, cef, v, k, kei, kef), key


def edges_without_nodes(key):
    """True for a state (key of `check_state`) with edges but no rows or no variables for them: every id of such a list is out of
    range.  The single-state session raises BAD_INDEX for it on the host and the batched call hands it to that session
    (`GCNN._admit_state`); the library refuses it as well (edges_without_nodes, gcnn_capi.hip)."""
    n_cons, n_vars, n_cuts, e1, e2 = key
    return bool((e1 and (n_cons == 0 or n_vars == 0)) or (e2 and (n_cuts == 0 or n_vars == 0)))


def pack_state(buf, base, arrays, key, where, scratch):
    """Write one checked state into a staging buffer.  `buf`: writable uint8 array, `base`: its address; `where`: the byte offset
    of each of the seven arrays.  Features are cast to fp32; an edge set lands as [rows | cols] int32 and fp32 values, brought
    into row order on the way when it is not (gcnn_host_pack_edges: one native pass per list, a stable counting sort only for a
    list in another order -- NumPy's stable argsort alone would take longer than the whole general path).  `scratch`: the sort's
    int32 scratch or None; returned, grown when a state needed more."""
    c, cei, cef, v, k, kei, kef = arrays
    oc, oci, ocf, ov, ok, oki, okf = where
    pack = _lib.lib().gcnn_host_pack_edges
    for off, a in ((oc, c), (ov, v), (ok, k)):
        if a.size:
            np.copyto(buf[off:off + 4 * a.size].view(np.float32).reshape(a.shape), a, casting="unsafe")
    for io, fo, ei, ef, n_left in ((oci, ocf, cei, cef, key[0]), (oki, okf, kei, kef, key[2])):
        if not ei.size:
            continue
        ei32 = np.ascontiguousarray(ei, dtype=np.int32)                  # no copies for what get_state hands over
        ef32 = np.ascontiguousarray(ef, dtype=np.float32).reshape(-1)
        if scratch is None or scratch.size < n_left + 1:
            scratch = np.empty(2 * (n_left + 1), np.int32)
        rc = pack(ei32.ctypes.data, ei32.ctypes.data + 4 * ei32.shape[1], ef32.ctypes.data, ei32.shape[1], n_left, base + io,
                  base + fo, scratch.ctypes.data)
        if rc < 0:      # (0 / 1 / 2: packed -- as it was, sorted here, or as it was with a row id the device check reports)
            _lib.check(rc, "gcnn_host_pack_edges")
    return scratch


def normalize_forced(forced, n_vars):
    """Forced rows as `GCNN.select_cuts` takes them -- None, (edge_inds [2,E], values [E]) or (edge_inds, values, n_forced), NumPy
    or torch -- -> host CSR (ptr, col, val) of `ops.pack_rows`.  Two entries take n_forced = max row id + 1."""
    if forced is None:
        forced = (np.zeros((2, 0), np.int32), np.zeros(0, np.float32), 0)
    if len(forced) == 2:
        fi = np.asarray(forced[0])
        forced = (forced[0], forced[1], int(fi[0].max()) + 1 if fi.size else 0)
    fi, fv, n_forced = forced
    if isinstance(fi, torch.Tensor):
        fi, fv = fi.cpu().numpy(), fv.cpu().numpy()
    return ops.pack_rows(fi, fv, int(n_forced), n_vars)


def al16(x):
    return (x + 15) & ~15


def prefix(xs):
    """[0, xs[0], xs[0] + xs[1], ...]: the offset of every item of a stack and, last, its total."""
    out = [0]
    for x in xs:
        out.append(out[-1] + x)
    return out


def forced_shapes(forced):
    """(rows, entries) per state of packed forced rows [(ptr, col, val)]; () for None."""
    return tuple((f[0].size - 1, f[1].size) for f in forced) if forced is not None else ()


def forced_counts(fshapes):
    """`forced_shapes` as the (n_forced, n_forced_entries) int32 arrays of a many-state call; (None, None) without forced rows."""
    n = len(fshapes)
    return tuple((C.c_int32 * n)(*(f[j] for f in fshapes)) for j in (0, 1)) if fshapes else (None, None)


def _carve(arena, blocks, floats):
    """{name: host copy of the `n` 32-bit words at byte offset `off` of a device arena} for blocks = {name: (off, n)}; int32 but for
    the names in `floats`."""
    return {name: arena[off:off + 4 * n].view(torch.float32 if name in floats else torch.int32).cpu().numpy()
            for name, (off, n) in blocks.items()}


def _unsupported(rc, what):
    """True when a layout function declines the sizes (-4); any other failure raises."""
    if rc != -4:
        _lib.check(rc, what)
    return rc == -4


class _Staging:
    """Persistent pinned staging buffers, a device arena, the packer's scratch and a bounded cache of layouts."""
    CAP = 256

    def __init__(self, model):
        self.model = model
        self.pin_in = self.pin_out = self.arena = None
        self.in_np = self.out_np = None
        self.scratch = None
        self.layouts = {}
        self.last = None          # what the last call left in the arena: the layout and its sizes (`last_plan`, `last_state`)

    def cached(self, key, make, *args):
        """The layout entry of `key`; `make(*args)` builds a missing one, or returns False where the library declines."""
        lay = self.layouts.get(key)
        if lay is None:
            lay = make(*args)
            if len(self.layouts) >= self.CAP:
                self.layouts.pop(next(iter(self.layouts)))   # evict the oldest entry only
            self.layouts[key] = lay
        return lay

    @staticmethod
    def _pin(pin, view, nbytes, floor):
        """A pinned staging buffer and its NumPy view that hold `nbytes`: one too small is replaced by one twice that size."""
        if pin is None or pin.numel() < nbytes:
            pin = torch.empty(max(2 * nbytes, floor), dtype=torch.uint8).pin_memory()
            view = pin.numpy()
        return pin, view

    def _buffers(self, L):
        self.pin_in, self.in_np = self._pin(self.pin_in, self.in_np, L.in_bytes, 1 << 20)
        self.pin_out, self.out_np = self._pin(self.pin_out, self.out_np, L.out_bytes, 1 << 16)
        if self.arena is None or self.arena.numel() < L.arena_bytes:
            self.arena = None
            self.arena = torch.empty(max(2 * L.arena_bytes, 1 << 24), dtype=torch.uint8, device=self.model.device)

    def _put_forced(self, offsets, arrays):
        """Forced-row arrays (host, packed) into the upload at their byte offsets."""
        for off, a in zip(offsets, arrays):
            self.in_np[off:off + a.nbytes] = a.view(np.uint8)

    def _put_forced_stacked(self, offsets, f_off, fe_off, forced):
        """The forced rows of every state of a many-state call, stacked, into the upload at the byte `offsets` of ptr | col | val.
        `f_off`, `fe_off`: the states' offsets over the stacked rows and entries.  A state's row offsets are shifted by the entries
        in front of it; its closing one is the next state's first.  `forced` None: the one offset of no rows."""
        buf = self.in_np
        if forced is None:
            buf[offsets[0]:offsets[0] + 4] = 0
            return
        o_ptr, o_col, o_val = offsets
        for s, (fptr, fcol, fval) in enumerate(forced):
            o, e = o_ptr + 4 * f_off[s], 4 * fe_off[s]
            buf[o:o + 4 * fptr.size].view(np.int32)[:] = fptr + fe_off[s]
            buf[o_col + e:o_col + e + fcol.nbytes] = fcol.view(np.uint8)
            buf[o_val + e:o_val + e + fval.nbytes] = fval.view(np.uint8)

    def _enqueue_wait(self, name, head, tail, timings=None, t0=0.0, params=True, arena=None, may_decline=False, **extra):
        """The C call `name`(*head, params, the two staging buffers, the arena and its size, *tail, stream) on the model's device
        and its current stream, then the wait for the download.  `params`: True for the model's own, the argument itself for a
        call of several models, None for a call that takes none.  `arena`: a device uint8 tensor to run in instead of the
        session's own.  `may_decline`: a call that returns -4 is not an error -- nothing was enqueued and True is returned.
        `timings` (optional dict): filled with the host-side phases in seconds -- `pack` (since `t0`), `enqueue`, `wait` -- and
        with `extra`."""
        t1 = time.perf_counter() if timings is not None else 0.0
        dev, P = self.model.device, C.c_void_p
        arena = self.arena if arena is None else arena
        first = () if params is None else (P(self.model._flat.data_ptr()) if params is True else params,)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            rc = getattr(_lib.lib(), name)(*head, *first, P(self.pin_in.data_ptr()), P(self.pin_out.data_ptr()), P(arena.data_ptr()),
                                           arena.numel(), *tail, P(stream.cuda_stream))
            if rc:
                if may_decline and rc == -4:
                    return True
                _lib.check(rc, name)
            if timings is None:
                stream.synchronize()
                return False
            t2 = time.perf_counter()
            stream.synchronize()
        timings.update(pack=t1 - t0, enqueue=t2 - t1, wait=time.perf_counter() - t2, **extra)
        return False

    def _verdict(self, flags_off):
        """The flag policy on one state's four plan flags in the download: "bad_index" (an index out of range), "declined"
        (anything else the specialised plan does not take) or None: the answer stands."""
        flags = self.out_np[flags_off:flags_off + 16].view(np.int32)
        if flags[0]:
            return "bad_index"
        return "declined" if flags[1] or flags[2] or flags[3] else None

    def _read(self, scores_off, order_off, n_kept_off, n, out=None):
        """(scores, order | None, n_kept | None) of a state's `n` cuts, read at the given byte offsets (None: not asked for) of the
        download `out` (default: the session's own)."""
        out = self.out_np if out is None else out
        scores = out[scores_off:scores_off + 4 * n].view(np.float32).copy().view(ScoreArray)
        order = None if order_off is None else out[order_off:order_off + 4 * n].view(np.int32).copy()
        n_kept = None if n_kept_off is None else int(out[n_kept_off:n_kept_off + 4].view(np.int32)[0])
        return scores, order, n_kept

    def _answer(self, flags_off, *where):
        """One state's answer of a single call: the flag policy as exceptions (ValueError, _UseGeneralPath), then `_read(*where)`."""
        verdict = self._verdict(flags_off)
        if verdict == "bad_index":
            raise ValueError(BAD_INDEX)
        if verdict:
            raise _UseGeneralPath()
        return self._read(*where)

    def _collect(self, out_off, k_off, n_states, mode, more=None):
        """Per state of a many-state call's download: ("ok", scores, order, n_kept), ("bad_index",) or ("declined",).  `k_off`: the
        states' offsets over the stacked cuts.  `more(s, lo, n)` (the LP call): what it returns is appended to the state's "ok"
        answer, the ValueError it raises becomes the state's ("error", exc)."""
        res = []
        for s in range(n_states):
            lo, n = 4 * k_off[s], k_off[s + 1] - k_off[s]
            try:
                tail = more(s, lo, n) if more else ()
            except ValueError as exc:
                res.append(("error", exc))
                continue
            verdict = self._verdict(out_off[3] + 16 * s)
            res.append((verdict,) if verdict else ("ok",) + self._read(
                out_off[0] + lo, out_off[1] + lo if mode else None, out_off[2] + 4 * s if mode == _lib.IBATCH_SELECT else None, n) + tail)
        return res


def _solo_layout(key, n_forced=None, n_entries=None):
    """Layout entry of one state: gcnn_infer's, or with forced sizes gcnn_infer_select's (whose extra offsets come last).
    in_off[0] .. in_off[1] is the block the caller zeroes, in_off[1..7] say `where` the seven arrays go."""
    dims = _lib.Dims(*key)
    if n_forced is None:
        L, SL = _lib.InferLayout(), None
        declined = _unsupported(_lib.lib().gcnn_infer_layout_for(C.byref(dims), C.byref(L)), "gcnn_infer_layout_for")
    else:
        SL = _lib.SelectLayout()
        declined = _unsupported(_lib.lib().gcnn_infer_select_layout_for(C.byref(dims), n_forced, n_entries, C.byref(SL)),
                                "gcnn_infer_select_layout_for")
        L = SL.infer
    in_off = tuple(L.in_off)
    return False if declined else (dims, L, in_off[0], in_off[1], in_off[1:], list(L.out_off), SL)


class _InferenceSession(_Staging):
    """Host side of gcnn_infer and gcnn_infer_select: one C call per state."""

    def _run(self, inputs, want_order, timings, forced=None, p_max=0.0, p_max_ub=0.0):
        """check -> layout -> pack -> call -> (scores, order | None, n_kept | None); with `forced` the call is gcnn_infer_select."""
        t0 = time.perf_counter()
        arrays, key = check_state(inputs)
        if edges_without_nodes(key):
            raise ValueError(BAD_INDEX)        # before anything is enqueued: the device plan has no row to park such ids on
        fshape = () if forced is None else (forced[0].size - 1, forced[1].size)
        lay = self.cached(key + fshape, _solo_layout, key, *fshape)
        if lay is False or (want_order and key[2] > 4096):
            raise _UseGeneralPath()
        dims, L, zero_from, zero_to, where, out_off, SL = lay
        self._buffers(L)
        self.in_np[zero_from:zero_to] = 0      # the plan's counters and flags travel zeroed inside the upload
        # The specialised plan wants lists sorted by row, which is what get_state emits (utils.py:102-104); `pack_state` sees to it
        self.scratch = pack_state(self.in_np, self.pin_in.data_ptr(), arrays, key, where, self.scratch)
        if forced is None:
            self._enqueue_wait("gcnn_infer", (C.byref(dims),), (int(want_order),), timings, t0)
        else:
            self._put_forced(SL.forced_off, forced)
            self._enqueue_wait("gcnn_infer_select", (C.byref(dims), *fshape), (float(p_max), float(p_max_ub)), timings, t0)
        self.last = (L, key)
        return self._answer(out_off[2], out_off[0], out_off[1] if want_order else None, SL.n_kept_off if forced is not None else None,
                            key[2])

    def last_plan(self):
        """The graph plan the last call left in the arena, as host arrays by name (tests compare it with a restatement entry by
        entry): the by-left offsets, both uploaded lists as the count step left them, the plan's counters and the device flags,
        and the by-variable structure of the constraint edges."""
        L, (c, v, k, e1, e2) = self.last
        i, d, z = list(L.in_off), list(L.dev_off), L.in_off[0]
        blocks = dict(vcount=(z, v), cursor=(z + 4 * v, v), flags=(z + 8 * v, 4), l_ptr0=(d[0], c + 1), l_ptr1=(d[1], k + 1),
                      inds0=(i[2], 2 * e1), inds1=(i[6], 2 * e2), v_ptr=(d[2], v + 1), v_pos=(d[3], e1), v_oth=(d[4], e1), v_coef=(d[5], e1))
        return _carve(self.arena, blocks, ("v_coef",))

    def run(self, inputs, want_order, timings=None):
        """Scores of ONE host state (`.rankings` from the device when `want_order`).  `timings` (optional dict): filled with the
        host-side phases in seconds (tools/latency.py)."""
        scores, order, _ = self._run(inputs, want_order, timings)
        if want_order:
            scores.rankings = order
        return scores

    def run_select(self, inputs, forced, p_max, p_max_ub):
        """gcnn_infer_select: scores, selection order and n_kept of ONE host state.  `forced`: (ptr, col, val) host arrays
        (ops.pack_rows).  Raises _UseGeneralPath where gcnn_infer would."""
        return self._run(inputs, True, None, forced, p_max, p_max_ub)


class _BatchSession(_Staging):
    """Host side of gcnn_infer_batch: one C call for up to 64 host states.  `run` answers per state: ("ok", scores, order, n_kept),
    ("bad_index",) or ("declined",)."""
    MAX = _lib.IBATCH_MAX
    CAP = 64
    # in_off[2..8] hold the seven arrays of every state: (table column of the state's offset, bytes per row or edge)
    PLACES = ((0, 16), (3, 8), (3, 4), (1, 56), (2, 24), (4, 8), (4, 4))

    def __init__(self, model):
        super().__init__(model)
        self.calls = 0            # C calls made (tools and tests read it)

    def _layout(self, keys, fshapes, mode):
        n = len(keys)
        dims = (_lib.Dims * n)(*(_lib.Dims(*k) for k in keys))
        nf, nfe = forced_counts(fshapes)
        L = _lib.IbatchLayout()
        if _unsupported(_lib.lib().gcnn_infer_batch_layout_for(n, dims, nf, nfe, mode, C.byref(L)), "gcnn_infer_batch_layout_for"):
            return False
        table = np.zeros(_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE, np.int32)
        _lib.check(_lib.lib().gcnn_infer_batch_fill_table(n, dims, nf, nfe, table.ctypes.data), "gcnn_infer_batch_fill_table")
        cols = table.reshape(_lib.IBATCH_TABLE_COLS, _lib.IBATCH_TABLE_STRIDE)[:, :n + 1].tolist()
        return self._entry(dims, nf, nfe, L, table, cols)

    @classmethod
    def _entry(cls, dims, nf, nfe, L, table, cols, **more):
        """A layout entry: the call's arguments, the layout with its offsets as lists, the table, its columns as lists (c, v, k, e1,
        e2, f, fe offsets per state) and `where` every state's arrays go."""
        in_off = list(L.in_off)
        return SimpleNamespace(dims=dims, nf=nf, nfe=nfe, L=L, in_off=in_off, out_off=list(L.out_off), table=table, cols=cols,
                               where=cls._where(in_off, cols, len(dims)), **more)

    @classmethod
    def _where(cls, in_off, cols, n):
        """Per state the byte offsets of its seven arrays in the upload (`pack_state`'s `where`)."""
        return [tuple(in_off[2 + j] + size * cols[col][s] for j, (col, size) in enumerate(cls.PLACES)) for s in range(n)]

    def _pack(self, lay, checked, forced):
        """The upload of one call into the pinned buffer: the table, the zeroed block, every state, the forced rows."""
        in_off = lay.in_off
        self._buffers(lay.L)
        buf, base = self.in_np, self.pin_in.data_ptr()
        buf[in_off[0]:in_off[0] + lay.table.nbytes] = lay.table.view(np.uint8)
        buf[in_off[1]:in_off[2]] = 0          # flags and by-left offsets travel zeroed inside the upload
        for (arrays, key), where in zip(checked, lay.where):
            self.scratch = pack_state(buf, base, arrays, key, where, self.scratch)
        self._put_forced_stacked(in_off[9:12], lay.cols[5], lay.cols[6], forced)

    def run(self, checked, forced, mode, p_max=0.0, p_max_ub=0.0):
        """checked: [(arrays, key)] as `check_state` returns them; forced: None or [(ptr, col, val)] per state.
        Returns None when the library declines the union as a whole (too large: the caller splits it)."""
        keys = tuple(k for _, k in checked)
        fshapes = forced_shapes(forced)
        lay = self.cached((mode, keys, fshapes), self._layout, keys, fshapes, mode)
        if lay is False:
            return None
        self._pack(lay, checked, forced)
        self._enqueue_wait("gcnn_infer_batch", (len(checked), lay.dims, lay.nf, lay.nfe, mode), (float(p_max), float(p_max_ub)))
        self.calls += 1
        self.last = (lay.L, len(checked))
        return self._collect(lay.out_off, lay.cols[2], len(checked), mode)

    def last_plan(self):
        """The union's graph plan as the last call left it in the arena, as host arrays by name (`_InferenceSession.last_plan`'s
        counterpart): what k_ib_unpack wrote and the by-variable structure behind it."""
        L, s = self.last
        t, i, d = L.total, list(L.in_off), list(L.dev_off)
        e1, e2, v = t.n_cons_edges, t.n_cut_edges, t.n_vars
        l0 = i[1] + al16(16 * s)
        blocks = dict(flags=(i[1], 4 * s), l_ptr0=(l0, t.n_cons + 1), l_ptr1=(l0 + al16(4 * (t.n_cons + 1)), t.n_cuts + 1),
                      left=(d[0], e1), var0=(d[1], e1), var1=(d[2], e2), iota=(d[3], e1), v_ptr=(d[6], v + 1), v_oth=(d[7], e1),
                      v_coef=(d[8], e1), f_col=(d[9], L.n_forced_entries))
        return _carve(self.arena, blocks, ("v_coef",))


class _ModelsSession:
    """Host side of gcnn_infer_models: one C call for up to 64 host states of up to 8 models.  It packs with a `_BatchSession`'s
    packer into that session's pinned buffers and arena (`base`: the batch session of one of the models -- every model of the
    call lives on its device), and adds what the call needs beyond them: the model words of the table and the pinned staging
    buffer of the grouped forward passes' launch tables."""
    MAX = _lib.IBATCH_MAX
    MAX_MODELS = _lib.GROUP_MAX
    CAP = _BatchSession.CAP
    UNSUPPORTED = "unsupported"
    cached = _Staging.cached          # the same bounded cache of layouts

    def __init__(self, base):
        self.base = base
        self.layouts = {}
        self.staging = None
        self.calls = 0
        self.last = None

    def _layout(self, keys, fshapes, mode, model_of):
        n, n_models = len(keys), model_of[-1] + 1
        dims = (_lib.Dims * n)(*(_lib.Dims(*k) for k in keys))
        nf, nfe = forced_counts(fshapes)
        mos = (C.c_int32 * n)(*model_of)
        ML = _lib.MbatchLayout()
        if _unsupported(_lib.lib().gcnn_infer_models_layout_for(n, dims, nf, nfe, mode, n_models, mos, C.byref(ML)),
                        "gcnn_infer_models_layout_for"):
            return False
        table = np.zeros(_lib.MBATCH_TABLE_WORDS, np.int32)
        _lib.check(_lib.lib().gcnn_infer_models_fill_table(n, dims, nf, nfe, n_models, mos, table.ctypes.data),
                   "gcnn_infer_models_fill_table")
        cols = table[:_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE].reshape(_lib.IBATCH_TABLE_COLS, -1)[:, :n + 1].tolist()
        return _BatchSession._entry(dims, nf, nfe, ML.u, table, cols, ML=ML, mos=mos, n_models=n_models)

    def run(self, checked, forced, mode, model_of, models, p_max=0.0, p_max_ub=0.0):
        """checked, forced: as `_BatchSession.run` takes them, sorted by model; model_of: the model number of every state
        (non-decreasing, from 0, no gaps); models: the `GCNN` of every number.  Returns `_BatchSession.run`'s list, None when the
        library declines the union's sizes (the caller splits it) or UNSUPPORTED when it declines the call as a whole."""
        base = self.base
        keys = tuple(k for _, k in checked)
        fshapes = forced_shapes(forced)
        lay = self.cached((mode, keys, fshapes, tuple(model_of)), self._layout, keys, fshapes, mode, model_of)
        if lay is False:
            return None
        base._pack(lay, checked, forced)
        self.staging, _ = base._pin(self.staging, None, lay.ML.table_bytes, 1 << 16)
        params = (C.c_void_p * lay.n_models)(*(m._flat.data_ptr() for m in models))
        if base._enqueue_wait("gcnn_infer_models", (len(checked), lay.dims, lay.nf, lay.nfe, mode, lay.n_models, lay.mos),
                              (C.c_void_p(self.staging.data_ptr()), float(p_max), float(p_max_ub)), params=params, may_decline=True):
            return self.UNSUPPORTED
        self.calls += 1
        self.last = (lay.ML, len(checked))
        base.last = None          # the arena no longer holds that session's own plan
        return base._collect(lay.out_off, lay.cols[2], len(checked), mode)

    def last_plan(self):
        """Every model's graph plan as the last call left it in the arena: a list with, per model, the arrays of
        `_BatchSession.last_plan` for that model's sub-union (ids relative to the model), as host arrays by name."""
        ML, s = self.last
        L, t = ML.u, ML.u.total
        i, d, M = list(L.in_off), list(L.dev_off), ML.n_models
        l0 = i[1] + al16(16 * s)
        l1 = l0 + al16(4 * (t.n_cons + M))
        plans, c, v, k, e1, e2 = [], 0, 0, 0, 0, 0
        for m in range(M):
            dm = ML.model[m]
            blocks = dict(l_ptr0=(l0 + 4 * (c + m), dm.n_cons + 1), l_ptr1=(l1 + 4 * (k + m), dm.n_cuts + 1),
                          left=(d[0] + 4 * e1, dm.n_cons_edges), var0=(d[1] + 4 * e1, dm.n_cons_edges),
                          var1=(d[2] + 4 * e2, dm.n_cut_edges), v_ptr=(d[6] + 4 * (v + m), dm.n_vars + 1),
                          v_oth=(d[7] + 4 * e1, dm.n_cons_edges), v_coef=(d[8] + 4 * e1, dm.n_cons_edges))
            plans.append(_carve(self.base.arena, blocks, ("v_coef",)))
            c, v, k, e1, e2 = c + dm.n_cons, v + dm.n_vars, k + dm.n_cuts, e1 + dm.n_cons_edges, e2 + dm.n_cut_edges
        return plans


class _LPSession(_Staging):
    """Host side of the calls that start from a raw LP snapshot (lpstate.py): gcnn_lp_infer / gcnn_lp_infer_select -- one upload of
    the packed snapshot, the state built in the arena, one download -- and gcnn_lp_state, which leaves the state in device tensors."""
    def __init__(self, model):
        super().__init__(model)
        self.deep_check = False   # True: the O(nnz) facts are checked on the host as well (lpstate.check_snapshot)

    @staticmethod
    def _layout(dims, n_forced, n_entries):
        from . import lpstate
        _, L = lpstate.lp_layout(dims, n_forced, n_entries)
        return L, list(L.snap_off), list(L.forced_off), list(L.out_off)

    def _checked(self, snap, n_forced=-1, n_entries=0):
        from . import lpstate
        arrays, dims = lpstate.check_snapshot(snap, self.deep_check)
        key = tuple(v for k, v in dims.items() if isinstance(v, int)) + (n_forced, n_entries)
        return arrays, dims, self.cached(key, self._layout, dims, n_forced, n_entries)

    def run(self, snap, want_order, timings=None, forced=None, p_max=0.0, p_max_ub=0.0):
        """check -> layout -> pack -> one call -> (scores, order | None, n_kept | None, cut_index), all in STATE order."""
        from . import lpstate
        t0 = time.perf_counter()
        fshape = (-1, 0) if forced is None else (forced[0].size - 1, forced[1].size)
        arrays, dims, (L, snap_off, forced_off, out_off) = self._checked(snap, *fshape)
        n = dims["n_cuts"]
        if not L.call_supported or (want_order and n > 4096):
            raise _UseGeneralPath()
        d = _lib.LpDims(**dims)
        self._buffers(L)
        lpstate.pack_snapshot(self.in_np, snap_off, arrays)
        if forced is None:
            self._enqueue_wait("gcnn_lp_infer", (C.byref(d),), (int(want_order),), timings, t0, upload_bytes=int(L.in_bytes))
        else:
            self._put_forced(forced_off, forced)
            self._enqueue_wait("gcnn_lp_infer_select", (C.byref(d), *fshape), (float(p_max), float(p_max_ub)), timings, t0,
                               upload_bytes=int(L.in_bytes))
        self.last = (L, lpstate.state_key(dims))
        out = self.out_np
        lpstate.raise_for_flags(out[out_off[4]:out_off[4] + 16].view(np.int32))
        answer = self._answer(out_off[2], out_off[0], out_off[1] if want_order else None, out_off[3] if forced is not None else None, n)
        return answer + (out[out_off[5]:out_off[5] + 4 * n].view(np.int32).copy(),)

    def last_state(self):
        """The seven arrays the last single call built in the arena, as host arrays (tests compare them with gcnn_lp_state's)."""
        L, (c, v, k, e1, e2) = self.last
        off = list(L.state.in_off)
        shapes = ((c, 4), (2, e1), (e1, 1), (v, 14), (k, 6), (2, e2), (e2, 1))
        kinds = (torch.float32, torch.int32, torch.float32, torch.float32, torch.float32, torch.int32, torch.float32)
        out = []
        for o, shape, dt in zip(off[1:], shapes, kinds):
            out.append(self.arena[o:o + 4 * shape[0] * shape[1]].view(dt).view(shape).cpu().numpy())
        return tuple(out)

    def build_state(self, snap):
        """gcnn_lp_state: the snapshot goes up once, the state stays on the device.  Returns (the model's 10-tuple with device
        tensors, cut_index as a device tensor).  Raises ValueError for what the device flags."""
        from . import lpstate
        arrays, dims, (L, snap_off, _, _) = self._checked(snap)
        d = _lib.LpDims(**dims)
        self.pin_in, self.in_np = self._pin(self.pin_in, self.in_np, L.snap_bytes, 1 << 20)
        lpstate.pack_snapshot(self.in_np, snap_off, arrays)
        dev = self.model.device
        c, v, k, e1, e2 = lpstate.state_key(dims)
        f32, i32 = torch.float32, torch.int32
        with torch.cuda.device(dev):
            snap_dev = torch.empty(max(L.snap_bytes, 16), dtype=torch.uint8, device=dev)
            snap_dev.copy_(self.pin_in[:snap_dev.numel()], non_blocking=True)
            scratch = torch.empty(max(L.scratch_bytes, 16), dtype=torch.uint8, device=dev)
            outs = [torch.empty(s, dtype=t, device=dev) for s, t in (((c, 4), f32), ((2, e1), i32), ((e1, 1), f32), ((v, 14), f32),
                                                                     ((k, 6), f32), ((2, e2), i32), ((e2, 1), f32), ((k,), i32),
                                                                     ((4,), i32))]
            P = C.c_void_p
            stream = torch.cuda.current_stream(dev)
            _lib.check(_lib.lib().gcnn_lp_state(C.byref(d), P(snap_dev.data_ptr()), P(scratch.data_ptr()), scratch.numel(),
                                                *(P(t.data_ptr()) for t in outs), P(stream.cuda_stream)), "gcnn_lp_state")
            flags = outs[8].cpu().numpy()      # waits for the stream: the staging buffer is free again
        lpstate.raise_for_flags(flags)
        return tuple(outs[:7]) + (c, v, k), outs[7]


class _LPBatchSession(_Staging):
    """Host side of gcnn_lp_batch: one C call for up to 64 LP snapshots -- one upload of the tables and the packed snapshots, the
    states built in the arena where gcnn_infer_batch keeps its uploaded ones, one download.  `run` answers per snapshot, in STATE
    order: ("ok", scores, order, n_kept, cut_index), ("error", ValueError) for what the device flags in the snapshot,
    ("bad_index",) or ("declined",)."""
    MAX = _lib.IBATCH_MAX
    CAP = 64

    def __init__(self, model):
        super().__init__(model)
        self.calls = 0            # C calls made (tools and tests read it)
        self.deep_check = False   # as _LPSession.deep_check

    def check(self, snap):
        """-> (arrays, dims) of `lpstate.check_snapshot`."""
        from . import lpstate
        return lpstate.check_snapshot(snap, self.deep_check)

    @staticmethod
    def _dims_array(dims):
        return (_lib.LpDims * len(dims))(*(_lib.LpDims(**d) for d in dims))

    @staticmethod
    def _one(dims):
        from . import lpstate
        return list(lpstate.lp_layout(dims)[1].snap_off)

    def _entry(self, dims, fshapes, nf, nfe, L, **more):
        """A layout entry: the forced counts, the layout `L` (an `LpBatchLayout`) and what the packer and the reader derive from
        it -- where every array of every snapshot goes, the offsets of the states' cuts and forced rows, the built states' keys."""
        from . import lpstate
        base = list(L.snap_base)
        snap_at = [[base[s] + o for o in self.cached(("one",) + _int_key(d), self._one, d)] for s, d in enumerate(dims)]
        f_off, fe_off = (prefix(f[j] for f in fshapes) for j in (0, 1))
        return SimpleNamespace(nf=nf, nfe=nfe, L=L, snap_at=snap_at, k_off=prefix(d["n_cuts"] for d in dims), f_off=f_off, fe_off=fe_off,
                               forced_off=list(L.forced_off), out_off=list(L.out_off), keys=[lpstate.state_key(d) for d in dims], **more)

    def _layout(self, dims, fshapes, mode):
        nf, nfe = forced_counts(fshapes)
        L = _lib.LpBatchLayout()
        if _unsupported(_lib.lib().gcnn_lp_batch_layout_for(len(dims), self._dims_array(dims), nf, nfe, mode, C.byref(L)),
                        "gcnn_lp_batch_layout_for"):
            return False
        return self._entry(dims, fshapes, nf, nfe, L)

    def _pack(self, lay, checked, forced, mode, fill, *model_args):
        """The upload of one call into the pinned buffer: the tables (written by the library's `fill`, gcnn_lp_batch_fill_table or
        its twin for several models, which takes `model_args` behind the mode), every snapshot, the forced rows.  Returns the
        call's array of dims (the scalars are not part of the layout's key: the array is this call's)."""
        from . import lpstate
        d = self._dims_array([dims for _, dims in checked])
        self._buffers(lay.L)
        _lib.check(getattr(_lib.lib(), fill)(len(checked), d, lay.nf, lay.nfe, mode, *model_args, self.pin_in.data_ptr()), fill)
        for (arrays, _), at in zip(checked, lay.snap_at):
            lpstate.pack_snapshot(self.in_np, at, arrays)
        self._put_forced_stacked(lay.forced_off, lay.f_off, lay.fe_off, forced)
        return d

    def _answers(self, lay, n, mode):
        """`_collect` on the download of a call with `lay`'s output block: every snapshot's answer with its cut_index, or the
        ValueError of what the device flags in the snapshot itself."""
        from . import lpstate
        out, out_off = self.out_np, lay.out_off

        def lp_part(s, lo, cuts):
            lpstate.raise_for_flags(out[out_off[4] + 16 * s:out_off[4] + 16 * s + 16].view(np.int32))
            return (out[out_off[5] + lo:out_off[5] + lo + 4 * cuts].view(np.int32).copy(),)

        return self._collect(out_off, lay.k_off, n, mode, lp_part)

    def run(self, checked, forced, mode, p_max=0.0, p_max_ub=0.0):
        """checked: [(arrays, dims)] as `check` returns them; forced: None or [(ptr, col, val)] per snapshot.
        Returns None when the library declines the union as a whole (too large: the caller splits it)."""
        n = len(checked)
        dims = [d for _, d in checked]
        fshapes = forced_shapes(forced)
        lay = self.cached((mode, tuple(_int_key(d) for d in dims), fshapes), self._layout, dims, fshapes, mode)
        if lay is False:
            return None
        d = self._pack(lay, checked, forced, mode, "gcnn_lp_batch_fill_table")
        self._enqueue_wait("gcnn_lp_batch", (n, d, lay.nf, lay.nfe, mode), (float(p_max), float(p_max_ub)))
        self.calls += 1
        self.last = (lay.L, lay.keys)
        return self._answers(lay, n, mode)

    def last_states(self):
        """The seven arrays of every state the last call built in the arena, as host arrays (tests compare them with gcnn_lp_state's)."""
        L, keys = self.last
        off = list(L.state.in_off)
        kinds = (torch.float32, torch.int32, torch.float32, torch.float32, torch.float32, torch.int32, torch.float32)
        at, out = [0] * 5, []
        for key in keys:
            c, v, k, e1, e2 = key
            shapes = ((c, 4), (2, e1), (e1, 1), (v, 14), (k, 6), (2, e2), (e2, 1))
            arrays = []
            for j, ((col, size), shape, dt) in enumerate(zip(_BatchSession.PLACES, shapes, kinds)):
                o = off[2 + j] + size * at[col]
                arrays.append(self.arena[o:o + 4 * shape[0] * shape[1]].view(dt).view(shape).cpu().numpy())
            out.append(tuple(arrays))
            at = [a + b for a, b in zip(at, key)]
        return out


class _LPModelsSession(_ModelsSession):
    """Host side of gcnn_lp_models: one C call for up to 64 LP snapshots of up to 8 models.  `_ModelsSession` over an
    `_LPBatchSession` (`base`: the LP batch session of one of the models; every model of the call lives on its device): that
    session's checks, packer, pinned buffers, arena and reader, plus the model arguments and the launch tables' staging buffer.
    `last_plan()` is `_ModelsSession`'s: the union lies at the same places of the arena whether it was uploaded or built there."""

    def _layout(self, dims, fshapes, mode, model_of):
        n, n_models = len(dims), model_of[-1] + 1
        nf, nfe = forced_counts(fshapes)
        mos = (C.c_int32 * n)(*model_of)
        ML = _lib.LpModelsLayout()
        if _unsupported(_lib.lib().gcnn_lp_models_layout_for(n, self.base._dims_array(dims), nf, nfe, mode, n_models, mos, C.byref(ML)),
                        "gcnn_lp_models_layout_for"):
            return False
        return self.base._entry(dims, fshapes, nf, nfe, ML.lp, ML=ML, mos=mos, n_models=n_models)

    def run(self, checked, forced, mode, model_of, models, p_max=0.0, p_max_ub=0.0):
        """checked, forced: as `_LPBatchSession.run` takes them, sorted by model; model_of, models: as `_ModelsSession.run` takes
        them.  Returns `_LPBatchSession.run`'s list, None when the library declines the union's sizes (the caller splits it) or
        UNSUPPORTED when it declines the call as a whole."""
        base, n = self.base, len(checked)
        dims = [d for _, d in checked]
        fshapes = forced_shapes(forced)
        lay = self.cached((mode, tuple(_int_key(d) for d in dims), fshapes, tuple(model_of)), self._layout, dims, fshapes, mode, model_of)
        if lay is False:
            return None
        d = base._pack(lay, checked, forced, mode, "gcnn_lp_models_fill_table", lay.n_models, lay.mos)
        self.staging, _ = base._pin(self.staging, None, lay.ML.models.table_bytes, 1 << 16)
        params = (C.c_void_p * lay.n_models)(*(m._flat.data_ptr() for m in models))
        if base._enqueue_wait("gcnn_lp_models", (n, d, lay.nf, lay.nfe, mode, lay.n_models, lay.mos),
                              (C.c_void_p(self.staging.data_ptr()), float(p_max), float(p_max_ub)), params=params, may_decline=True):
            return self.UNSUPPORTED
        self.calls += 1
        self.last = (lay.ML.models, n)
        base.last = (lay.L, lay.keys)      # the arena holds this call's states, at the places `base.last_states` reads
        return base._answers(lay, n, mode)

    def last_states(self):
        """The seven arrays of every state the last call built in the arena (`_LPBatchSession.last_states`)."""
        return self.base.last_states()


class _EnsembleSession:
    """Host side of gcnn_infer_ensemble: one C call for ONE host state scored by up to 8 models -- the state goes up once, whatever
    the number of models.  It packs with a `_BatchSession`'s packer into that session's pinned buffers and arena (`base`: the batch
    session of one of the models; every model of the call lives on its device) and adds the pinned staging buffer of the grouped
    forward passes' launch tables.  `calls`: C calls made; `upload_bytes`: bytes of state uploads they made (the launch tables,
    the call's second copy, are not counted) -- tests and tools read both."""
    MAX_MODELS = _lib.GROUP_MAX
    CAP = _BatchSession.CAP
    cached = _Staging.cached          # the same bounded cache of layouts

    def __init__(self, base):
        self.base = base
        self.layouts = {}
        self.staging = None
        self.calls = 0
        self.upload_bytes = 0

    @staticmethod
    def _counts(fshape, mode):
        return (int(fshape[0]), int(fshape[1])) if mode == _lib.IBATCH_SELECT else (0, 0)

    def _layout(self, key, fshape, mode, n_models):
        dims = (_lib.Dims * 1)(_lib.Dims(*key))
        f, fe = self._counts(fshape, mode)
        EL = _lib.EnsembleLayout()
        if _unsupported(_lib.lib().gcnn_infer_ensemble_layout_for(dims, f, fe, mode, n_models, C.byref(EL)), "gcnn_infer_ensemble_layout_for"):
            return False
        nf, nfe = forced_counts(((f, fe),))
        table = np.zeros(_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE, np.int32)
        _lib.check(_lib.lib().gcnn_infer_batch_fill_table(1, dims, nf, nfe, table.ctypes.data), "gcnn_infer_batch_fill_table")
        cols = table.reshape(_lib.IBATCH_TABLE_COLS, _lib.IBATCH_TABLE_STRIDE)[:, :2].tolist()
        return _BatchSession._entry(dims, nf, nfe, EL.u, table, cols, EL=EL, counts=(f, fe), n_cuts=key[2])

    def _call(self, name, lay, head, mode, models, p_max, p_max_ub, timings, t0):
        """The C call `name` on what lies packed in the base session's buffers; True where the library declines it."""
        base = self.base
        self.staging, _ = base._pin(self.staging, None, lay.EL.table_bytes, 1 << 16)
        params = (C.c_void_p * len(models))(*(m._flat.data_ptr() for m in models))
        nbytes = int(lay.L.in_bytes)
        if base._enqueue_wait(name, (*head, *lay.counts, mode, len(models)), (C.c_void_p(self.staging.data_ptr()), float(p_max), float(p_max_ub)),
                              timings, t0, params=params, may_decline=True, upload_bytes=nbytes):
            return True
        self.calls += 1
        self.upload_bytes += nbytes
        base.last = None              # the arena no longer holds that session's own plan
        return False

    def _answer(self, lay, mode, n_models):
        """(mean, order | None, n_kept | None, members [M, K]) of the download; the flag policy as exceptions."""
        base, out_off, n = self.base, lay.out_off, lay.n_cuts
        verdict = base._verdict(out_off[3])
        if verdict == "bad_index":
            raise ValueError(BAD_INDEX)
        if verdict:
            raise _UseGeneralPath()
        mean, order, n_kept = base._read(out_off[0], out_off[1] if mode else None, out_off[2] if mode == _lib.IBATCH_SELECT else None, n)
        at, stride = int(lay.EL.member_off), int(lay.EL.member_stride)
        members = np.stack([base.out_np[at + m * stride:at + m * stride + 4 * n].view(np.float32) for m in range(n_models)])
        return mean, order, n_kept, members

    def run(self, inputs, forced, mode, models, p_max=0.0, p_max_ub=0.0, timings=None):
        """inputs: the model's 10-tuple of host arrays; forced: packed (ptr, col, val), read in selection mode only; models: the
        `GCNN`s in the ensemble's order.  Returns (mean, order | None, n_kept | None, members); raises _UseGeneralPath for what
        the call declines and ValueError for an index out of range."""
        t0 = time.perf_counter()
        arrays, key = check_state(inputs)
        if edges_without_nodes(key):
            raise ValueError(BAD_INDEX)
        fshape = (forced[0].size - 1, forced[1].size) if mode == _lib.IBATCH_SELECT else (0, 0)
        lay = self.cached((mode, key, fshape, len(models)), self._layout, key, fshape, mode, len(models))
        if lay is False:
            raise _UseGeneralPath()
        self.base._pack(lay, [(arrays, key)], [forced] if mode == _lib.IBATCH_SELECT else None)
        if self._call("gcnn_infer_ensemble", lay, (lay.dims,), mode, models, p_max, p_max_ub, timings, t0):
            raise _UseGeneralPath()
        return self._answer(lay, mode, len(models))


class _LPEnsembleSession(_EnsembleSession):
    """Host side of gcnn_lp_ensemble: `_EnsembleSession` over an `_LPBatchSession` (`base`) -- one upload of the packed snapshot,
    the state built once in the arena.  The library writes the call's tables into the pinned upload itself."""

    def _layout(self, dims, fshape, mode, n_models):
        f, fe = self._counts(fshape, mode)
        L = _lib.LpEnsembleLayout()
        if _unsupported(_lib.lib().gcnn_lp_ensemble_layout_for(C.byref(_lib.LpDims(**dims)), f, fe, mode, n_models, C.byref(L)),
                        "gcnn_lp_ensemble_layout_for"):
            return False
        return self.base._entry([dims], ((f, fe),), None, None, L.lp, EL=L.ens, counts=(f, fe), n_cuts=dims["n_cuts"])

    def run(self, snap, forced, mode, models, p_max=0.0, p_max_ub=0.0, timings=None):
        """`_EnsembleSession.run` from an `LPSnapshot`: (mean, order | None, n_kept | None, members, cut_index), in STATE order."""
        from . import lpstate
        t0 = time.perf_counter()
        base = self.base
        arrays, dims = base.check(snap)
        select = mode == _lib.IBATCH_SELECT
        fshape = (forced[0].size - 1, forced[1].size) if select else (0, 0)
        lay = self.cached((mode, _int_key(dims), fshape, len(models)), self._layout, dims, fshape, mode, len(models))
        if lay is False:
            raise _UseGeneralPath()
        base._buffers(lay.L)
        lpstate.pack_snapshot(base.in_np, lay.snap_at[0], arrays)
        base._put_forced_stacked(lay.forced_off, lay.f_off, lay.fe_off, [forced] if select else None)
        d = _lib.LpDims(**dims)
        if self._call("gcnn_lp_ensemble", lay, (C.byref(d),), mode, models, p_max, p_max_ub, timings, t0):
            raise _UseGeneralPath()
        base.last = (lay.L, lay.keys)      # the arena holds this call's state, at the places `base.last_states` reads
        out, out_off, n = base.out_np, lay.out_off, lay.n_cuts
        lpstate.raise_for_flags(out[out_off[4]:out_off[4] + 16].view(np.int32))
        return self._answer(lay, mode, len(models)) + (out[out_off[5]:out_off[5] + 4 * n].view(np.int32).copy(),)


class _EnsembleBatchSession(_EnsembleSession):
    """Host side of gcnn_infer_ensemble_batch: one C call for up to 64 host states scored by ONE ensemble of up to 8 models -- the
    states go up once as gcnn_infer_batch's union, whatever the number of models.  `_EnsembleSession` over the same `_BatchSession`
    (`base`: its packer, pinned buffers and arena).  `run` answers per state as `_BatchSession.run` does, an "ok" answer carrying the
    mean as its scores and the members' rows [M, K_s] last.  `calls`, `upload_bytes`: as `_EnsembleSession`; `max_states_per_call`:
    the most states one call served."""
    MAX = _lib.IBATCH_MAX
    ENTRY = "gcnn_infer_ensemble_batch"

    def __init__(self, base):
        super().__init__(base)
        self.max_states_per_call = 0

    def _layout(self, keys, fshapes, mode, n_models):
        n = len(keys)
        dims = (_lib.Dims * n)(*(_lib.Dims(*k) for k in keys))
        nf, nfe = forced_counts(fshapes)
        EL = _lib.EnsembleLayout()
        if _unsupported(_lib.lib().gcnn_infer_ensemble_batch_layout_for(n, dims, nf, nfe, mode, n_models, C.byref(EL)),
                        "gcnn_infer_ensemble_batch_layout_for"):
            return False
        table = np.zeros(_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE, np.int32)
        _lib.check(_lib.lib().gcnn_infer_batch_fill_table(n, dims, nf, nfe, table.ctypes.data), "gcnn_infer_batch_fill_table")
        cols = table.reshape(_lib.IBATCH_TABLE_COLS, _lib.IBATCH_TABLE_STRIDE)[:, :n + 1].tolist()
        return _BatchSession._entry(dims, nf, nfe, EL.u, table, cols, EL=EL, counts=(), k_off=cols[2])

    def _finish(self, got, lay, n, n_models):
        """The call's answers with every "ok" state's member rows [M, K_s] appended, read from the same download."""
        at, stride, out = int(lay.EL.member_off), int(lay.EL.member_stride), self.base.out_np
        for s, r in enumerate(got):
            if r[0] == "ok":
                lo, hi = at + 4 * lay.k_off[s], at + 4 * lay.k_off[s + 1]
                got[s] = r + (np.stack([out[lo + m * stride:hi + m * stride].view(np.float32) for m in range(n_models)]),)
        self.max_states_per_call = max(self.max_states_per_call, n)
        return got

    def run(self, checked, forced, mode, models, p_max=0.0, p_max_ub=0.0):
        """checked, forced: as `_BatchSession.run` takes them; models: the `GCNN`s in the ensemble's order.  Returns per state
        ("ok", mean, order, n_kept, members), ("bad_index",) or ("declined",); every state ("declined",) where the library declines
        the call as a whole; None where it declines the union's sizes (the caller splits it)."""
        n = len(checked)
        keys = tuple(k for _, k in checked)
        fshapes = forced_shapes(forced) if mode == _lib.IBATCH_SELECT else ()
        lay = self.cached((mode, keys, fshapes, len(models)), self._layout, keys, fshapes, mode, len(models))
        if lay is False:
            return None
        self.base._pack(lay, checked, forced if mode == _lib.IBATCH_SELECT else None)
        if self._call(self.ENTRY, lay, (n, lay.dims, lay.nf, lay.nfe), mode, models, p_max, p_max_ub, None, 0.0):
            return [("declined",)] * n
        return self._finish(self.base._collect(lay.out_off, lay.k_off, n, mode), lay, n, len(models))


class _LPEnsembleBatchSession(_EnsembleBatchSession):
    """Host side of gcnn_lp_ensemble_batch: `_EnsembleBatchSession` over an `_LPBatchSession` (`base`) -- one upload of the packed
    snapshots, every state built once in the arena.  The library writes the call's tables into the pinned upload itself.  An "ok"
    answer is ("ok", mean, order, n_kept, cut_index, members), in STATE order."""
    ENTRY = "gcnn_lp_ensemble_batch"

    def _layout(self, dims, fshapes, mode, n_models):
        nf, nfe = forced_counts(fshapes)
        L = _lib.LpEnsembleLayout()
        if _unsupported(_lib.lib().gcnn_lp_ensemble_batch_layout_for(len(dims), self.base._dims_array(dims), nf, nfe, mode, n_models,
                                                                     C.byref(L)), "gcnn_lp_ensemble_batch_layout_for"):
            return False
        return self.base._entry(dims, fshapes, nf, nfe, L.lp, EL=L.ens, counts=())

    def run(self, checked, forced, mode, models, p_max=0.0, p_max_ub=0.0):
        """checked: [(arrays, dims)] as `_LPBatchSession.check` returns them; otherwise as `_EnsembleBatchSession.run`, with
        ("error", ValueError) for what the device flags in a snapshot itself."""
        from . import lpstate
        base, n = self.base, len(checked)
        dims = [d for _, d in checked]
        select = mode == _lib.IBATCH_SELECT
        fshapes = forced_shapes(forced) if select else ()
        lay = self.cached((mode, tuple(_int_key(d) for d in dims), fshapes, len(models)), self._layout, dims, fshapes, mode, len(models))
        if lay is False:
            return None
        base._buffers(lay.L)
        for (arrays, _), at in zip(checked, lay.snap_at):
            lpstate.pack_snapshot(base.in_np, at, arrays)
        base._put_forced_stacked(lay.forced_off, lay.f_off, lay.fe_off, forced if select else None)
        if self._call(self.ENTRY, lay, (n, base._dims_array(dims), lay.nf, lay.nfe), mode, models, p_max, p_max_ub, None, 0.0):
            return [("declined",)] * n
        base.last = (lay.L, lay.keys)      # the arena holds this call's states, at the places `base.last_states` reads
        return self._finish(base._answers(lay, n, mode), lay, n, len(models))


class LPSession(_Staging):
    """An LP resident on the device across the separation rounds of one node (`GCNN.open_lp`): the rows, `col_type` and `col_obj`
    go up once, what depends on them alone -- the constraint features' static half, the constraint edges and both their CSR
    orders -- is built once (gcnn_lp_rows_build + gcnn_graph_build), and a round (`lpstate.LPRound`) uploads only the solve and
    the candidate cuts (gcnn_lp_round / gcnn_lp_round_select: one upload, two state launches, the forward pass, one download).
    A round's result is by definition what `state_from_lp` / `score_lp` / `select_cuts_lp` give on
    `lpstate.assemble(rows, round)`, bit for bit.  Rows can be appended and removed -- inside a round's own call (`append=` /
    `remove=` of `select_cuts`, `score`, `state`: gcnn_lp_round_append derives only the new rows and copies, shifts and merges the
    resident arrays into the session's other set of buffers; gcnn_lp_round_remove derives nothing: it compacts the resident arrays
    and the raw rows into the other sets, with an append behind it in the same call) or on their own (`append_rows`,
    `remove_rows`).  `remove` numbers the rows AFTER the append of the same call, in any order; the round's `row_dual` and
    `row_basis` cover the kept rows in their order; a removal that would leave no row at all is refused (open a new session).
    Either edit is all or nothing: if the call raises, the session holds exactly the rows and derived state it held.  Not
    covered: any other change of the LP -- a row changed, a column added, another objective -- which means opening a new
    session.  There is no variable limit; an order
    (ranking on the device, selection) takes at most 4,096 cuts, a table at most 2^24 rows.  The session holds no parameters:
    every round reads the model's current flat parameter buffer.  After a rejected round (ValueError, GcnnError) the session
    stays usable and the next round sees nothing of the rejected one."""
    GUARD = 0                 # bytes of guard in front of and behind every device buffer of the session (tests set it)
    GUARD_BYTE = 0xA5

    def __init__(self, model, rows, deep=True):
        from . import lpstate
        super().__init__(model)
        self.deep_check = bool(deep)
        self._buffers_made = []           # (whole tensor, payload bytes) of every guarded buffer alive
        arrays, dims = lpstate.check_rows(rows, self.deep_check)
        self._dims = dims                 # the resident rows' dims: what a round's dims start from
        self._raw = None                  # device: row_ptr, row_col, row_val, row_lhs, row_rhs (capacity >= the resident counts)
        self._cap = (0, 0)
        self._kept = {}                   # host copies of the optional column arrays as the last accepted rounds gave them
        self._stale = set()               # optional arrays whose device copy a rejected round overwrote
        self._derived = self._graph = self._res = None
        self._cur = self._cur_struct = None     # {name: device tensor} of `_lib.LP_SET_FIELDS`: the derived arrays the rounds read
        self._cur_set = -1                # which of `_sets` they are; -1: the rebuild's own block and graph
        self._sets = [None, None]         # the two sets an incremental append alternates between: ({name: tensor}, (capR, capC, capE), structs)
        self._lhs = (0, 0)                # lhs-sided state rows and their entries: where an appended lhs row goes
        self._col_deg = np.zeros(dims["n_cols"], np.int64)      # listed entries per column, and the longest segments: kept on the host
        self._max_deg = (0, 0)
        self._book = None                 # per resident row: entry count, side bits; a copy of row_col (`lpstate.row_book`): a removal's exact account
        self._raw_alt, self._cap_alt = None, (0, 0)     # the second set of raw buffers: a removal compacts the raw rows into it
        self._transit = [None]            # the third set of derived buffers: between the removal and the append of one call
        self.closed = False
        V = dims["n_cols"]
        dev = model.device
        with torch.cuda.device(dev):
            self._col_type = self._alloc(V)
            self._col_obj = self._alloc(8 * V)
            self._opt = [self._alloc(8 * V) for _ in lpstate.OPTIONAL]
            self._col_type[:V].copy_(torch.from_numpy(arrays[5].view(np.uint8)))
            self._col_obj[:8 * V].copy_(torch.from_numpy(arrays[6].view(np.uint8)))
        self._dims = dict(dims, n_rows=0, row_nnz=0, n_state_rows=0, n_state_edges=0)
        self._append(arrays[:5], (dims["n_rows"], dims["row_nnz"], dims["n_state_rows"], dims["n_state_edges"]), first=True)

    # ---- device buffers ----------------------------------------------------------------------------------------------------------
    def _alloc(self, nbytes):
        """A device uint8 tensor of `nbytes` (at least 16); with GUARD set it lies between two guard blocks of GUARD_BYTE."""
        n, g = max(int(nbytes), 16), self.GUARD
        if not g:
            return torch.empty(n, dtype=torch.uint8, device=self.model.device)
        whole = torch.full((n + 2 * g,), self.GUARD_BYTE, dtype=torch.uint8, device=self.model.device)
        self._buffers_made.append((weakref.ref(whole), n))      # (the payload view keeps `whole` alive for as long as it is in use)
        return whole[g:g + n]

    def guards_intact(self):
        """True when no guard byte of a live buffer of the session (resident buffers and the round arena) has changed."""
        g = self.GUARD
        live = [(ref(), n) for ref, n in self._buffers_made if ref() is not None]
        return all(bool((w[:g] == self.GUARD_BYTE).all()) and bool((w[g + n:] == self.GUARD_BYTE).all()) for w, n in live)

    def _buffers(self, L):
        self.pin_in, self.in_np = self._pin(self.pin_in, self.in_np, L.in_bytes, 1 << 20)
        self.pin_out, self.out_np = self._pin(self.pin_out, self.out_np, L.out_bytes, 1 << 16)
        if self.arena is None or self.arena.numel() < L.arena_bytes:
            self.arena = None
            self.arena = self._alloc(max(2 * L.arena_bytes, 1 << 22))

    # ---- rows --------------------------------------------------------------------------------------------------------------------
    @property
    def n_rows(self):
        return self._dims["n_rows"]

    @property
    def n_cols(self):
        return self._dims["n_cols"]

    def append_rows(self, row_ptr, row_col, row_val, row_lhs, row_rhs, incremental=False):
        """Append rows (CSR over the same columns, `row_ptr` from 0) behind the resident ones: only they are uploaded.  By default
        what is derived from the rows is then rebuilt on the device (an appended lhs-sided row moves every rhs-sided state row
        behind it); with `incremental` only the new rows are derived and the resident arrays are copied, shifted and merged into
        the session's other set of buffers (gcnn_lp_rows_append), with one read of the flag words.  The resident state is the same
        either way, bit for bit.  Appending zero rows is a no-op."""
        from . import lpstate
        self._open()
        arrays, counts = lpstate.check_row_block(row_ptr, row_col, row_val, row_lhs, row_rhs, self.n_cols, self._dims["infinity"],
                                                 self.deep_check)
        if counts[0] == 0:
            return
        if incremental:
            self._append_incremental(arrays, counts)
        else:
            self._append(arrays, counts, first=False)

    def _grow_raw(self, R, N):
        """Room for R rows and N entries in the raw buffers: amortised doubling, device to device: no resident row goes up again."""
        old = self._dims
        capR, capN = self._cap
        if self._raw is None or R > capR or N > capN:
            capR, capN = max(R, 2 * capR if R > capR else capR), max(N, 2 * capN if N > capN else capN)
            new = [self._alloc(4 * (capR + 1)), self._alloc(4 * capN), self._alloc(8 * capN), self._alloc(8 * capR), self._alloc(8 * capR)]
            if self._raw is not None:
                used = (4 * (old["n_rows"] + 1), 4 * old["row_nnz"], 8 * old["row_nnz"], 8 * old["n_rows"], 8 * old["n_rows"])
                for dst, src, n in zip(new, self._raw, used):
                    dst[:n].copy_(src[:n])
            self._raw, self._cap = new, (capR, capN)

    def _upload_block(self, arrays, first):
        """The block into the tail of the raw buffers (enqueued; `row_ptr` shifted to the resident entries)."""
        from . import lpstate
        old = self._dims
        dR, dN = arrays[3].shape[0], arrays[1].shape[0]
        _, total = lpstate.rows_upload_layout(dR, dN, first)
        self.pin_in, self.in_np = self._pin(self.pin_in, self.in_np, total, 1 << 20)
        places = lpstate.pack_row_block(self.in_np, arrays, old["row_nnz"], first)
        at = (4 * (old["n_rows"] + (0 if first else 1)), 4 * old["row_nnz"], 8 * old["row_nnz"], 8 * old["n_rows"], 8 * old["n_rows"])
        for dst, (off, n), to in zip(self._raw, places, at):
            if n:
                dst[to:to + n].copy_(self.pin_in[off:off + n], non_blocking=True)

    def _after(self, counts, old=None):
        """The resident dims (`old`: dims to start from instead) after a block of `counts`; ValueError where the sums leave int32."""
        dR, dN, dC, dE = counts
        old = self._dims if old is None else old
        R, N = old["n_rows"] + dR, old["row_nnz"] + dN
        if old["n_state_edges"] + dE > 2 ** 31 - 1 or N > 2 ** 31 - 1:
            raise ValueError("the state's constraint edges do not fit int32")
        return dict(old, n_rows=R, row_nnz=N, n_state_rows=old["n_state_rows"] + dC, n_state_edges=old["n_state_edges"] + dE)

    def _host_counts(self, arrays, base=None):
        """What the host keeps of the resident state once `arrays` are part of it: (lhs rows, lhs entries), the per-column
        degrees' update, the longest segments -- exact, without a device read -- and the arrays, for the rows' book.  `base`:
        (col_deg, max_deg) to start from instead of the session's (a removal in front of the block)."""
        from . import lpstate
        col_deg, max_deg = (self._col_deg, self._max_deg) if base is None else base
        dL, dEL, longest, (cols, counts) = lpstate.block_sides(arrays, self.n_cols, self._dims["infinity"])
        v_max = max(max_deg[1], int((col_deg[cols] + counts).max())) if cols.size else max_deg[1]
        return (dL, dEL), (cols, counts), (max(max_deg[0], longest), v_max), arrays

    def _adopt_counts(self, host):
        from . import lpstate
        (dL, dEL), (cols, counts), self._max_deg, arrays = host
        self._lhs = (self._lhs[0] + dL, self._lhs[1] + dEL)
        self._col_deg[cols] += counts
        new = lpstate.row_book(arrays, self._dims["infinity"])
        self._book = new if self._book is None else tuple(np.concatenate(pair) for pair in zip(self._book, new))

    def _append(self, arrays, counts, first):
        dims = self._after(counts)
        host = self._host_counts(arrays)
        with torch.cuda.device(self.model.device):
            self._grow_raw(dims["n_rows"], dims["row_nnz"])
            self._upload_block(arrays, first)
            self._rebuild(dims)         # raises for rows the device flags: the session then keeps the rows it had
        self._adopt_counts(host)

    def _rebuild(self, dims):
        """gcnn_lp_rows_build + gcnn_graph_build on the raw rows for `dims`; adopts both (and `dims`) once the device has accepted
        the rows.  Synchronises: the flags and the longest segments come home here, so that no round has to wait for them."""
        from . import lpstate
        from .graph import BipartiteGraph
        d, L, P = _lib.LpDims(**dims), _lib.LpRowsLayout(), C.c_void_p
        _lib.check(_lib.lib().gcnn_lp_rows_layout_for(C.byref(d), C.byref(L)), "gcnn_lp_rows_layout_for")
        dev = self.model.device
        derived = self._alloc(L.bytes)
        off = list(L.off)
        stream = torch.cuda.current_stream(dev)
        _lib.check(_lib.lib().gcnn_lp_rows_build(C.byref(d), *(P(t.data_ptr()) for t in self._raw), P(self._col_obj.data_ptr()),
                                                 P(derived.data_ptr()), derived.numel(), P(stream.cuda_stream)), "gcnn_lp_rows_build")
        flags = derived[off[5]:off[5] + 16].view(torch.int32).cpu().numpy()      # waits: the staging buffer is free again
        lpstate.raise_for_flags(flags)
        c, e1 = dims["n_state_rows"], dims["n_state_edges"]
        inds = derived[off[1]:off[1] + 8 * e1].view(torch.int32).view(2, e1)
        feats = derived[off[2]:off[2] + 4 * e1].view(torch.float32)
        graph = BipartiteGraph(inds, feats, c, dims["n_cols"], validate=False, sync_max_degree=True)
        res = _lib.LpResident(derived.data_ptr() + off[3], derived.data_ptr() + off[4], derived.data_ptr() + off[0],
                              self._col_type.data_ptr(), self._col_obj.data_ptr(), *(t.data_ptr() for t in self._opt), graph.c)
        u8 = lambda t: t.view(torch.uint8)
        cur = dict(cons_feats=derived[off[0]:], edge_row=derived[off[1]:], edge_col=derived[off[1] + 4 * e1:], edge_coef=derived[off[2]:],
                   l_ptr=u8(graph.l_ptr), v_ptr=u8(graph.v_ptr), v_oth=u8(graph.v_oth), v_coef=u8(graph.v_coef),
                   row_place=derived[off[3]:], row_scale=derived[off[4]:])
        self._derived, self._graph, self._res, self._dims = derived, graph, res, dims
        self._cur, self._cur_struct, self._cur_set = cur, self._set_struct(cur), -1
        self.layouts.clear()

    # ---- the incremental append ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _set_struct(cur):
        return _lib.LpRowsSet(*(cur[name].data_ptr() if cur[name].numel() else 0 for name in _lib.LP_SET_FIELDS))

    def _other_set(self, dims, max_deg):
        """(index, tensors, gcnn_lp_rows_set, gcnn_lp_resident) of the set of derived buffers an append into `dims` writes: the one
        the rounds do not read, with room for `dims`.  One that is too small is replaced by one of twice the size needed, on
        the device; nothing is copied, an append writes every array whole.  The two structs are made once per allocation; only
        the longest segments change from append to append."""
        i = 1 - self._cur_set if self._cur_set >= 0 else 0
        self._sets[i] = held = self._fit_set(self._sets, i, dims)
        res = held[3]
        res.cons_graph.l_max_deg, res.cons_graph.v_max_deg = max_deg
        return i, held[0], held[2], res

    def _fit_set(self, slots, i, dims):
        """`slots[i]` -- (tensors, capacities, gcnn_lp_rows_set, gcnn_lp_resident) -- with room for `dims`: as it is, or replaced."""
        need = (dims["n_rows"], dims["n_state_rows"], dims["n_state_edges"])
        held = slots[i]
        if held is None or any(n > c for n, c in zip(need, held[1])):
            cap = tuple(2 * n if n > c else c for n, c in zip(need, held[1] if held else (0, 0, 0)))
            slots[i] = held = None
            capR, capC, capE = cap
            sizes = dict(cons_feats=16 * capC, edge_row=4 * capE, edge_col=4 * capE, edge_coef=4 * capE, l_ptr=4 * (capC + 1),
                         v_ptr=4 * (dims["n_cols"] + 1), v_oth=4 * capE, v_coef=4 * capE, row_place=8 * capR, row_scale=8 * capR)
            cur = {name: self._alloc(sizes[name]) for name in _lib.LP_SET_FIELDS}
            p = {name: t.data_ptr() for name, t in cur.items()}
            res = _lib.LpResident(p["row_place"], p["row_scale"], p["cons_feats"], self._col_type.data_ptr(), self._col_obj.data_ptr(),
                                  *(t.data_ptr() for t in self._opt),
                                  _lib.Graph(p["l_ptr"], p["edge_col"], p["edge_coef"], p["v_ptr"], p["v_oth"], p["v_coef"], 0, 0))
            held = (cur, cap, self._set_struct(cur), res)
        return held

    def _block_dims(self, counts, host, lhs=None):
        return counts + host[0] + (self._lhs if lhs is None else lhs)

    def _adopt_set(self, i, cur, struct, dims, host, res):
        self._cur, self._cur_struct, self._cur_set, self._dims, self._res = cur, struct, i, dims, res
        self._derived = self._graph = None          # the rebuild's block, if the rounds read it until now
        self._adopt_counts(host)
        self.layouts.clear()

    def _append_incremental(self, arrays, counts):
        from . import lpstate
        dims = self._after(counts)
        host = self._host_counts(arrays)
        P = C.c_void_p
        dev = self.model.device
        with torch.cuda.device(dev):
            self._grow_raw(dims["n_rows"], dims["row_nnz"])
            i, dst, dst_struct, res = self._other_set(dims, host[2])
            d, b, L = lpstate.lp_append_layout(self._dims, self._block_dims(counts, host), 0)
            if self.arena is None or self.arena.numel() < L.scratch_bytes + 256:
                self.arena = None
                self.arena = self._alloc(max(2 * (L.scratch_bytes + 256), 1 << 22))
            self._upload_block(arrays, False)
            flags_at = (L.scratch_bytes + 15) & ~15
            stream = torch.cuda.current_stream(dev)
            _lib.check(_lib.lib().gcnn_lp_rows_append(C.byref(d), C.byref(b), *(P(t.data_ptr()) for t in self._raw), P(self._col_obj.data_ptr()),
                                                      C.byref(self._cur_struct), C.byref(dst_struct), P(self.arena.data_ptr()),
                                                      L.scratch_bytes, P(self.arena.data_ptr() + flags_at),
                                                      P(stream.cuda_stream)), "gcnn_lp_rows_append")
            flags = self.arena[flags_at:flags_at + 16].view(torch.int32).cpu().numpy()      # the one read; waits
        lpstate.raise_for_flags(flags)
        self._adopt_set(i, dst, dst_struct, dims, host, res)

    # ---- the removal -------------------------------------------------------------------------------------------------------------
    def _raw_other(self, R, N):
        """The second set of raw buffers with room for R rows and N entries: a removal compacts the raw rows into it (out of
        place: the accepted rounds' raw rows are not written before the call is accepted).  Nothing is copied on growth."""
        capR, capN = self._cap_alt
        if self._raw_alt is None or R > capR or N > capN:
            if self._raw_alt is None:
                capR, capN = max(R, self._cap[0]), max(N, self._cap[1])
            else:
                capR, capN = max(R, 2 * capR if R > capR else capR), max(N, 2 * capN if N > capN else capN)
            self._raw_alt = None
            self._raw_alt = [self._alloc(4 * (capR + 1)), self._alloc(4 * capN), self._alloc(8 * capN), self._alloc(8 * capR), self._alloc(8 * capR)]
            self._cap_alt = (capR, capN)
        return self._raw_alt

    def _removal_host(self, idx, append):
        """The host half of removing the resident rows `idx` (ascending, checked), with `append` (a block, or None) behind it:
        the removed rows' eight counts, the dims after the removal and after the whole edit, the checked block and its eight
        counts, and what the host keeps of the rows once the call is accepted -- all exact, nothing of the session changes."""
        from . import lpstate
        six, book, col_deg, lhs, max_deg = lpstate.removal_counts(self._book, self._col_deg, self._lhs, idx)
        old = self._dims
        mid = dict(old, n_rows=old["n_rows"] - six[0], row_nnz=old["row_nnz"] - six[1], n_state_rows=old["n_state_rows"] - six[2],
                   n_state_edges=old["n_state_edges"] - six[3])
        e = SimpleNamespace(idx=idx.astype(np.int32), removed=six + self._lhs, mid=mid, final=mid, blk=None, block=None)
        if append is not None:
            e.blk = self._check_block(append, (mid, col_deg, max_deg))
        if e.blk is not None:
            arrays, counts, e.final, ((dL, dEL), (cols, add), max_deg, _) = e.blk
            e.block = counts + (dL, dEL) + lhs
            lhs = (lhs[0] + dL, lhs[1] + dEL)
            col_deg[cols] += add                    # (`removal_counts` made this copy)
            book = tuple(np.concatenate(pair) for pair in zip(book, lpstate.row_book(arrays, old["infinity"])))
        e.host = (lhs, col_deg, max_deg, book)
        return e

    def _adopt_removal(self, job):
        """The session after an accepted call with a removal: the destination sets become the current ones."""
        i, cur, struct, res = job.set
        e = job.rm
        self._cur, self._cur_struct, self._cur_set, self._dims, self._res = cur, struct, i, e.final, res
        self._derived = self._graph = None
        self._lhs, self._col_deg, self._max_deg, self._book = e.host
        self._raw, self._raw_alt, self._cap, self._cap_alt = e.raw_dst, self._raw, self._cap_alt, self._cap
        self.layouts.clear()

    def remove_rows(self, remove):
        """Remove the resident rows at the indices `remove` (any order; ValueError for an index that is not an integer, is out
        of range or given twice, and where no row would be left): nothing goes up but the list, nothing is derived -- the
        resident arrays and the raw rows are compacted into the session's other sets of buffers (gcnn_lp_rows_remove), with one
        read of the flag words.  The resident state is afterwards a fresh session's on the kept rows, bit for bit.  Removing
        zero rows is a no-op."""
        from . import lpstate
        self._open()
        idx, _ = lpstate.split_remove(remove, self.n_rows)
        if not idx.size:
            return
        e = self._removal_host(idx, None)
        P, dev = C.c_void_p, self.model.device
        job = SimpleNamespace(rm=e)
        with torch.cuda.device(dev):
            e.raw_dst = self._raw_other(e.final["n_rows"], e.final["row_nnz"])
            job.set = self._other_set(e.final, e.host[2])
            d, m, _, L = lpstate.lp_remove_layout(self._dims, e.removed, None, 0)
            flags_at = L.list_bytes + ((L.scratch_bytes + 255) & ~255)
            if self.arena is None or self.arena.numel() < flags_at + 256:
                self.arena = None
                self.arena = self._alloc(max(2 * (flags_at + 256), 1 << 22))
            n = 4 * e.idx.size
            self.pin_in, self.in_np = self._pin(self.pin_in, self.in_np, n, 1 << 20)
            self.in_np[:n] = e.idx.view(np.uint8)
            self.arena[:n].copy_(self.pin_in[:n], non_blocking=True)
            stream = torch.cuda.current_stream(dev)
            at = self.arena.data_ptr()
            _lib.check(_lib.lib().gcnn_lp_rows_remove(C.byref(d), C.byref(m), P(at), *(P(t.data_ptr()) for t in self._raw),
                                                      *(P(t.data_ptr()) for t in e.raw_dst), C.byref(self._cur_struct), C.byref(job.set[2]),
                                                      P(at + L.list_bytes), L.scratch_bytes, P(at + flags_at), P(stream.cuda_stream)),
                       "gcnn_lp_rows_remove")
            flags = self.arena[flags_at:flags_at + 16].view(torch.int32).cpu().numpy()      # the one read; waits
        lpstate.raise_for_flags(flags)
        self._adopt_removal(job)

    def resident_state(self):
        """Host copies of what the session holds of the rows, as the rounds read it: the ten derived arrays (`cons_feats` [C, 4]
        with the columns 1 and 3 as the last round left them), the longest segments and the sizes."""
        self._open()
        d, cur = self._dims, self._cur
        r, c, e, v = d["n_rows"], d["n_state_rows"], d["n_state_edges"], d["n_cols"]
        shape = dict(cons_feats=(torch.float32, 4 * c), edge_row=(torch.int32, e), edge_col=(torch.int32, e), edge_coef=(torch.float32, e),
                     l_ptr=(torch.int32, c + 1), v_ptr=(torch.int32, v + 1), v_oth=(torch.int32, e), v_coef=(torch.float32, e),
                     row_place=(torch.int32, 2 * r), row_scale=(torch.float64, r))
        out = {name: cur[name][:n * torch.empty(0, dtype=dt).element_size()].view(dt).cpu().numpy() for name, (dt, n) in shape.items()}
        out["cons_feats"] = out["cons_feats"].reshape(c, 4)
        out["row_place"] = out["row_place"].reshape(r, 2)
        g = self._res.cons_graph
        out.update(l_max_deg=int(g.l_max_deg), v_max_deg=int(g.v_max_deg), n_rows=r, n_state_rows=c, n_state_edges=e)
        return out

    # ---- rounds ------------------------------------------------------------------------------------------------------------------
    def _open(self):
        if self.closed:
            raise _lib.GcnnError("the LP session is closed")

    def _checked(self, rnd, n_forced=-1, n_entries=0, rm=None, blk=None):
        """A round checked on the host -> (arrays, presence mask, dims, layout record, the edits' counts).  An optional array whose
        device copy a rejected round overwrote travels again from the host copy of the last accepted one.  `rm`, `blk`: the
        round's edits (`_edit_host`); the round then covers the rows after them, and the layout is that of the call which
        carries them.  The counts: the removed rows' eight and the block's eight, each only where there is one."""
        from . import lpstate
        self._open()
        row_dims = block = removed = None
        if rm is not None:
            row_dims, block, removed = rm.final, rm.block, rm.removed
        elif blk is not None:
            row_dims, block = blk[2], self._block_dims(blk[1], blk[3])
        arrays, present, dims = lpstate.check_round(rnd, self._dims if row_dims is None else row_dims, self._kept, self.deep_check)
        for q, name in enumerate(lpstate.OPTIONAL):
            needed = not name.startswith("col_primal") or dims["has_incumbent"]
            if name in self._stale and needed and not present >> q & 1:
                arrays[5 + q] = self._kept[name]
                present |= 1 << q
        key = _int_key(dims) + (present, n_forced, n_entries) + (block or ()) + (("remove",) + removed if removed else ())
        before = dict(self._dims, n_cuts=dims["n_cuts"], cut_nnz=dims["cut_nnz"], has_incumbent=dims["has_incumbent"])
        lay = self.cached(key, self._edit_layout, before, removed, block, present, n_forced, n_entries)
        return arrays, present, dims, lay, (removed or ()) + (block or ())

    @staticmethod
    def _edit_layout(before, removed, block, present, n_forced, n_entries):
        """The layout record of a round with its edits, whichever library layout applies (gcnn_lp_remove_layout_for,
        gcnn_lp_append_layout_for, gcnn_lp_round_layout_for) for the dims BEFORE the edits: `L`, that layout (in_bytes, out_bytes,
        arena_bytes); the round's `in_off`, `forced_off` and `dev_off`, shifted to the whole upload and the whole arena, and its
        `out_off`; `block_off`, absolute; `flag_words`, where the download carries the flags of the removal, of the append and of
        the round, in that order; `d`, `m`, `b`, the ctypes dims of the call (`m`, `b`: None without that edit)."""
        from . import lpstate
        m = b = None
        if removed is not None:
            d, m, b, L = lpstate.lp_remove_layout(before, removed, block, present, n_forced, n_entries)
            R, up, arena = L.round, L.list_bytes + L.block_bytes, L.round_off
            flags = (int(L.flags_off),) + (() if b is None else (int(L.append_flags_off),))
        elif block is not None:
            d, b, L = lpstate.lp_append_layout(before, block, present, n_forced, n_entries)
            R, up, arena, flags = L.round, L.block_bytes, L.round_off, (int(L.flags_off),)
        else:
            d, L = lpstate.lp_round_layout(before, present, n_forced, n_entries)
            R, up, arena, flags = L, 0, 0, ()
        return SimpleNamespace(L=L, in_off=[up + o for o in R.in_off], forced_off=[up + o for o in R.forced_off], out_off=list(R.out_off),
                               dev_off=[arena + o for o in R.dev_off], block_off=() if b is None else tuple(L.block_off),
                               flag_words=flags + (R.out_off[4],), d=d, m=m, b=b)

    def _edit_host(self, append, remove):
        """The host half of a round's edits -> (rm, blk): `_removal_host`'s record where resident rows leave, or None; the checked
        block (`_check_block`), or None.  `remove` numbers the rows after the append: indices that point into the block are
        resolved here -- the rows are dropped from the block before it is checked -- so the device only sees removals of resident
        rows followed by an append of the filtered block.  Nothing of the session changes."""
        from . import lpstate
        if remove is not None:
            self._open()
            idx, append = lpstate.split_remove(remove, self.n_rows, append)
            if idx.size:
                rm = self._removal_host(idx, append)
                return rm, rm.blk
        return None, self._check_block(append) if append is not None else None

    def upload_bytes(self, rnd, forced=None, append=None, remove=None):
        """Bytes the one upload of this round would carry (with `forced`: packed forced rows of a selection; with `append`: the
        block that goes up with it; with `remove`: the list of removed resident rows, and the block without the rows it names)."""
        fshape = (-1, 0) if forced is None else (forced[0].size - 1, forced[1].size)
        return int(self._checked(rnd, *fshape, *self._edit_host(append, remove))[3].L.in_bytes)

    def _check_block(self, block, base=None):
        """An `LPRowBlock` checked on the host -> (arrays, counts, the resident dims after it, the host's counts); None for an
        empty block.  `base`: (dims, col_deg, max_deg) the block lands on instead of the session's (a removal in front of it)."""
        from . import lpstate
        self._open()
        arrays, counts = lpstate.check_row_block(*block.arrays(), self.n_cols, self._dims["infinity"], self.deep_check)
        if counts[0] == 0:
            return None
        if base is None:
            return arrays, counts, self._after(counts), self._host_counts(arrays)
        return arrays, counts, self._after(counts, base[0]), self._host_counts(arrays, base[1:])

    # A round's call in three parts, which the solo path (`_run`) and `LPSessionGroup` share: `_plan` (the host half: check,
    # layout, the buffers the edits write), `_pack` into a given staging buffer, then either `_enqueue` (the solo C call) or the
    # group's call, and `_finish` (the verdict half: the download's flags -> raise / adopt / remember).  A job has one shape: its
    # two optional edits `rm` (a removal of resident rows) and `blk` (a block appended behind it), each possibly None, and the round.
    def _plan(self, rnd, forced=None, append=None, remove=None):
        """check -> layout -> the buffers the edits write.  Returns the job the other parts read: `rm`, `blk`, the checked round,
        the fields of its layout record (`_edit_layout`), `block` (the edits' counts: what the layout depends on besides the
        dims) and `set` (the set of derived buffers the edits leave, or None).  Nothing of the session changes that a rejected
        round would have to undo: an append extends the raw rows behind the resident ones and writes the other of `_sets`; a
        removal reads the current sets and writes the second raw set and the other of `_sets`; with an append behind it the
        removal writes a transit set (allocated on the first such call, never the current one) and the append goes from there
        into the other of `_sets`, its rows behind the second raw set's.  Where no resident row is removed the job is the plain
        or the appending one, launch for launch."""
        job = SimpleNamespace(forced=forced, fshape=(-1, 0) if forced is None else (forced[0].size - 1, forced[1].size), set=None)
        job.rm, job.blk = rm, blk = self._edit_host(append, remove)
        job.arrays, job.present, job.dims, lay, job.block = self._checked(rnd, *job.fshape, rm, blk)
        vars(job).update(vars(lay))           # L, in_off, forced_off, out_off, dev_off, block_off, flag_words, d, m, b
        if rm is None and blk is None:
            return job
        final, max_deg = (blk[2], blk[3][2]) if rm is None else (rm.final, rm.host[2])
        with torch.cuda.device(self.model.device):
            if rm is None:
                self._grow_raw(final["n_rows"], final["row_nnz"])
            else:
                rm.raw_dst = self._raw_other(final["n_rows"], final["row_nnz"])
                rm.transit = None
                if blk is not None:
                    rm.transit = self._transit[0] = self._fit_set(self._transit, 0, rm.mid)
            job.set = self._other_set(final, max_deg)
        return job

    @staticmethod
    def _pack(job, buf):
        """The job's one upload into `buf` (a staging buffer, or a member's slice of a group's): the list of removed rows, the
        block, the round, the forced rows."""
        from . import lpstate
        if job.rm is not None:
            buf[:4 * job.rm.idx.size] = job.rm.idx.view(np.uint8)
        if job.blk is not None:
            for off, a in zip(job.block_off, job.blk[0]):
                if a.size:
                    buf[off:off + a.nbytes] = a.view(np.uint8)
        lpstate.pack_round(buf, job.in_off, job.arrays, job.present)
        if job.forced is not None:
            for off, a in zip(job.forced_off, job.forced):
                buf[off:off + a.nbytes] = a.view(np.uint8)

    def _enqueue(self, job, want_order, p_max, p_max_ub, timings, t0):
        """The solo call of a packed job and the wait for its download: of the four entry points the one the job's edits ask for."""
        P, e, d = C.c_void_p, job.rm, C.byref(job.d)
        tail = (int(want_order), float(p_max), float(p_max_ub))
        if e is not None or job.blk is not None:      # an edit: from the current sets into `set`, the round on what it leaves
            _, _, dst_struct, res = job.set
            raw, src, dst = tuple(P(t.data_ptr()) for t in self._raw), C.byref(self._cur_struct), (C.byref(dst_struct), C.byref(res))
        if e is not None:
            name = "gcnn_lp_round_remove"
            head = (d, C.byref(job.m), None if job.b is None else C.byref(job.b), job.present) + job.fshape + raw + tuple(
                P(t.data_ptr()) for t in e.raw_dst) + (src, None if e.transit is None else C.byref(e.transit[2])) + dst
        elif job.blk is not None:
            name, head = "gcnn_lp_round_append", (d, C.byref(job.b), job.present) + job.fshape + raw + (src,) + dst
        elif job.forced is not None:
            name, head, tail = "gcnn_lp_round_select", (d, job.present) + job.fshape + (C.byref(self._res),), tail[1:]
        else:
            name, head, tail = "gcnn_lp_round", (d, job.present, C.byref(self._res)), tail[:1]
        self._enqueue_wait(name, head, tail, timings, t0, upload_bytes=int(job.L.in_bytes))

    def _finish(self, job, out):
        """The verdict on a job's download block `out`: ValueError for a round or block the device flags (the session keeps the
        rows it held; the optional arrays the round gave count as stale), else the rows are adopted and the round's optional
        arrays remembered."""
        from . import lpstate
        given = {name: job.arrays[5 + q] for q, name in enumerate(lpstate.OPTIONAL) if job.present >> q & 1}
        try:
            for at in job.flag_words:
                lpstate.raise_for_flags(out[at:at + 16].view(np.int32))
        except ValueError:
            self._stale.update(given)       # their device copies hold the rejected round's values
            raise
        if job.rm is not None:
            self._adopt_removal(job)
        elif job.blk is not None:
            i, dst, dst_struct, res = job.set
            self._adopt_set(i, dst, dst_struct, job.blk[2], job.blk[3], res)
        self._kept.update(given)
        self._stale.difference_update(given)

    def _member(self, job, edit=False):
        """The job as a member of gcnn_lp_rounds, or with `edit` of gcnn_lp_rounds_edit, which also takes a job with a removal
        (the structs it points at live in the job and the session)."""
        m = _lib.LpRoundsEditMember() if edit else _lib.LpRoundsMember()
        m.dims, m.present, (m.n_forced, m.n_forced_entries) = job.d, job.present, job.fshape
        m.resident, m.params = C.pointer(self._res), self.model._flat.data_ptr()
        if job.set is not None:             # an edit: it reads the current sets and leaves `set`
            _, _, dst_struct, res = job.set
            m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs = (t.data_ptr() for t in self._raw)
            m.src, m.dst, m.resident = C.pointer(self._cur_struct), C.pointer(dst_struct), C.pointer(res)
        if job.b is not None:
            m.has_append, m.block = 1, job.b
        if job.rm is not None:
            m.has_remove, m.removed = 1, job.m
            m.out_ptr, m.out_col, m.out_val, m.out_lhs, m.out_rhs = (t.data_ptr() for t in job.rm.raw_dst)
            if job.rm.transit is not None:
                m.transit = C.pointer(job.rm.transit[2])
        return m

    def _run(self, rnd, want_order, timings=None, forced=None, p_max=0.0, p_max_ub=0.0, append=None, remove=None):
        """check -> layout -> pack -> one call -> the download's LP flags checked.  Returns (the round's dims, the download's
        offsets, the arena's offsets); what the round gave of the optional column arrays is remembered once it is accepted.
        With `append` the call is gcnn_lp_round_append: the block goes up with the round, the append's launches run in front of
        the round's, and the session adopts the rows once the download shows that the device accepted the block and the round.
        With `remove` (resident rows among the indices) the call is gcnn_lp_round_remove: the list goes up in front, the removal's
        launches run first, then the append's, then the round's."""
        t0 = time.perf_counter()
        job = self._plan(rnd, forced, append, remove)
        self._buffers(job.L)
        self._pack(job, self.in_np)
        self._enqueue(job, want_order, p_max, p_max_ub, timings, t0)
        self._finish(job, self.out_np)
        return job.dims, job.out_off, job.dev_off

    def state(self, rnd, append=None, remove=None):
        """The model's 10-tuple as host arrays and `cut_index`, as `GCNN.state_from_lp` gives them for the assembled snapshot
        (with `append`: the rows of the block appended first, in the same call; with `remove`: those rows removed then)."""
        dims, out_off, dev = self._run(rnd, -1, append=append, remove=remove)
        c, v, k, e1, e2 = dims["n_state_rows"], dims["n_cols"], dims["n_cuts"], dims["n_state_edges"], dims["cut_nnz"]
        f32, i32 = torch.float32, torch.int32
        cur, A = self._cur, self.arena

        def host(buf, off, shape, dt):
            return buf[off:off + 4 * shape[0] * shape[1]].view(dt).view(shape).cpu().numpy()

        inds = np.stack([host(cur["edge_row"], 0, (1, e1), i32)[0], host(cur["edge_col"], 0, (1, e1), i32)[0]])
        arrays = (host(cur["cons_feats"], 0, (c, 4), f32), inds, host(cur["edge_coef"], 0, (e1, 1), f32), host(A, dev[1], (v, 14), f32),
                  host(A, dev[2], (k, 6), f32), host(A, dev[3], (2, e2), i32), host(A, dev[4], (e2, 1), f32))
        return arrays + (c, v, k), self.out_np[out_off[5]:out_off[5] + 4 * k].view(np.int32).copy()

    def _results(self, dims, out_off, want_order, select, out=None):
        """(scores, order, n_kept, cut_index) of a round in the download block `out` (default: the session's own)."""
        n = dims["n_cuts"]
        out = self.out_np if out is None else out
        scores, order, n_kept = self._read(out_off[0], out_off[1] if want_order else None, out_off[3] if select else None, n, out)
        return scores, order, n_kept, out[out_off[5]:out_off[5] + 4 * n].view(np.int32).copy()

    def score(self, rnd, rank=False, timings=None, append=None, remove=None):
        """`GCNN.score_lp` for the assembled snapshot: a `ScoreArray` in STATE order with `.cut_index` and, with `rank`,
        `.rankings`.  `append` (an `lpstate.LPRowBlock`): rows appended in the same call, in front of the round, whose `row_dual`
        and `row_basis` cover them; all or nothing -- if the call raises, the session holds the rows it held before.  `remove`:
        indices of rows removed in the same call, numbered AFTER the append (a just-appended row may be removed), any order; the
        round covers the kept rows in their order: the answer is that of `lpstate.rows_without(rows_with(rows, append), remove)`."""
        n = int(np.asarray(rnd.cut_lhs).shape[0])
        on_device = self.model._rank_on_device(rank, n) and n <= 4096
        dims, out_off, _ = self._run(rnd, int(on_device), timings, append=append, remove=remove)
        scores, order, _, cut_index = self._results(dims, out_off, on_device, False)
        scores.cut_index = cut_index
        if rank:
            scores.rankings = order if on_device else stable_ranking(scores)
        return scores

    def select_cuts(self, rnd, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, timings=None, append=None, remove=None):
        """`GCNN.select_cuts_lp` for the assembled snapshot: a `SelectResult` with `cut_index`.  More than 4,096 cuts raise
        `GcnnError` before anything is enqueued.  `append`: as in `score` -- the separation loop's call, which appends the cuts
        the last selection kept and selects among the new candidates in one upload, one run of launches and one download.
        `remove`: as in `score` -- the rows the solver's clean-up dropped since the last round leave in the same call."""
        ops.check_thresholds(p_max, p_max_ub)
        self.model._check_select_size("LPSession.select_cuts", "round", int(np.asarray(rnd.cut_lhs).shape[0]))
        packed = normalize_forced(forced, self.n_cols)
        dims, out_off, _ = self._run(rnd, 1, timings, packed, p_max, p_max_ub, append=append, remove=remove)
        scores, order, n_kept, cut_index = self._results(dims, out_off, True, True)
        return SelectResult(order, n_kept, n_selected(n_kept, max_selected), scores, cut_index)

    def close(self):
        """Release the device buffers (all derived sets and both raw sets included); the session cannot be used afterwards."""
        self.closed = True
        self._raw = self._derived = self._graph = self._res = self.arena = self._cur = self._cur_struct = None
        self._sets = [None, None]
        self._raw_alt, self._transit, self._book = None, [None], None
        self._col_type = self._col_obj = self._opt = None
        self._buffers_made = []
        self._kept, self._stale = {}, set()


class LPEnsembleSession(LPSession):
    """An `LPSession` whose rounds are scored by an ensemble of 1..8 models (`ModelSet.open_lp_ensemble`): the reference trains
    five seeds per problem (model_trainer.py:38-49) and its selector plugin ranks and filters by one quality vector
    (model_evaluator.py:82-154), here the fp32 mean of the members' scores.  Nothing in a resident LP belongs to a model, so the
    session is the plain one -- rows, edits, `state`, guards and `upload_bytes` are inherited unchanged -- and only the round's
    call differs: gcnn_lp_round_ensemble uploads what the plain round uploads, whatever the number of models, runs the edits and
    the round's two state launches once, the M forward passes as one group over that one state, the mean, and the ranking or the
    selection over the mean, and brings the mean and the members' rows home in one download.
    A round's result is by definition what `ModelSet.score_lp_ensemble` / `select_cuts_lp_ensemble` give for the same keys on
    `lpstate.assemble(rows after the call's edits, round)`, bit for bit, field for field: the mean, `.members` (float32 [M, K];
    row m is what `models[m].open_lp(rows).score(round)` returns), `.rankings` or `order`, `n_kept`, `n_selected`, `.cut_index`.
    The session holds no parameters: every round reads each model's current flat parameter buffer.  It takes its device from the
    first model.  An `LPSessionGroup` refuses it: one ensemble of five fills a grouped call's eight forward passes.
    `calls`: gcnn_lp_round_ensemble calls made."""

    def __init__(self, models, rows, deep=True):
        self.models = list(models)
        if not 1 <= len(self.models) <= _lib.GROUP_MAX:
            raise ValueError(f"an ensemble holds 1..{_lib.GROUP_MAX} models, got {len(self.models)}")
        if len({str(m.device) for m in self.models}) != 1:
            raise ValueError("LPEnsembleSession: all models must be on one device")
        self.pin_tab = None
        self.calls = 0
        self._ens = None                  # the layout of the last ensemble call: where its download keeps the members' rows
        super().__init__(self.models[0], rows, deep)

    def _buffers(self, L):
        """The plain session's buffers for `L`; for the layout of an ensemble call (it has `table_bytes`) also the pinned staging
        buffer of the group's launch tables."""
        super()._buffers(L)
        if hasattr(L, "table_bytes"):
            self.pin_tab, _ = self._pin(self.pin_tab, None, L.table_bytes, 1 << 16)

    def _enqueue(self, job, want_order, p_max, p_max_ub, timings, t0):
        """The one C call of a packed job and the wait for its download: gcnn_lp_round_ensemble for scores, ranking or selection,
        whatever edits the job carries; the state alone (`want_order` < 0) needs no model and takes the plain session's call."""
        if want_order < 0:
            return super()._enqueue(job, want_order, p_max, p_max_ub, timings, t0)
        mode = _lib.IBATCH_SELECT if job.forced is not None else (_lib.IBATCH_RANK if want_order else _lib.IBATCH_SCORES)
        member, n = self._member(job, edit=True), len(self.models)
        EL = _lib.LpRoundEnsembleLayout()
        _lib.check(_lib.lib().gcnn_lp_round_ensemble_layout_for(C.byref(member), mode, n, C.byref(EL)), "gcnn_lp_round_ensemble_layout_for")
        if EL.in_bytes != job.L.in_bytes:         # the plain round's upload, which `_pack` has already written
            raise _lib.GcnnError("gcnn_lp_round_ensemble_layout_for: the upload is not the plain round's")
        self._buffers(EL)
        params = (C.c_void_p * n)(*(m._flat.data_ptr() for m in self.models))
        self._enqueue_wait("gcnn_lp_round_ensemble", (C.byref(member), mode, n), (C.c_void_p(self.pin_tab.data_ptr()), float(p_max), float(p_max_ub)),
                           timings, t0, params=params, upload_bytes=int(EL.in_bytes))
        self._ens = EL
        self.calls += 1

    def _results(self, dims, out_off, want_order, select, out=None):
        """(mean, order, n_kept, cut_index, members [M, K]) of a round in the session's download."""
        n, EL = dims["n_cuts"], self._ens
        at, stride = int(EL.member_off), int(EL.member_stride)
        members = np.stack([self.out_np[at + m * stride:at + m * stride + 4 * n].view(np.float32).copy() for m in range(len(self.models))])
        return super()._results(dims, out_off, want_order, select, out) + (members,)

    def score(self, rnd, rank=False, timings=None, append=None, remove=None):
        """`ModelSet.score_lp_ensemble` for the assembled snapshot: a `ScoreArray` of the mean in STATE order with `.cut_index`,
        `.members` and, with `rank`, `.rankings` (on the host up to `HOST_RANK_MAX` cuts, on the device up to 4,096, on the host
        beyond).  `append`, `remove`: as in `LPSession.score`."""
        n = int(np.asarray(rnd.cut_lhs).shape[0])
        on_device = self.model._rank_on_device(rank, n) and n <= 4096
        dims, out_off, _ = self._run(rnd, int(on_device), timings, append=append, remove=remove)
        scores, order, _, cut_index, members = self._results(dims, out_off, on_device, False)
        scores.cut_index, scores.members = cut_index, members
        if rank:
            scores.rankings = order if on_device else stable_ranking(scores)
        return scores

    def select_cuts(self, rnd, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, timings=None, append=None, remove=None):
        """`ModelSet.select_cuts_lp_ensemble` for the assembled snapshot: a `SelectResult` over the mean with `.cut_index` and
        `.members`.  More than 4,096 cuts raise `GcnnError` before anything is enqueued, and the session stays usable.
        `append`, `remove`: as in `LPSession.select_cuts`."""
        ops.check_thresholds(p_max, p_max_ub)
        self.model._check_select_size("LPEnsembleSession.select_cuts", "round", int(np.asarray(rnd.cut_lhs).shape[0]))
        packed = normalize_forced(forced, self.n_cols)
        dims, out_off, _ = self._run(rnd, 1, timings, packed, p_max, p_max_ub, append=append, remove=remove)
        scores, order, n_kept, cut_index, members = self._results(dims, out_off, True, True)
        result = SelectResult(order, n_kept, n_selected(n_kept, max_selected), scores, cut_index)
        result.members = members
        return result

    def close(self):
        super().close()
        self._ens = None


class LPSessionGroup:
    """The rounds of several `LPSession`s in one call (gcnn_lp_rounds): what a scoring server does with the rounds of different
    solver workers that wait at the same time.  One upload of all rounds and appended blocks, every stage of the members' work as
    one launch per distinct kernel, one download; up to 8 sessions per call, more are served in several calls.  The sessions may
    belong to different models on the group's device; a session may appear once per call.  Entry i of a result is what
    `sessions[i].score(...)` / `.select_cuts(...)` gives with the same arguments, bit for bit, and the session is afterwards in
    the state that solo call leaves.  Errors are per member: a round the host rejects stays out of the call, one the device
    flags raises in its own slot (the session stays usable, as after a rejected solo round), and a member the batched call
    declines (a ranking left to the host, a shape the recorder cannot take, and -- unless the group was made with
    `batch_removes=True`, which sends a chunk with such a member through gcnn_lp_rounds_edit -- a member that removes rows) goes
    through its solo call and comes back in place:
    a call the library declines or refuses as a whole is halved until the member it is about stands alone, so the others still
    share their calls, and `solo_rounds` counts every member that was answered by its own call.
    The group owns the call's arena and pinned buffers; they grow as a session's do, and `LPSession.GUARD` applies to the arena."""
    MAX = _lib.LP_ROUNDS_MAX
    CAP = 256
    GUARD = None                      # bytes of guard around the arena; None: `LPSession.GUARD`

    def __init__(self, device, batch_removes=False):
        self.device = torch.device(device)
        self.batch_removes = bool(batch_removes)      # a member with a removal: inside the batched call (gcnn_lp_rounds_edit), or solo
        self.pin_in = self.pin_out = self.pin_tab = self.arena = self._whole = None
        self.in_np = self.out_np = self.tab_np = None
        self.layouts = {}
        self.calls = 0                    # gcnn_lp_rounds / gcnn_lp_rounds_edit calls made
        self.max_sessions_per_call = 0    # the most sessions one of them served
        self.solo_rounds = 0              # members answered by their session's own call: left to it, or declined by the batched call

    def guards_intact(self):
        """True when no guard byte around the group's arena has changed (`LPSession.GUARD` set when it was allocated)."""
        g, w = self._guard(), self._whole
        if not g or w is None:
            return True
        return bool((w[:g] == LPSession.GUARD_BYTE).all()) and bool((w[w.numel() - g:] == LPSession.GUARD_BYTE).all())

    def _guard(self):
        return LPSession.GUARD if self.GUARD is None else self.GUARD

    def _buffers(self, L):
        pin = _Staging._pin
        self.pin_in, self.in_np = pin(self.pin_in, self.in_np, L.in_bytes, 1 << 20)
        self.pin_out, self.out_np = pin(self.pin_out, self.out_np, L.out_bytes, 1 << 16)
        self.pin_tab, self.tab_np = pin(self.pin_tab, self.tab_np, L.table_bytes, 1 << 16)
        if self.arena is None or self.arena.numel() < L.arena_bytes:
            self.arena = self._whole = None
            n, g = max(2 * L.arena_bytes, 1 << 22), self._guard()
            if g:
                self._whole = torch.full((n + 2 * g,), LPSession.GUARD_BYTE, dtype=torch.uint8, device=self.device)
                self.arena = self._whole[g:g + n]
            else:
                self.arena = torch.empty(n, dtype=torch.uint8, device=self.device)

    def _layout(self, members, n, mode, edit=False):
        name = "gcnn_lp_rounds_edit_layout_for" if edit else "gcnn_lp_rounds_layout_for"
        L = _lib.LpRoundsEditLayout() if edit else _lib.LpRoundsLayout()
        rc = getattr(_lib.lib(), name)(n, members, mode, C.byref(L))
        return False if _unsupported(rc, name) else (L, list(L.in_off), list(L.out_off))

    def _call(self, sessions, jobs, mode, p_max, p_max_ub, timings=None):
        """One gcnn_lp_rounds call over checked jobs -- gcnn_lp_rounds_edit where one of them removes rows: per job its download
        block (a view of the group's pinned buffer), or None where the library declines the call as a whole (nothing was
        enqueued); any other refusal raises `GcnnError`, also before anything is enqueued."""
        t0 = time.perf_counter()
        n = len(jobs)
        edit = any(j.rm is not None for j in jobs)
        name = "gcnn_lp_rounds_edit" if edit else "gcnn_lp_rounds"
        kind = _lib.LpRoundsEditMember if edit else _lib.LpRoundsMember
        members = (kind * n)(*(s._member(j, edit) for s, j in zip(sessions, jobs)))
        key = (mode, edit) + tuple(_int_key(j.dims) + (j.present, j.rm is not None) + j.fshape + j.block for j in jobs)
        lay = self.layouts.get(key)
        if lay is None:
            lay = self._layout(members, n, mode, edit)
            if len(self.layouts) >= self.CAP:
                self.layouts.pop(next(iter(self.layouts)))
            self.layouts[key] = lay
        if lay is False:
            return None
        L, in_off, out_off = lay
        self._buffers(L)
        for j, off in zip(jobs, in_off):
            LPSession._pack(j, self.in_np[off:])
        t1 = time.perf_counter()
        P = C.c_void_p
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = getattr(_lib.lib(), name)(n, members, mode, P(self.pin_in.data_ptr()), P(self.pin_out.data_ptr()), P(self.arena.data_ptr()),
                                           self.arena.numel(), P(self.pin_tab.data_ptr()), float(p_max), float(p_max_ub),
                                           P(stream.cuda_stream))
            if rc == -4:
                return None
            _lib.check(rc, name)
            t2 = time.perf_counter()
            stream.synchronize()
        if timings is not None:
            timings.update(pack=t1 - t0, enqueue=t2 - t1, wait=time.perf_counter() - t2, upload_bytes=int(L.in_bytes))
        self.calls += 1
        self.max_sessions_per_call = max(self.max_sessions_per_call, n)
        return [self.out_np[o:] for o in out_off[:n]]

    def _serve(self, sessions, mode, plan, answer, solo, p_max=0.0, p_max_ub=0.0, timings=None):
        """Results per session, each an answer or an exception.  `plan(i)`: the job of session i for the batched call (what it
        raises belongs to that slot), None where the member goes to its solo call; `answer(i, job, out)`: the result read from
        the member's download block; `solo(i)`: the session's own call."""
        n = len(sessions)
        if any(isinstance(s, LPEnsembleSession) for s in sessions):       # (its M forward passes would fill the grouped call alone)
            raise ValueError("LPSessionGroup: an ensemble session's rounds take its own call; grouping them is not supported")
        if len({id(s) for s in sessions}) != n:
            raise ValueError("LPSessionGroup: a session may appear once per call")
        for s in sessions:
            if torch.device(s.model.device) != self.device:
                raise ValueError(f"LPSessionGroup: a session of a model on {s.model.device}, the group is on {self.device}")
        results, jobs, solo_ids = [None] * n, {}, []
        for i in range(n):
            try:
                job = plan(i)
            except Exception as exc:  # noqa: BLE001 -- the error belongs to this member's slot
                results[i] = exc
                continue
            if job is None:
                solo_ids.append(i)
            else:
                jobs[i] = job
        ids = list(jobs)
        todo = [ids[lo:lo + self.MAX] for lo in range(0, len(ids), self.MAX)]
        while todo:
            part = todo.pop(0)
            try:
                outs = self._call([sessions[i] for i in part], [jobs[i] for i in part], mode, p_max, p_max_ub, timings)
            except _lib.GcnnError:          # refused before anything was enqueued: as a declined call, the member's own call says why
                outs = None
            if outs is None:
                if len(part) == 1:
                    solo_ids.append(part[0])
                else:                       # halves: the member the refusal is about ends up alone, the others keep their calls
                    todo[:0] = [part[:len(part) // 2], part[len(part) // 2:]]
                continue
            for i, out in zip(part, outs):
                try:
                    sessions[i]._finish(jobs[i], out)
                    results[i] = answer(i, jobs[i], out)
                except Exception as exc:  # noqa: BLE001
                    results[i] = exc
        self.solo_rounds += len(solo_ids)
        for i in sorted(solo_ids):
            try:
                results[i] = solo(i)
            except Exception as exc:  # noqa: BLE001
                results[i] = exc
        return results

    @staticmethod
    def _finish_many(results, return_exceptions):
        if not return_exceptions:
            for r in results:
                if isinstance(r, Exception):
                    raise r
        return results

    @staticmethod
    def _per_session(what, items, n):
        items = [None] * n if items is None else list(items)
        if len(items) != n:
            raise ValueError(f"{what}: one entry per session expected, got {len(items)} for {n} sessions")
        return items

    def _removes(self, i, removes):
        """Whether member i comes with a removal that its solo call answers: every removal unless the group was made with
        `batch_removes` (gcnn_lp_rounds takes none; gcnn_lp_rounds_edit does)."""
        return not self.batch_removes and removes[i] is not None and np.asarray(removes[i]).size > 0

    def score(self, sessions, rounds, rank=False, appends=None, return_exceptions=False, timings=None, removes=None):
        """`sessions[i].score(rounds[i], rank, append=appends[i], remove=removes[i])` for every i, as a list of `ScoreArray`.
        With `return_exceptions` a member's exception sits in its slot; otherwise the first one is raised after every member has
        been served.  A member with a removal is answered through its solo call and comes back in place (counted in
        `solo_rounds`) while the others keep their batched call; with `batch_removes` it is a member of the batched call."""
        sessions, rounds = list(sessions), list(rounds)
        appends = self._per_session("appends", appends, len(sessions))
        removes = self._per_session("removes", removes, len(sessions))
        self._per_session("rounds", rounds, len(sessions))

        def on_device(i):
            n = int(np.asarray(rounds[i].cut_lhs).shape[0])
            return sessions[i].model._rank_on_device(rank, n) and n <= 4096

        def plan(i):
            if (rank and not on_device(i)) or self._removes(i, removes):
                return None                 # the host ranks this one, or it removes rows: its solo call
            return sessions[i]._plan(rounds[i], None, appends[i], removes[i] if self.batch_removes else None)

        def answer(i, job, out):
            scores, order, _, cut_index = sessions[i]._results(job.dims, job.out_off, bool(rank), False, out)
            scores.cut_index = cut_index
            if rank:
                scores.rankings = order
            return scores

        results = self._serve(sessions, _lib.IBATCH_RANK if rank else _lib.IBATCH_SCORES, plan, answer,
                              lambda i: sessions[i].score(rounds[i], rank, append=appends[i], remove=removes[i]), timings=timings)
        return self._finish_many(results, return_exceptions)

    def select_cuts(self, sessions, rounds, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, appends=None,
                    return_exceptions=False, timings=None, removes=None):
        """`sessions[i].select_cuts(rounds[i], forced[i], p_max=..., p_max_ub=..., max_selected=..., append=appends[i],
        remove=removes[i])` for every i, as a list of `SelectResult`; errors and removals as in `score`."""
        ops.check_thresholds(p_max, p_max_ub)
        sessions, rounds = list(sessions), list(rounds)
        n = len(sessions)
        appends, forced = self._per_session("appends", appends, n), self._per_session("forced", forced, n)
        removes = self._per_session("removes", removes, n)
        self._per_session("rounds", rounds, n)

        def plan(i):
            s = sessions[i]
            s.model._check_select_size("LPSession.select_cuts", "round", int(np.asarray(rounds[i].cut_lhs).shape[0]))
            if self._removes(i, removes):
                return None
            return s._plan(rounds[i], normalize_forced(forced[i], s.n_cols), appends[i], removes[i] if self.batch_removes else None)

        def answer(i, job, out):
            scores, order, n_kept, cut_index = sessions[i]._results(job.dims, job.out_off, True, True, out)
            return SelectResult(order, n_kept, n_selected(n_kept, max_selected), scores, cut_index)

        def solo(i):
            return sessions[i].select_cuts(rounds[i], forced[i], p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected, append=appends[i],
                                           remove=removes[i])

        results = self._serve(sessions, _lib.IBATCH_SELECT, plan, answer, solo, p_max, p_max_ub, timings)
        return self._finish_many(results, return_exceptions)


def _int_key(dims):
    """The sizes of a snapshot's dims (what a layout depends on; the three scalars are not part of it)."""
    return tuple(v for v in dims.values() if isinstance(v, int))
