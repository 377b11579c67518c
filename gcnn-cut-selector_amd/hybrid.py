"""SCIP's hybrid cut selection from the cut rows alone, on the device: the `function=None` arm of the reference's selector
(model_evaluator.py:104-154), the baseline arm of model_benchmarker.py and every non-expert round of data_collector.py:145-195.

    quality = efficacy + 0.1 * int_support + 0.1 * objective parallelism          (float64, input cut order)

followed by the same greedy parallelism filter as `GCNN.select_cuts`.  No model is involved and no LP rows, duals or bases are
read: a `lpstate.CutSnapshot` (or an `LPSnapshot`) goes up, one C call (gcnn_hybrid_select: at most four launches for up to 64
snapshots) answers.  There is no CPU fallback."""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, lpstate, ops
from .infer import SelectResult, _Staging, forced_counts, forced_shapes, n_selected, prefix
from .model import GCNN, _packed_forced, _snapshot_vars


class _HybridSession(_Staging):
    """Host side of gcnn_hybrid_select: one C call for up to 64 cut snapshots.  `run` answers per snapshot
    ("ok", quality, features, order | None, n_kept | None) or ("error", ValueError) for what the device flags."""
    MAX = _lib.IBATCH_MAX
    CAP = 64

    def __init__(self, owner):
        super().__init__(owner)      # (`owner.device` is all the staging reads)
        self.calls = 0               # C calls made (tools and tests read it)
        self.upload_bytes = 0        # bytes of the last call's upload

    @staticmethod
    def _dims_array(dims):
        return (_lib.HybridDims * len(dims))(*(_lib.HybridDims(**d) for d in dims))

    def _layout(self, dims, fshapes, mode):
        n = len(dims)
        nf, nfe = forced_counts(fshapes)
        L = _lib.HybridLayout()
        _lib.check(_lib.lib().gcnn_hybrid_layout_for(n, self._dims_array(dims), nf, nfe, mode, C.byref(L)), "gcnn_hybrid_layout_for")
        k_off = prefix(d["n_cuts"] for d in dims)
        f_off, fe_off = (prefix(f[j] for f in fshapes) for j in (0, 1))
        return nf, nfe, L, [list(L.snap_off[s]) for s in range(n)], k_off, f_off, fe_off, list(L.forced_off), list(L.out_off)

    def run(self, checked, forced, mode, p_max=0.0, p_max_ub=0.0, arena=None):
        """checked: [(arrays, dims)] as `lpstate.check_cut_snapshot` returns them; forced: None or [(ptr, col, val)] per snapshot.
        `arena` (tests): a device uint8 tensor to run in instead of the session's own."""
        n = len(checked)
        dims = [d for _, d in checked]
        fshapes = forced_shapes(forced)
        key = (mode, tuple((d["n_cols"], d["n_cuts"], d["cut_nnz"]) for d in dims), fshapes)
        nf, nfe, L, snap_at, k_off, f_off, fe_off, forced_off, out_off = self.cached(key, self._layout, dims, fshapes, mode)
        d = self._dims_array(dims)          # (infinity is not part of the layout's key: the array is this call's)
        self._buffers(L)
        buf = self.in_np
        _lib.check(_lib.lib().gcnn_hybrid_fill_table(n, d, nf, nfe, mode, self.pin_in.data_ptr()), "gcnn_hybrid_fill_table")
        for (arrays, _), at in zip(checked, snap_at):
            for off, a in zip(at, arrays):
                if a.size:
                    buf[off:off + a.nbytes] = a.view(np.uint8)
        self._put_forced_stacked(forced_off, f_off, fe_off, forced)
        self._enqueue_wait("gcnn_hybrid_select", (n, d, nf, nfe, mode), (float(p_max), float(p_max_ub)), params=None, arena=arena)
        self.calls += 1
        self.upload_bytes = int(L.in_bytes)
        self.last = L
        out, res = self.out_np, []
        for s in range(n):
            k0, cuts = k_off[s], k_off[s + 1] - k_off[s]
            try:
                lpstate.raise_for_flags(out[out_off[4] + 16 * s:out_off[4] + 16 * s + 16].view(np.int32))
            except ValueError as exc:
                res.append(("error", exc))
                continue
            quality = out[out_off[0] + 8 * k0:out_off[0] + 8 * (k0 + cuts)].view(np.float64).copy()
            features = out[out_off[1] + 24 * k0:out_off[1] + 24 * (k0 + cuts)].view(np.float64).reshape(cuts, 3).copy()
            order = n_kept = None
            if mode != _lib.HYBRID_QUALITY:
                order = out[out_off[2] + 4 * k0:out_off[2] + 4 * (k0 + cuts)].view(np.int32).copy()
                n_kept = int(out[out_off[3] + 4 * s:out_off[3] + 4 * s + 4].view(np.int32)[0])
            res.append(("ok", quality, features, order, n_kept))
        return res

    def last_rows(self):
        """The stacked fp32 rows the last call left in the arena (tests compare them with the LP path's cut edges): (ptr, col, val)."""
        L = self.last
        K, E = L.total_cuts, L.total_nnz
        off = list(L.rows_off)
        view = lambda o, n, dt: self.arena[o:o + 4 * n].view(dt).cpu().numpy()  # noqa: E731
        return view(off[0], K + 1, torch.int32), view(off[1], E, torch.int32), view(off[2], E, torch.float32)


class HybridSelector:
    """`HybridSelector(device=None)`: the hybrid arm of the cut selector on `device` (default: the current CUDA device)."""

    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._session = None

    def _sess(self):
        if self._session is None:
            self._session = _HybridSession(self)
        return self._session

    def _many(self, snapshots, mode, packed=None, p_max=0.0, p_max_ub=0.0):
        """Per snapshot ("ok", quality, features, order, n_kept) or an exception; more than 64 are served in several calls."""
        n = len(snapshots)
        results, checked, ids = [None] * n, {}, []
        for i, snap in enumerate(snapshots):
            try:
                if packed is not None and isinstance(packed[i], Exception):
                    raise packed[i]
                arrays, dims = lpstate.check_cut_snapshot(snap, deep=False)
                if mode != _lib.HYBRID_QUALITY:
                    GCNN._check_select_size("HybridSelector.select_cuts", "snapshot", dims["n_cuts"])
                if dims["n_cuts"] == 0:
                    results[i] = ("ok", np.zeros(0, np.float64), np.zeros((0, 3), np.float64), np.zeros(0, np.int32), 0)
                    continue
                checked[i] = (arrays, dims)
                ids.append(i)
            except Exception as exc:  # noqa: BLE001 -- the error belongs to this snapshot's slot
                results[i] = exc
        session = self._sess()
        for j in range(0, len(ids), session.MAX):
            part = ids[j:j + session.MAX]
            got = session.run([checked[i] for i in part], None if packed is None else [packed[i] for i in part], mode, p_max, p_max_ub)
            for i, r in zip(part, got):
                results[i] = r[1] if r[0] == "error" else r
        return results

    def quality(self, snapshot):
        """The float64 hybrid quality of every cut, in input order.  `.features` [K, 3]: efficacy, integer support, objective
        parallelism (float64)."""
        (r,) = self._many([snapshot], _lib.HYBRID_QUALITY)
        if isinstance(r, Exception):
            raise r
        q = r[1].view(_Quality)
        q.features = r[2]
        return q

    def select_cuts(self, snapshot, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        """`GCNN.select_cuts_lp` with the hybrid quality in place of the model's scores.  The `SelectResult`'s `scores` is the
        float64 quality and `order` is in INPUT cut order; `cut_index` is the identity, so code written against `select_cuts_lp`
        runs as it is; `.features` [K, 3] float64."""
        return self.select_cuts_many([snapshot], [forced], p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected)[0]

    def select_cuts_many(self, snapshots, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        """`select_cuts` for many snapshots at once (up to 64 per C call, more in several calls).  `forced`: None, or one entry per
        snapshot in the forms `GCNN.select_cuts` accepts.  Errors per snapshot as in `GCNN.select_cuts_lp_many`: a snapshot of more
        than 4,096 cuts holds the `GcnnError` of the size check, one the device flags its `ValueError`."""
        ops.check_thresholds(p_max, p_max_ub)
        snapshots = list(snapshots)
        forced, packed = _packed_forced(snapshots, forced, _snapshot_vars, "snapshot")
        results = self._many(snapshots, _lib.HYBRID_SELECT, packed, p_max, p_max_ub)
        for i, r in enumerate(results):
            if isinstance(r, tuple):
                _, quality, features, order, n_kept = r
                res = SelectResult(order, n_kept, n_selected(n_kept, max_selected), quality, np.arange(quality.size, dtype=np.int32))
                res.features = features
                results[i] = res
        return GCNN._finish_many(results, return_exceptions)


class _Quality(np.ndarray):
    """The hybrid quality as an ndarray that also carries `.features` and answers `.numpy()`."""
    features = None

    def numpy(self):
        return np.asarray(self)
