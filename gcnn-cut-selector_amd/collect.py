"""The data collector's expert rounds on the device: the fourth cut-selector plugin of the reference,
data_collector.SamplingAgent.cutselselect (data_collector.py:86-195), in a round that queries the expert.

SCIP's dives give a float64 quality per cut (data_collector.py:104-131).  The plugin then needs the sample's state,
`get_state(self.model, cuts)` (data_collector.py:135), and the same ranking and parallelism filter as every other arm
(data_collector.py:150-195) over that quality.  `Collector.collect_lp` answers both with one C call (gcnn_lp_collect: one upload, at
most six launches, one download) from a `lpstate.LPSnapshot`, and hands back the labels aligned with the state it built:
`get_state` lists the cuts that take their lhs side first (utils.py:180-185) while the reference pickles the quality in input cut
order (data_collector.py:136).  No model is involved.  There is no CPU fallback."""

from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch

from . import _lib, lpstate, ops
from .infer import _LPSession, _Staging, n_selected, normalize_forced
from .lpstate import CollectResult, check_quality
from .model import GCNN

__all__ = ["Collector", "CollectResult"]


class _CollectSession(_Staging):
    """Host side of gcnn_lp_collect: check -> layout -> pack -> one call -> the download's fourteen pieces."""

    def __init__(self, owner):
        super().__init__(owner)      # (`owner.device` is all the staging reads)
        self.calls = 0               # C calls made (tools and tests read it)
        self.upload_bytes = 0        # bytes of the last call's upload
        self.download_bytes = 0      # bytes of the last call's download

    @staticmethod
    def _layout(dims, n_forced, n_entries):
        d, L = _lib.LpDims(**dims), _lib.LpCollectLayout()
        _lib.check(_lib.lib().gcnn_lp_collect_layout_for(C.byref(d), n_forced, n_entries, C.byref(L)), "gcnn_lp_collect_layout_for")
        return L, list(L.snap_off), list(L.forced_off), list(L.out_off)

    def run(self, arrays, dims, quality, forced, p_max, p_max_ub, timings=None, t0=0.0, arena=None):
        """arrays, dims: as `lpstate.check_snapshot` returns them; quality: checked float64 [K]; forced: packed (ptr, col, val).
        -> (state 10-tuple, cut_index, hybrid quality, features, order, n_kept); ValueError for what the device flags."""
        fshape = (forced[0].size - 1, forced[1].size)
        key = tuple(v for v in dims.values() if isinstance(v, int)) + fshape
        L, snap_off, forced_off, out_off = self.cached(key, self._layout, dims, *fshape)
        d = _lib.LpDims(**dims)         # (the scalars are not part of the layout's key: the struct is this call's)
        self._buffers(L)
        lpstate.pack_snapshot(self.in_np, snap_off, arrays)
        if quality.size:
            self.in_np[L.quality_off:L.quality_off + quality.nbytes] = quality.view(np.uint8)
        self._put_forced(forced_off, forced)
        self._enqueue_wait("gcnn_lp_collect", (C.byref(d), *fshape), (float(p_max), float(p_max_ub)), timings, t0, params=None,
                           arena=arena, upload_bytes=int(L.in_bytes), download_bytes=int(L.out_bytes))
        self.calls += 1
        self.upload_bytes, self.download_bytes = int(L.in_bytes), int(L.out_bytes)
        self.last = L
        out = self.out_np
        lpstate.raise_for_flags(out[out_off[8]:out_off[8] + 16].view(np.int32))
        lpstate.raise_for_flags(out[out_off[13]:out_off[13] + 16].view(np.int32))
        c, v, k, e1, e2 = lpstate.state_key(dims)
        f32, i32, f64 = np.float32, np.int32, np.float64
        shapes = (((c, 4), f32), ((2, e1), i32), ((e1, 1), f32), ((v, 14), f32), ((k, 6), f32), ((2, e2), i32), ((e2, 1), f32),
                  ((k,), i32), None, ((k,), f64), ((k, 3), f64), ((k,), i32))

        def piece(i):
            shape, dt = shapes[i]
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            return out[out_off[i]:out_off[i] + n].view(dt).reshape(shape).copy()

        state = tuple(piece(i) for i in range(7)) + (c, v, k)
        n_kept = int(out[out_off[12]:out_off[12] + 4].view(np.int32)[0])
        return state, piece(7), piece(9), piece(10), piece(11), n_kept

    def last_table(self):
        """The table the last call wrote into the upload, as bytes (tests compare its positions with the layout's)."""
        L = self.last
        return self.in_np[L.table_off:L.table_off + L.table_bytes].copy()


class Collector:
    """`Collector(device=None)`: the expert rounds of the data collector on `device` (default: the current CUDA device).  It needs
    no model.  `collect_lp` serves a round whose qualities came from SCIP's dives; `state_from_lp` builds the state alone."""

    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._session = None
        self._lp_session = None

    def _sess(self):
        if self._session is None:
            self._session = _CollectSession(self)
        return self._session

    def state_from_lp(self, snapshot):
        """`GCNN.state_from_lp` for a process that has no model (gcnn_lp_state): (the 10-tuple as host arrays, cut_index)."""
        if self._lp_session is None:
            self._lp_session = _LPSession(self)      # (`self.device` is all gcnn_lp_state's host side reads)
        state, cut_index = self._lp_session.build_state(snapshot)
        return tuple(t.cpu().numpy() for t in state[:7]) + state[7:], cut_index.cpu().numpy()

    def collect_lp(self, snapshot, quality, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, timings=None):
        """One expert round.  `snapshot`: a `lpstate.LPSnapshot`; `quality`: float64 [K] in INPUT cut order, one finite value per
        cut; `forced` as `GCNN.select_cuts` takes it.  Returns a `CollectResult`: `state` and `cut_index` as `state_from_lp` gives
        them, `improvements` = quality[cut_index], and `order`, `n_kept`, `n_selected` -- the plugin's ranking
        (`sorted(range(K), key=lambda x: quality[x], reverse=True)`: ties in input order), low-quality flags by position against
        0.9 * quality[order[0]] in float64, forced phase, greedy walk -- in INPUT cut indices; `hybrid_quality` and `features` as
        `HybridSelector` reports them.  ValueError for a quality of the wrong length or dtype kind or with a value that is not
        finite, for thresholds that are not finite, and (after the download) for what the device flags in the snapshot;
        `GcnnError` for more than 4,096 cuts.  `timings` (optional dict): the host-side phases in seconds (pack, enqueue, wait) and
        the call's upload and download bytes."""
        t0 = time.perf_counter()
        ops.check_thresholds(p_max, p_max_ub)
        arrays, dims = lpstate.check_snapshot(snapshot, deep=False)
        q = check_quality(quality, dims["n_cuts"])
        GCNN._check_select_size("collect_lp", "snapshot", dims["n_cuts"])
        packed = normalize_forced(forced, dims["n_cols"])
        state, cut_index, hybrid_quality, features, order, n_kept = self._sess().run(arrays, dims, q, packed, p_max, p_max_ub, timings, t0)
        return CollectResult(state, cut_index, q[cut_index], order, n_kept, n_selected(n_kept, max_selected), hybrid_quality, features)
