"""`GCNN` with the call surface of the reference's model (/root/reference/model.py), running on hand-written HIP.

Surface mirrored (file:line in the reference):
  GCNN()                                   model.py:164-226   no-arg constructor, attrs emb_size/cons_feats/...
  model(inputs10, training) / model.call   model.py:257-300   -> flat fp32 scores, `.numpy()` works (model_evaluator.py:103)
  save_state / restore_state               model.py:47-67     62 consecutive pickle.dump(np.ndarray) records
  pretrain_init / pretrain / pretrain_next model.py:69-133    PreNorm fitting hooks (model_trainer.py:207-230)
  variables / trainable_variables          model.py:215, model_trainer.py:272-273
  input_signature                          model.py:218-226   kept as a description of dtypes/shapes
All arithmetic happens in libgcnn_hip.so (include/gcnn_hip.h); torch only stores tensors and hosts the autograd node.
"""

from __future__ import annotations

import ctypes as C
import os
import pickle

import numpy as np
import torch

from . import _lib, _safe_pickle, ops
from .graph import BipartiteGraph, _ptr, _stream
from .infer import (BAD_INDEX, LPEnsembleSession, LPSession, LPSessionGroup, ScoreArray, SelectResult, _BatchSession, _EnsembleBatchSession, _EnsembleSession, _InferenceSession, _LPBatchSession, _LPEnsembleBatchSession, _LPEnsembleSession, _LPModelsSession, _LPSession,
                    _ModelsSession,
                    _UseGeneralPath,
                    check_feature_shapes, check_state, edges_without_nodes, is_host_state, n_selected, normalize_forced, stable_ranking)

EMB = 64


def _emb_spec(prefix, f):
    return [(f"{prefix}_prenorm/shift", (f,), False), (f"{prefix}_prenorm/scale", (f,), False),
            (f"{prefix}_emb_1/kernel", (f, EMB), True), (f"{prefix}_emb_1/bias", (EMB,), True),
            (f"{prefix}_emb_2/kernel", (EMB, EMB), True), (f"{prefix}_emb_2/bias", (EMB,), True)]


def _conv_spec(name):
    return [(f"{name}_feat_left/kernel", (EMB, EMB), True), (f"{name}_feat_left/bias", (EMB,), True),
            (f"{name}_feat_edge/kernel", (1, EMB), True), (f"{name}_feat_right/kernel", (EMB, EMB), True),
            (f"{name}_final_prenorm/scale", (1,), False),
            (f"{name}_feat_final/kernel", (EMB, EMB), True), (f"{name}_feat_final/bias", (EMB,), True),
            (f"{name}_post_prenorm/scale", (1,), False),
            (f"{name}_out_1/kernel", (2 * EMB, EMB), True), (f"{name}_out_1/bias", (EMB,), True),
            (f"{name}_out_2/kernel", (EMB, EMB), True), (f"{name}_out_2/bias", (EMB,), True)]


# Checkpoint order = Keras `Model.variables` of the reference (model.py:53-56, 215): tracked sub-layers in attribute
# order, each Dense [kernel, bias], each PreNormLayer [shift, scale].  Inferred from Keras 2.7 semantics; not verifiable
# here without TensorFlow (shapes make a wrong order fail loudly in restore_state).
VARIABLE_SPEC = (_emb_spec("cons", 4)
                 + [("cons_edge_prenorm/shift", (1,), False), ("cons_edge_prenorm/scale", (1,), False)]
                 + _emb_spec("var", 14) + _emb_spec("cut", 6)
                 + [("cut_edge_prenorm/shift", (1,), False), ("cut_edge_prenorm/scale", (1,), False)]
                 + _conv_spec("cons_conv") + _conv_spec("var_conv") + _conv_spec("cut_conv")
                 + [("out_1/kernel", (EMB, EMB), True), ("out_1/bias", (EMB,), True),
                    ("out_2/kernel", (EMB, 1), True), ("out_2/bias", (1,), True)])


# The 11 PreNorm layers in CALL order (model.py:287-296, 563-570): (shift variable | None, scale variable, units).
PRENORM_LAYERS = [("cons_prenorm/shift", "cons_prenorm/scale", 4), ("cons_edge_prenorm/shift", "cons_edge_prenorm/scale", 1),
                  ("var_prenorm/shift", "var_prenorm/scale", 14), ("cut_prenorm/shift", "cut_prenorm/scale", 6),
                  ("cut_edge_prenorm/shift", "cut_edge_prenorm/scale", 1),
                  (None, "cons_conv_final_prenorm/scale", 1), (None, "cons_conv_post_prenorm/scale", 1),
                  (None, "var_conv_final_prenorm/scale", 1), (None, "var_conv_post_prenorm/scale", 1),
                  (None, "cut_conv_final_prenorm/scale", 1), (None, "cut_conv_post_prenorm/scale", 1)]


class ScoreTensor(torch.Tensor):
    """Device tensor whose `.numpy()` copies to the host, so the reference's `model(...).numpy()` call sites work."""

    def numpy(self, *args, **kwargs):
        return torch.Tensor.numpy(self.detach().cpu().as_subclass(torch.Tensor), *args, **kwargs)


def prenorm_count(dims, layer):
    """The elements PreNorm layer `layer` (call order) absorbs from a batch of these dims."""
    if layer <= 4:
        return [dims.n_cons, dims.n_cons_edges, dims.n_vars, dims.n_cuts, dims.n_cut_edges][layer]
    conv, post = (layer - 5) // 2, (layer - 5) % 2
    n_recv = [dims.n_cons, dims.n_vars, dims.n_cuts][conv]
    n_edge = [dims.n_cons_edges, dims.n_cons_edges, dims.n_cut_edges][conv]
    return (n_recv if post else n_edge) * EMB


class Batch:
    """A stacked mini-batch resident on the GPU: features + both CSR orders of both edge sets (GCNN.prepare)."""

    def __init__(self, cons_feats, var_feats, cut_feats, cons_graph, cut_graph):
        self.cons_feats, self.var_feats, self.cut_feats = cons_feats, var_feats, cut_feats
        self.cons_graph, self.cut_graph = cons_graph, cut_graph
        self.dims = _lib.Dims(cons_feats.shape[0], var_feats.shape[0], cut_feats.shape[0], cons_graph.n_edges,
                              cut_graph.n_edges)
        self.n_edges = cons_graph.n_edges + cut_graph.n_edges
        self.device = cons_feats.device


def _as_device(x, dtype, device):
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype != dtype:
        if dtype == torch.int32 and t.dtype in (torch.int64, torch.int16, torch.uint8, torch.int8):
            t = t.to(torch.int32)
        elif dtype == torch.float32 and t.dtype in (torch.float64, torch.float16, torch.bfloat16, torch.bool,
                                                    torch.int64, torch.int32):
            t = t.to(torch.float32)
        else:
            raise ValueError(f"expected {dtype}, got {t.dtype}")
    return t.to(device, non_blocking=True).contiguous()


class _GCNNFunction(torch.autograd.Function):
    """Autograd node around gcnn_forward / gcnn_backward (the role tf.GradientTape plays in model_trainer.py:269-272)."""

    @staticmethod
    def forward(ctx, flat, model, batch):
        ws = model._take_workspace(batch)
        scores = model._forward_into(flat, batch, ws)
        ctx.model, ctx.batch, ctx.ws = model, batch, ws
        ctx.save_for_backward(flat)
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        model, batch, ws = ctx.model, ctx.batch, ctx.ws
        if ws is None:
            raise RuntimeError("GCNN backward called twice on the same forward pass")
        (flat,) = ctx.saved_tensors
        grads = torch.zeros_like(flat)  # non-trainable / padding slots are never written by gcnn_backward
        model._backward_into(flat, batch, ws, d_scores.contiguous().to(torch.float32), grads)
        model._give_workspace(ws)
        ctx.ws = None
        return grads, None, None


def _serve_many(n, admit, split, run, solo):
    """The driver of every `*_many` entry point (`GCNN._many`, `ModelSet._many`): results per state, each ("ok", ...) or an exception.
    `admit(i)`: the checked entry of state i for the batched call, None where it goes to the solo entry point; what it raises
    belongs to that state's slot.  `split(ids)`: the admitted states as the calls that serve them.  `run(ids, checked)`: one call's
    answers per state -- ("ok", ...), ("error", exc), ("bad_index",), anything else = declined -- or None where the library
    declines the union as a whole (too large: halves, and a single state goes solo).  `solo(i)`: the single-state entry point."""
    results, checked, batch_ids, solo_ids = [None] * n, {}, [], []
    for i in range(n):
        try:
            entry = admit(i)
        except Exception as exc:  # noqa: BLE001 -- the error belongs to this state's slot
            results[i] = exc
            continue
        if entry is None:
            solo_ids.append(i)
        else:
            checked[i] = entry
            batch_ids.append(i)
    todo = split(batch_ids)
    while todo:
        ids = todo.pop(0)
        got = run(ids, checked)
        if got is None:
            if len(ids) == 1:
                solo_ids.append(ids[0])
            else:
                todo[:0] = [ids[:len(ids) // 2], ids[len(ids) // 2:]]
            continue
        for i, r in zip(ids, got):
            if r[0] == "ok":
                results[i] = r
            elif r[0] == "error":
                results[i] = r[1]
            elif r[0] == "bad_index":
                results[i] = ValueError(BAD_INDEX)
            else:
                solo_ids.append(i)
    for i in solo_ids:
        try:
            results[i] = solo(i)
        except Exception as exc:  # noqa: BLE001
            results[i] = exc
    return results


def _state_vars(state):
    if isinstance(state, Batch):
        return state.dims.n_vars
    v = state[3]                  # (a device tensor has a shape too, and NumPy cannot read it)
    return int(v.shape[0]) if hasattr(v, "shape") else int(np.asarray(v).shape[0])


def _snapshot_vars(snapshot):
    return int(np.asarray(snapshot.col_type).shape[0])


def _packed_forced(items, forced, n_vars_of, noun):
    """The forced rows of a `*_many` selection over `items` (`noun`s): (`forced` as a list with one entry per item, those entries
    packed by `normalize_forced`).  An entry that cannot be packed holds its exception: it belongs to that item's slot."""
    forced = [None] * len(items) if forced is None else list(forced)
    if len(forced) != len(items):
        raise ValueError(f"forced: one entry per {noun} expected, got {len(forced)} for {len(items)} {noun}s")
    packed = []
    for item, f in zip(items, forced):
        try:
            packed.append(normalize_forced(f, n_vars_of(item)))
        except Exception as exc:  # noqa: BLE001
            packed.append(exc)
    return forced, packed


def _as_scores(results, rank, cut_index=False):
    """`_serve_many`'s ("ok", scores, order, n_kept[, cut_index]) answers as `ScoreArray`s, in place; exceptions stay."""
    for i, r in enumerate(results):
        if isinstance(r, tuple):
            scores = r[1]
            if cut_index:
                scores.cut_index = r[4]
            if rank:
                scores.rankings = r[2]
            results[i] = scores
    return results


def _as_selections(results, max_selected, cut_index=False):
    """`_serve_many`'s ("ok", scores, order, n_kept[, cut_index]) answers as `SelectResult`s, in place; exceptions stay."""
    for i, r in enumerate(results):
        if isinstance(r, tuple):
            results[i] = SelectResult(r[2], r[3], n_selected(r[3], max_selected), r[1], r[4] if cut_index else None)
    return results


class GCNN:
    """Bipartite GCNN cut scorer (the reference's `GCNN(BaseModel)`, model.py:136-300) on MI355X."""

    def __init__(self, device=None, seed=None):
        self.emb_size, self.cons_feats, self.edge_feats, self.var_feats, self.cut_feats = EMB, 4, 1, 14, 6
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.GcnnError("GCNN needs an MI355X: torch.cuda.is_available() is False and there is no CPU path")
            device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", torch.cuda.current_device())))
        self.device = torch.device(device)
        layout, total = _lib.param_layout()
        if len(layout) != len(VARIABLE_SPEC):
            raise _lib.GcnnError("library / binding disagree on the number of model variables")
        for (off, rows, cols, tr), (name, shape, trainable) in zip(layout, VARIABLE_SPEC):
            if rows * cols != int(np.prod(shape)) or tr != trainable:
                raise _lib.GcnnError(f"library / binding disagree on variable {name}")
        self._layout, self._total = layout, total
        self._flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._flat.requires_grad_(True)
        mask = torch.zeros(total, dtype=torch.bool)
        for (off, rows, cols, tr) in layout:
            if tr:
                mask[off:off + rows * cols] = True
        self._trainable_mask = mask.to(self.device)
        self.variables_topological_order = [name for name, _, _ in VARIABLE_SPEC]
        self.input_signature = [(("float32", (None, 4)), ("int32", (2, None)), ("float32", (None, 1)),
                                 ("float32", (None, 14)), ("float32", (None, 6)), ("int32", (2, None)),
                                 ("float32", (None, 1)), ("int32", ()), ("int32", ()), ("int32", ())), ("bool", ())]
        self._ws_pool = []
        self._session = None      # single-state inference (gcnn_infer): pinned staging + device arena, created on first use
        self._batch_session = None   # many host states per call (gcnn_infer_batch), created on first use
        self._lp_session = None   # calls that start from a raw LP snapshot (gcnn_lp_*), created on first use
        self._lp_batch_session = None   # many LP snapshots per call (gcnn_lp_batch), created on first use
        self._pin = None          # pinned host staging buffer for prepare()
        self._pin_event = None
        self._prenorm_state = None
        self._init_weights(np.random.default_rng(seed))

    # ---- variables ---------------------------------------------------------------------------------------------
    def _init_weights(self, rng):
        """Keras defaults of the reference (model.py:175, 334, 342): orthogonal kernels, zero biases, shift 0, scale 1."""
        host = np.zeros(self._total, np.float32)
        for (off, rows, cols, _), (name, shape, _) in zip(self._layout, VARIABLE_SPEC):
            n = rows * cols
            if name.endswith("/kernel"):
                r, c = shape
                q, tri = np.linalg.qr(rng.standard_normal((max(r, c), min(r, c))))
                q = q * np.sign(np.diag(tri))
                host[off:off + n] = (q if r >= c else q.T).astype(np.float32).reshape(-1)
            elif name.endswith("/scale"):
                host[off:off + n] = 1.0
        with torch.no_grad():
            self._flat.copy_(torch.from_numpy(host))

    @property
    def flat_parameters(self) -> torch.Tensor:
        """The single flat fp32 buffer holding all 62 variables (leaf tensor; `.grad` is filled by backward)."""
        return self._flat

    @property
    def variables(self):
        out = []
        for (off, rows, cols, _), (_, shape, _) in zip(self._layout, VARIABLE_SPEC):
            out.append(self._flat.detach()[off:off + rows * cols].view(shape))
        return out

    @property
    def trainable_variables(self):
        return [v for v, (_, _, tr) in zip(self.variables, VARIABLE_SPEC) if tr]

    def gradients(self, flat_grad=None):
        """The 46 gradient views matching `trainable_variables` (model_trainer.py:272), from a flat gradient buffer."""
        g = self._flat.grad if flat_grad is None else flat_grad
        if g is None:
            raise RuntimeError("no gradient has been computed yet")
        return [g[off:off + rows * cols].view(shape) for (off, rows, cols, tr), (_, shape, _) in
                zip(self._layout, VARIABLE_SPEC) if tr]

    def get_variable(self, name):
        return self.variables[self.variables_topological_order.index(name)]

    def set_weights(self, arrays):
        """Assign the 62 variables from arrays in checkpoint order (dict name->array also accepted)."""
        if isinstance(arrays, dict):
            arrays = [arrays[n] for n in self.variables_topological_order]
        if len(arrays) != len(VARIABLE_SPEC):
            raise ValueError(f"expected {len(VARIABLE_SPEC)} arrays, got {len(arrays)}")
        host = self._flat.detach().cpu().numpy().copy()
        for a, (off, rows, cols, _), (name, shape, _) in zip(arrays, self._layout, VARIABLE_SPEC):
            a = np.asarray(a, dtype=np.float32)
            if a.shape != tuple(shape):
                raise ValueError(f"variable {name}: expected shape {tuple(shape)}, got {a.shape}")
            host[off:off + rows * cols] = a.reshape(-1)
        with torch.no_grad():
            self._flat.copy_(torch.from_numpy(host))

    def get_weights(self):
        host = self._flat.detach().cpu().numpy()
        return [host[off:off + rows * cols].reshape(shape).copy() for (off, rows, cols, _), (_, shape, _) in
                zip(self._layout, VARIABLE_SPEC)]

    def save_state(self, path: str):
        """model.py:47-56: one pickle.dump(np.ndarray) per variable, no header."""
        with open(path, "wb") as file:
            for a in self.get_weights():
                pickle.dump(a, file)

    def restore_state(self, path: str):
        """model.py:58-67.  The records are read with an unpickler that admits NumPy arrays only (`_safe_pickle`)."""
        arrays = []
        with open(path, "rb") as file:
            for _ in VARIABLE_SPEC:
                arrays.append(_safe_pickle.load(file))
        self.set_weights(arrays)

    # ---- inputs ------------------------------------------------------------------------------------------------
    def _stage_host_arrays(self, arrays):
        """ONE host->device copy for all seven input arrays: pack them (16-byte aligned) into a pinned staging buffer,
        copy once, and hand out typed views of the device buffer (which the views keep alive)."""
        specs, total = [], 0
        for a, dt in arrays:
            a = np.ascontiguousarray(np.asarray(a), dtype=dt)
            specs.append((a, total))
            total += (a.nbytes + 15) & ~15
        total = max(total, 16)
        if self._pin is None or self._pin.numel() < total:
            self._pin = torch.empty(max(total, 1 << 16), dtype=torch.uint8).pin_memory()
            self._pin_event = None
        if self._pin_event is not None:
            self._pin_event.synchronize()      # the previous batch's copy must have left the staging buffer
        host = self._pin.numpy()
        for a, off in specs:
            host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        dev_buf = torch.empty(total, dtype=torch.uint8, device=self.device)
        dev_buf.copy_(self._pin[:total], non_blocking=True)
        self._pin_event = torch.cuda.Event()
        self._pin_event.record(torch.cuda.current_stream(self.device))
        out = []
        for a, off in specs:
            tdt = torch.float32 if a.dtype == np.float32 else torch.int32
            out.append(dev_buf[off:off + a.nbytes].view(tdt).view(a.shape))
        return out

    def prepare(self, inputs, validate=True) -> Batch:
        """10-tuple of NumPy arrays / torch tensors (model.py:263-275) -> device-resident Batch with CSR plans."""
        if isinstance(inputs, Batch):
            return inputs
        if len(inputs) != 10:
            raise ValueError(f"expected the reference's 10-tuple input, got {len(inputs)} items")
        c, cei, cef, v, k, kei, kef, n_cons, n_vars, n_cuts = inputs
        dev = self.device
        if not any(isinstance(x, torch.Tensor) for x in (c, cei, cef, v, k, kei, kef)):
            for name, x, kind in (("cons_edge_inds", cei, "iu"), ("cut_edge_inds", kei, "iu")):
                if np.asarray(x).dtype.kind not in kind:
                    raise ValueError(f"{name} must be an integer array, got {np.asarray(x).dtype}")
            f32, i32 = np.float32, np.int32
            c, cei, cef, v, k, kei, kef = self._stage_host_arrays(
                [(c, f32), (cei, i32), (cef, f32), (v, f32), (k, f32), (kei, i32), (kef, f32)])
        else:
            c, v, k = (_as_device(x, torch.float32, dev) for x in (c, v, k))
            cei, kei = _as_device(cei, torch.int32, dev), _as_device(kei, torch.int32, dev)
            cef, kef = _as_device(cef, torch.float32, dev), _as_device(kef, torch.float32, dev)
        check_feature_shapes(c, v, k, n_cons, n_vars, n_cuts)
        return Batch(c, v, k, BipartiteGraph(cei, cef, c.shape[0], v.shape[0], validate),
                     BipartiteGraph(kei, kef, k.shape[0], v.shape[0], validate))

    # ---- workspaces --------------------------------------------------------------------------------------------
    def _take_workspace(self, batch):
        need = _lib.lib().gcnn_workspace_floats(C.byref(batch.dims))
        if need == 0:   # the size function's refusal (a negative count): no workspace is sized from it
            raise _lib.GcnnError(f"gcnn_workspace_floats refused the batch's sizes {tuple(getattr(batch.dims, f) for f, _ in _lib.Dims._fields_)}")
        best = None
        for i, ws in enumerate(self._ws_pool):
            if ws.numel() >= need and (best is None or ws.numel() < self._ws_pool[best].numel()):
                best = i
        if best is not None:
            return self._ws_pool.pop(best)
        try:
            return torch.empty(max(need, 4), dtype=torch.float32, device=self.device)
        except torch.OutOfMemoryError:
            self._ws_pool.clear()
            torch.cuda.empty_cache()
            return torch.empty(max(need, 4), dtype=torch.float32, device=self.device)

    def _give_workspace(self, ws):
        self._ws_pool.append(ws)
        if len(self._ws_pool) > 2:
            self._ws_pool.sort(key=lambda t: t.numel())
            self._ws_pool.pop(0)

    # ---- forward / backward ------------------------------------------------------------------------------------
    def _forward_into(self, flat, batch, ws, save=True):
        scores = torch.empty(batch.dims.n_cuts, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gcnn_forward(C.byref(batch.dims), _ptr(flat), _ptr(batch.cons_feats),
                                               _ptr(batch.var_feats), _ptr(batch.cut_feats), C.byref(batch.cons_graph.c),
                                               C.byref(batch.cut_graph.c), _ptr(ws), ws.numel(), _ptr(scores),
                                               int(save), _stream(self.device)), "gcnn_forward")
        return scores

    def _forward_loss_into(self, flat, batch, ws, targets, loss_scale):
        """Forward with the MSE head fused into its last launch (gcnn_forward_loss); continue with
        `_backward_into(d_scores=None, ..., loss_out=...)`."""
        scores = torch.empty(batch.dims.n_cuts, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gcnn_forward_loss(C.byref(batch.dims), _ptr(flat), _ptr(batch.cons_feats),
                                                    _ptr(batch.var_feats), _ptr(batch.cut_feats), C.byref(batch.cons_graph.c),
                                                    C.byref(batch.cut_graph.c), _ptr(ws), ws.numel(), _ptr(scores),
                                                    _ptr(targets), float(loss_scale), _stream(self.device)), "gcnn_forward_loss")
        return scores

    def _backward_into(self, flat, batch, ws, d_scores, grads, count_slot=None, loss_out=None, adam=None):
        """`adam`: optional `_lib.AdamArgs` -- the optimizer step then rides in the backward's last launch."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gcnn_backward(C.byref(batch.dims), _ptr(flat), _ptr(batch.cons_feats),
                                                _ptr(batch.var_feats), _ptr(batch.cut_feats), C.byref(batch.cons_graph.c),
                                                C.byref(batch.cut_graph.c), _ptr(ws), ws.numel(), _ptr(d_scores),
                                                _ptr(grads), _ptr(count_slot), _ptr(loss_out),
                                                C.byref(adam) if adam is not None else None, _stream(self.device)),
                       "gcnn_backward")

    def call(self, inputs, training=False):
        """GCNN.call (model.py:257-300): flat fp32 scores, one per candidate cut.  `training` is accepted and ignored
        exactly like the reference (no dropout / batch-norm).  Differentiable w.r.t. `flat_parameters` under autograd."""
        batch = self.prepare(inputs)
        if torch.is_grad_enabled() and self._flat.requires_grad:
            scores = _GCNNFunction.apply(self._flat, self, batch)
        else:
            ws = self._take_workspace(batch)
            scores = self._forward_into(self._flat.detach(), batch, ws, save=False)
            self._give_workspace(ws)
        return scores.as_subclass(ScoreTensor)

    def __call__(self, inputs, training=False):
        return self.call(inputs, training)

    # ---- PreNorm pretraining hooks (model.py:69-133, 384-437) --------------------------------------------------------
    def pretrain_init(self):
        """BaseModel.pretrain_init (model.py:69-87): every PreNorm layer starts waiting for updates."""
        self._prenorm_state = [dict(waiting=True, received=False, mean=np.zeros(u, np.float32), var=np.zeros(u, np.float32),
                                    count=np.float32(0)) for _, _, u in PRENORM_LAYERS]

    def _waiting_layer(self):
        """The PreNorm layer being fitted: the first one, in call order, that still waits for updates (None: none does)."""
        return next((i for i, st in enumerate(self._prenorm_state or ()) if st["waiting"]), None)

    def pretrain(self, inputs, training=True) -> bool:
        """BaseModel.pretrain (model.py:119-133): run the model; the first PreNorm layer (in call order) that is still
        waiting absorbs this batch's statistics (PreNormLayer.update_params, model.py:394-423) and the call stops there
        (the reference raises PreNormException).  Returns True when a layer absorbed the batch."""
        layer = self._waiting_layer()
        if layer is None:
            return False
        st = self._prenorm_state[layer]
        units = PRENORM_LAYERS[layer][2]
        batch = self.prepare(inputs)
        sample_count = prenorm_count(batch.dims, layer)
        st["received"] = True
        if sample_count == 0:
            return True
        ws = self._take_workspace(batch)
        flat = self._flat.detach()
        if layer >= 5:
            self._forward_into(flat, batch, ws, save=2)   # 2: the two-layer form that materialises A (the post-conv PreNorm's input)
        out = torch.empty(2 * units, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gcnn_prenorm_stats(C.byref(batch.dims), _ptr(flat), _ptr(batch.cons_feats),
                                                     _ptr(batch.var_feats), _ptr(batch.cut_feats), C.byref(batch.cons_graph.c),
                                                     C.byref(batch.cut_graph.c), _ptr(ws), ws.numel(), layer, _ptr(out),
                                                     _stream(self.device)), "gcnn_prenorm_stats")
        host = out.cpu().numpy()
        self._give_workspace(ws)
        # streaming merge of Chan et al. in fp32, exactly the arithmetic of model.py:415-423
        f = np.float32
        sample_mean, sample_var, sample_count = host[:units].astype(f), host[units:].astype(f), f(sample_count)
        delta = sample_mean - st["mean"]
        m2 = st["var"] * st["count"] + sample_var * sample_count + delta ** 2 * st["count"] * sample_count / (st["count"] + sample_count)
        st["count"] = f(st["count"] + sample_count)
        st["mean"] = (st["mean"] + delta * sample_count / st["count"]).astype(f)
        st["var"] = (m2 / st["count"]).astype(f)
        return True

    def pretrain_sync(self, process_group):
        """Data-parallel fitting: merge the statistics of the layer that is absorbing updates across the ranks of
        `process_group` (every rank saw only its shard of the pretraining batches).  Call once per pass, on every rank,
        before `pretrain_next`.  The merge is the same Chan update as between batches (model.py:415-423), in rank order."""
        layer = self._waiting_layer()
        if layer is None or process_group is None:   # (identical on every rank: only this method's callers change the fitted set)
            return
        from .parallel import allgather_prenorm
        st = self._prenorm_state[layer]
        st["count"], st["mean"], st["var"], st["received"] = allgather_prenorm(st["count"], st["mean"], st["var"], st["received"],
                                                                              process_group, self.device)

    def pretrain_next(self):
        """BaseModel.pretrain_next (model.py:89-117): freeze the layer that just received updates
        (PreNormLayer.stop_updates, model.py:425-437: shift = -mean, scale = 1/sqrt(var), var == 0 -> 1)."""
        if self._prenorm_state is None:
            return None
        for i, st in enumerate(self._prenorm_state):
            if st["waiting"] and st["received"]:
                shift_name, scale_name, units = PRENORM_LAYERS[i]
                var = np.where(st["var"] == 0, np.float32(1), st["var"]).astype(np.float32)
                with torch.no_grad():
                    if shift_name is not None:
                        self.get_variable(shift_name).copy_(torch.from_numpy((-st["mean"]).astype(np.float32)))
                    self.get_variable(scale_name).copy_(torch.from_numpy((1 / np.sqrt(var)).astype(np.float32)))
                st["waiting"] = False
                return i, scale_name.rsplit("/", 1)[0]
        return None

    # Below this many cuts the descending stable ranking is done on the host (a stable NumPy argsort of a few dozen floats takes
    # ~2 us; the device ranking kernel costs a launch plus a dependent kernel in the chain: ~10 us end to end, tools/latency.py)
    HOST_RANK_MAX = 1024

    def _sess(self, attr, cls):
        """The session kept in attribute `attr` (pinned staging + device arena), created on first use."""
        if getattr(self, attr) is None:
            setattr(self, attr, cls(self))
        return getattr(self, attr)

    def _rank_on_device(self, rank, n_cuts):
        return bool(rank) and (rank == "device" or n_cuts > self.HOST_RANK_MAX)

    @staticmethod
    def _check_select_size(entry, noun, n_cuts):
        if n_cuts > ops.SELECT_MAX_CUTS:
            raise _lib.GcnnError(f"{entry}: the {noun} has {n_cuts} cuts; the device selection handles at most "
                                 f"{ops.SELECT_MAX_CUTS} and there is no CPU fallback")

    def _select_general(self, state, packed, p_max, p_max_ub, n_cuts):
        """The selection on the general path -- prepare + forward + gcnn_select_cuts -- for a state the single calls decline, device
        tensors and prepared `Batch`es: (scores, order, n_kept) as host values.  `packed`: the forced rows (normalize_forced)."""
        with torch.no_grad():
            batch = self.prepare(state)
            scores_dev = self.call(batch, False).as_subclass(torch.Tensor)
            forced_dev = tuple(torch.from_numpy(a).to(self.device) for a in packed)
            order, n_kept = ops.select_cuts(scores_dev, batch.cut_graph, None, forced_dev, p_max=p_max, p_max_ub=p_max_ub,
                                            max_cuts=n_cuts)
            return scores_dev.cpu().numpy().view(ScoreArray), order.cpu().numpy(), int(n_kept.cpu()[0])

    def score_state(self, inputs, rank=False):
        """Scores of ONE sampled state given as host arrays (the SCIP plugins' call, model_evaluator.py:84-111), through the
        single-call path gcnn_infer: one upload, a three-launch graph plan, the inference forward pass, one download.
        Returns a `ScoreArray` (ndarray with `.numpy()`); with `rank=True` its `.rankings` holds the cut indices in descending
        score order (ties in index order): computed by the device ranking kernel for more than HOST_RANK_MAX cuts or with
        `rank="device"`, else by a stable argsort on the host (faster for a few dozen cuts).  States the specialised plan declines (edge lists not sorted by row, more than
        32,768 variables, ...) run through `prepare` + the general forward pass instead; results are identical."""
        on_device = self._rank_on_device(rank, int(np.asarray(inputs[4]).shape[0]))
        try:
            scores = self._sess("_session", _InferenceSession).run(inputs, on_device)
        except _UseGeneralPath:
            on_device = False
            with torch.no_grad():
                scores = self.call(inputs, False).numpy().view(ScoreArray)
        if rank and not on_device:
            scores.rankings = stable_ranking(scores)
        return scores

    def select_cuts(self, state, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        """Score ONE state and run the parallelism filter of the SCIP plugin's cutselselect (model_evaluator.py:109-154) on the
        device.  `forced`: None or (edge_inds [2,E], values [E], n_forced) -- the forced cuts' rows built as get_state builds the
        cut edges (coefficient / norm over LP column positions); (edge_inds, values) alone takes n_forced = max row id + 1.
        Host arrays take the single call gcnn_infer_select (one upload, one download); states it declines, device tensors and
        prepared `Batch`es take prepare + forward + gcnn_select_cuts.  Both give the same bits.  Returns a `SelectResult`."""
        ops.check_thresholds(p_max, p_max_ub)
        n_cuts = state.dims.n_cuts if isinstance(state, Batch) else int(state[4].shape[0])
        n_vars = state.dims.n_vars if isinstance(state, Batch) else int(state[3].shape[0])
        self._check_select_size("select_cuts", "state", n_cuts)
        packed = normalize_forced(forced, n_vars)
        result = None
        if is_host_state(state):
            try:
                result = self._sess("_session", _InferenceSession).run_select(state, packed, p_max, p_max_ub)
            except _UseGeneralPath:
                pass
        scores, order, n_kept = result or self._select_general(state, packed, p_max, p_max_ub, n_cuts)
        return SelectResult(order, n_kept, n_selected(n_kept, max_selected), scores)

    # ---- from a raw LP snapshot (lpstate.LPSnapshot): get_state's arithmetic on the device, in front of the same calls ---------
    def _lp(self):
        return self._sess("_lp_session", _LPSession)

    def state_from_lp(self, snapshot):
        """The model's 10-tuple as host arrays, built on the device from an `LPSnapshot` (gcnn_lp_state: utils.get_state's
        arithmetic, utils.py:35-238), and `cut_index` (int32: state position -> input cut).  What a sample writer stores
        (`utils.inputs_to_state` + `utils.save_sample`).  Raises ValueError for a snapshot that breaks its contract."""
        state, cut_index = self._lp().build_state(snapshot)
        return tuple(t.cpu().numpy() for t in state[:7]) + state[7:], cut_index.cpu().numpy()

    def score_lp(self, snapshot, rank=False):
        """`score_state` from an `LPSnapshot`: ONE upload of the packed snapshot, two launches build the state where gcnn_infer
        keeps its uploaded arrays, then the same plan and forward pass, one download (gcnn_lp_infer).  Scores are in STATE order;
        `.cut_index[p]` is the input cut at state position p, `.rankings` (with `rank`) as `score_state` gives them.  A snapshot
        past gcnn_infer's limits, or one whose state the specialised plan declines, is built with gcnn_lp_state and goes through
        `prepare` + the general forward pass as device tensors; the bits are the same."""
        on_device = self._rank_on_device(rank, int(np.asarray(snapshot.cut_lhs).shape[0]))
        try:
            scores, order, _, cut_index = self._lp().run(snapshot, on_device)
        except _UseGeneralPath:
            on_device = False
            state, cut_index = self._lp().build_state(snapshot)
            with torch.no_grad():
                scores = self.call(state, False).numpy().view(ScoreArray)
            cut_index = cut_index.cpu().numpy()
        scores.cut_index = cut_index
        if rank:
            scores.rankings = order if on_device else stable_ranking(scores)
        return scores

    def select_cuts_lp(self, snapshot, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        """`select_cuts` from an `LPSnapshot` (gcnn_lp_infer_select).  `forced` as `select_cuts` takes it.  The `SelectResult`'s
        `order` is in STATE order and it carries `cut_index`: `cut_index[order[:n_selected]]` are the selected input cuts."""
        ops.check_thresholds(p_max, p_max_ub)
        n_cuts, n_vars = int(np.asarray(snapshot.cut_lhs).shape[0]), int(np.asarray(snapshot.col_type).shape[0])
        self._check_select_size("select_cuts_lp", "snapshot", n_cuts)
        packed = normalize_forced(forced, n_vars)
        try:
            scores, order, n_kept, cut_index = self._lp().run(snapshot, True, None, packed, p_max, p_max_ub)
        except _UseGeneralPath:
            state, cut_index = self._lp().build_state(snapshot)
            scores, order, n_kept = self._select_general(state, packed, p_max, p_max_ub, n_cuts)
            cut_index = cut_index.cpu().numpy()
        return SelectResult(order, n_kept, n_selected(n_kept, max_selected), scores, cut_index)

    def collect_lp(self, snapshot, quality, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        """An expert round of the data collector (data_collector.py:101-195): `collect.Collector.collect_lp` on this model's
        device -- the sample's state and the plugin's selection over the expert's float64 `quality`, in one call.  No parameter
        of the model is read: a process without a model uses a `Collector` directly."""
        if getattr(self, "_collector", None) is None:
            from .collect import Collector
            self._collector = Collector(self.device)
        return self._collector.collect_lp(snapshot, quality, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected)

    def open_lp(self, rows, *, deep=True):
        """Keep an LP on the device across the separation rounds of one node: `rows` (`lpstate.LPRows`) goes up once, every
        `lpstate.LPRound` then uploads only the solve and the candidate cuts.  Returns an `LPSession` (infer.py): `state`, `score`,
        `select_cuts`, `append_rows`, `close`; a round's result is `state_from_lp` / `score_lp` / `select_cuts_lp` on
        `lpstate.assemble(rows, round)`, bit for bit.  Rows can only be appended: any other change of the LP means a new session.
        `deep`: check the O(nnz) facts (columns in range and strictly increasing) on the host too; without it the device finds
        them and the call raises ValueError after the download."""
        return LPSession(self, rows, deep)

    # ---- many host states in one call (gcnn_infer_batch): what a scoring server does with the requests that queued up ----------
    @staticmethod
    def _admit_state(st, mode):
        """A host state for the batched call: (arrays, key), or None where it goes to the solo entry point."""
        if not is_host_state(st) or len(st) != 10:
            return None                     # device tensors, prepared batches, malformed tuples: the solo path answers (or raises)
        arrays, key = check_state(st)
        n_cuts = key[2]
        declined = n_cuts == 0 or (mode != _lib.IBATCH_SCORES and n_cuts > 4096) or edges_without_nodes(key)
        return None if declined else (arrays, key)

    def _many(self, states, mode, solo, forced=None, p_max=0.0, p_max_ub=0.0, lp=False):
        """Common part of `score_states` / `select_cuts_many` and, with `lp`, of `score_lps` / `select_cuts_lp_many`: results per
        state -- ("ok", scores, order, n_kept[, cut_index]), or an exception.
        `solo(i)`: the existing single-state entry point for state i (a state the batch declines goes there and comes back in
        place).  `forced`: None or per state a packed (ptr, col, val) / an exception raised while it was packed."""
        session = self._sess("_lp_batch_session", _LPBatchSession) if lp else self._sess("_batch_session", _BatchSession)

        def admit(i):
            if forced is not None and isinstance(forced[i], Exception):
                raise forced[i]
            if not lp:
                return self._admit_state(states[i], mode)
            entry = session.check(states[i])
            n_cuts = entry[1]["n_cuts"]
            return None if n_cuts == 0 or (mode != _lib.IBATCH_SCORES and n_cuts > 4096) else entry

        def run(ids, checked):
            return session.run([checked[i] for i in ids], None if forced is None else [forced[i] for i in ids], mode, p_max, p_max_ub)

        return _serve_many(len(states), admit, lambda ids: [ids[j:j + session.MAX] for j in range(0, len(ids), session.MAX)], run, solo)

    @staticmethod
    def _finish_many(results, return_exceptions):
        if not return_exceptions:
            for r in results:
                if isinstance(r, Exception):
                    raise r
        return results

    def score_states(self, states, rank=False, return_exceptions=False):
        """`score_state` for many host states at once: one upload, ONE forward pass over their disjoint union, one download
        (gcnn_infer_batch; up to 64 states per call, more are served in several calls).  Returns a list of `ScoreArray`, with
        `.rankings` when `rank`.  Errors are per state: with `return_exceptions=True` a state's exception (e.g. the ValueError
        of an out-of-range index) sits in its slot; otherwise the first one is raised after every state has been served.  States
        the batch declines (no cuts, more than 4,096 cuts when ranking, ...) go through `score_state` and come back in place."""
        states = list(states)
        mode = _lib.IBATCH_RANK if rank else _lib.IBATCH_SCORES
        results = self._many(states, mode, lambda i: self.score_state(states[i], rank))
        return self._finish_many(_as_scores(results, rank), return_exceptions)

    def select_cuts_many(self, states, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        """`select_cuts` for many host states at once (gcnn_infer_batch in selection mode).  `forced`: None, or one entry per state
        in the forms `select_cuts` accepts (None = no forced rows).  Returns a list of `SelectResult`; errors per state as in
        `score_states` (a state with more than 4,096 cuts holds the `GcnnError` `select_cuts` raises for it)."""
        ops.check_thresholds(p_max, p_max_ub)
        states = list(states)
        forced, packed = _packed_forced(states, forced, _state_vars, "state")

        def solo(i):
            return self.select_cuts(states[i], forced[i], p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected)

        results = self._many(states, _lib.IBATCH_SELECT, solo, packed, p_max, p_max_ub)
        return self._finish_many(_as_selections(results, max_selected), return_exceptions)

    # ---- many LP snapshots in one call (gcnn_lp_batch): what a scoring server does with the snapshots that queued up ----------
    def score_lps(self, snapshots, rank=False, return_exceptions=False):
        """`score_lp` for many `LPSnapshot`s at once: one upload of the packed snapshots, two launches build all their states where
        gcnn_infer_batch keeps its uploaded ones, ONE forward pass over the union, one download (gcnn_lp_batch; up to 64 per call,
        more are served in several calls).  Returns a list of `ScoreArray` in STATE order with `.cut_index`, and `.rankings` when
        `rank`.  There is no variable limit.  Errors per snapshot as in `score_states`.  Snapshots the batch declines (no cuts,
        more than 4,096 cuts when ranking) go through `score_lp` and come back in place."""
        snapshots = list(snapshots)
        mode = _lib.IBATCH_RANK if rank else _lib.IBATCH_SCORES
        results = self._many(snapshots, mode, lambda i: self.score_lp(snapshots[i], rank), lp=True)
        return self._finish_many(_as_scores(results, rank, cut_index=True), return_exceptions)

    def select_cuts_lp_many(self, snapshots, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        """`select_cuts_lp` for many `LPSnapshot`s at once (gcnn_lp_batch in selection mode).  `forced`: None, or one entry per
        snapshot in the forms `select_cuts` accepts.  Returns a list of `SelectResult` with `.cut_index`; errors per snapshot as in
        `select_cuts_many`."""
        ops.check_thresholds(p_max, p_max_ub)
        snapshots = list(snapshots)
        forced, packed = _packed_forced(snapshots, forced, _snapshot_vars, "snapshot")

        def solo(i):
            return self.select_cuts_lp(snapshots[i], forced[i], p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected)

        results = self._many(snapshots, _lib.IBATCH_SELECT, solo, packed, p_max, p_max_ub, lp=True)
        return self._finish_many(_as_selections(results, max_selected, cut_index=True), return_exceptions)

    def get_concrete_function(self):
        """Counterpart of `tf.function(model.call).get_concrete_function()` (model_evaluator.py:310-311): an inference
        callable `(state10, training) -> scores` with `.numpy()`.  Host arrays (what `get_state` produces) take the
        single-call path `score_state`; device tensors / prepared batches the general forward pass."""
        def get_improvements(state, training=False, rank=False):
            if is_host_state(state):
                return self.score_state(state, rank)
            with torch.no_grad():
                return self.call(state, training)
        return get_improvements


class ModelSet:
    """Several models behind one call: `ModelSet({"setcov/0": m0, "setcov/1": m1, ...})`.  The evaluators' task farm runs `seed`
    innermost (model_evaluator.py:211-219), so the states that wait at a scoring server belong to different models; `score_states`
    and `select_cuts_many` take them together with the key of each state's model and answer them with ONE gcnn_infer_models call
    per 8 models / 64 states: one upload, one index pass and one by-variable stage, the models' forward passes as a group, one
    download.  Every state's result has the bits of its own model's `GCNN.score_states` / `select_cuts_many` on that model's
    states alone.  `score_lps` and `select_cuts_lp_many` are the same for raw `LPSnapshot`s (gcnn_lp_models: the states are built
    on the device in front of the same work), with the bits of `GCNN.score_lps` / `select_cuts_lp_many`.  `score_ensemble`,
    `select_cuts_ensemble` and their LP forms let up to 8 of the models score ONE state and rank or select by the mean of their
    scores, in one call (gcnn_infer_ensemble / gcnn_lp_ensemble); `open_lp_ensemble` keeps an LP resident for such an ensemble
    (gcnn_lp_round_ensemble); `score_ensemble_many`, `select_cuts_ensemble_many` and their LP forms answer up to 64 states per call
    with one such ensemble (gcnn_infer_ensemble_batch / gcnn_lp_ensemble_batch).  All models live on one device."""
    MAX_MODELS = _ModelsSession.MAX_MODELS

    def __init__(self, models):
        self.models = dict(models)
        if not self.models:
            raise ValueError("ModelSet: no model")
        devices = {str(m.device) for m in self.models.values()}
        if len(devices) != 1:
            raise ValueError(f"ModelSet: all models must be on one device, got {sorted(devices)}")
        self._number = {k: i for i, k in enumerate(self.models)}
        self._session = None
        self._lp_session = None
        self._ensemble = None             # the sessions of the `*_ensemble` methods, built on first use
        self._lp_ensemble = None
        self._ensemble_batch = None       # the sessions of the `*_ensemble_many` methods, built on first use
        self._lp_ensemble_batch = None
        self._lp_rounds = None            # the LPSessionGroup of `score_rounds` / `select_cuts_rounds`, built on first use
        self.calls = 0                    # gcnn_infer_models and gcnn_lp_models calls made
        self.max_models_per_call = 0      # the most models one of them served

    def _sess(self, lp=False):
        first = next(iter(self.models.values()))
        if lp:
            if self._lp_session is None:
                self._lp_session = _LPModelsSession(first._sess("_lp_batch_session", _LPBatchSession))
            return self._lp_session
        if self._session is None:
            self._session = _ModelsSession(first._sess("_batch_session", _BatchSession))
        return self._session

    def _many(self, keys, states, mode, solo, forced=None, p_max=0.0, p_max_ub=0.0, lp=False):
        """`GCNN._many` over states -- with `lp`, LP snapshots -- of several models: results per state in the caller's order."""
        if len(keys) != len(states):
            raise ValueError(f"keys: one model key per state expected, got {len(keys)} for {len(states)} states")
        session = self._sess(lp)
        more = dict(lp=True) if lp else {}

        def admit(i):
            if keys[i] not in self.models:
                raise KeyError(f"no model {keys[i]!r}")
            if forced is not None and isinstance(forced[i], Exception):
                raise forced[i]
            if not lp:
                return GCNN._admit_state(states[i], mode)
            entry = session.base.check(states[i])
            n_cuts = entry[1]["n_cuts"]
            return None if n_cuts == 0 or (mode != _lib.IBATCH_SCORES and n_cuts > 4096) else entry

        def split(ids):
            """Sorted stably by model (a model's states keep their relative order), at most 8 models and 64 states per call."""
            calls, cur, cur_models = [], [], set()
            for i in sorted(ids, key=lambda i: self._number[keys[i]]):
                if len(cur) == session.MAX or (keys[i] not in cur_models and len(cur_models) == self.MAX_MODELS):
                    calls.append(cur)
                    cur, cur_models = [], set()
                cur.append(i)
                cur_models.add(keys[i])
            return calls + [cur] if cur else calls

        def run(ids, checked):
            order = list(dict.fromkeys(keys[i] for i in ids))     # the call's models, numbered as they appear
            number = {k: m for m, k in enumerate(order)}
            got = session.run([checked[i] for i in ids], None if forced is None else [forced[i] for i in ids], mode,
                              [number[keys[i]] for i in ids], [self.models[k] for k in order], p_max, p_max_ub)
            if got is session.UNSUPPORTED:      # the grouped forward declines: one call per model, each with its own solo tail
                got = [None] * len(ids)
                for k in order:
                    mine = [j for j, i in enumerate(ids) if keys[i] == k]
                    sub = self.models[k]._many([states[ids[j]] for j in mine], mode, lambda x, mine=mine: solo(ids[mine[x]]),
                                               None if forced is None else [forced[ids[j]] for j in mine], p_max, p_max_ub, **more)
                    for j, r in zip(mine, sub):
                        got[j] = ("error", r) if isinstance(r, Exception) else r
            elif got is not None:
                self.calls += 1
                self.max_models_per_call = max(self.max_models_per_call, len(order))
            return got

        return _serve_many(len(states), admit, split, run, solo)

    def score_states(self, keys, states, rank=False, return_exceptions=False):
        """`GCNN.score_states` for states of several models: `keys[i]` names the model of `states[i]`, in any order.  Returns a
        list of `ScoreArray` in the caller's order, with `.rankings` when `rank`; errors per state as `GCNN.score_states` reports
        them (an unknown key is its state's KeyError).  States the call declines go through their own model's `score_state`."""
        keys, states = list(keys), list(states)
        mode = _lib.IBATCH_RANK if rank else _lib.IBATCH_SCORES
        results = self._many(keys, states, mode, lambda i: self.models[keys[i]].score_state(states[i], rank))
        return GCNN._finish_many(_as_scores(results, rank), return_exceptions)

    def select_cuts_many(self, keys, states, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        """`GCNN.select_cuts_many` for states of several models (`keys[i]` names the model of `states[i]`).  Returns a list of
        `SelectResult` in the caller's order."""
        ops.check_thresholds(p_max, p_max_ub)
        keys, states = list(keys), list(states)
        forced, packed = _packed_forced(states, forced, _state_vars, "state")

        def solo(i):
            return self.models[keys[i]].select_cuts(states[i], forced[i], p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected)

        results = self._many(keys, states, _lib.IBATCH_SELECT, solo, packed, p_max, p_max_ub)
        return GCNN._finish_many(_as_selections(results, max_selected), return_exceptions)

    # ---- LP snapshots of several models in one call (gcnn_lp_models) ------------------------------------------------------------
    def score_lps(self, keys, snapshots, rank=False, return_exceptions=False):
        """`GCNN.score_lps` for `LPSnapshot`s of several models: `keys[i]` names the model of `snapshots[i]`, in any order.  ONE
        gcnn_lp_models call per 8 models / 64 snapshots: one upload of the packed snapshots, two launches build every state where
        gcnn_infer_models keeps its uploaded ones, then that call's device work, one download.  Returns a list of `ScoreArray` in
        the caller's order, each in STATE order with `.cut_index`, and `.rankings` when `rank`; errors per snapshot as
        `GCNN.score_lps` reports them (an unknown key is its snapshot's KeyError).  Snapshots the call declines go through their
        own model's `score_lp`."""
        keys, snapshots = list(keys), list(snapshots)
        mode = _lib.IBATCH_RANK if rank else _lib.IBATCH_SCORES
        results = self._many(keys, snapshots, mode, lambda i: self.models[keys[i]].score_lp(snapshots[i], rank), lp=True)
        return GCNN._finish_many(_as_scores(results, rank, cut_index=True), return_exceptions)

    def select_cuts_lp_many(self, keys, snapshots, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        """`GCNN.select_cuts_lp_many` for `LPSnapshot`s of several models (`keys[i]` names the model of `snapshots[i]`).  Returns
        a list of `SelectResult` with `.cut_index`, in the caller's order."""
        ops.check_thresholds(p_max, p_max_ub)
        keys, snapshots = list(keys), list(snapshots)
        forced, packed = _packed_forced(snapshots, forced, _snapshot_vars, "snapshot")

        def solo(i):
            return self.models[keys[i]].select_cuts_lp(snapshots[i], forced[i], p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected)

        results = self._many(keys, snapshots, _lib.IBATCH_SELECT, solo, packed, p_max, p_max_ub, lp=True)
        return GCNN._finish_many(_as_selections(results, max_selected, cut_index=True), return_exceptions)

    # ---- rounds of resident LPs of several models in one call (gcnn_lp_rounds) ---------------------------------------------------
    def _rounds(self, keys, sessions, batch_removes=False):
        """The set's `LPSessionGroup`, once `keys` (taken for symmetry with the other methods: a session knows its model) name the
        sessions' models.  `batch_removes`: how this call's members with a removal are served (`LPSessionGroup`)."""
        keys, sessions = list(keys), list(sessions)
        if len(keys) != len(sessions):
            raise ValueError(f"keys: one model key per session expected, got {len(keys)} for {len(sessions)} sessions")
        if any(isinstance(s, LPEnsembleSession) for s in sessions):
            raise ValueError("an ensemble session's rounds take its own call; grouping them is not supported")
        for k, s in zip(keys, sessions):
            if k not in self.models:
                raise KeyError(f"no model {k!r}")
            if s.model is not self.models[k]:
                raise ValueError(f"the session was not opened on model {k!r}")
        if self._lp_rounds is None:
            self._lp_rounds = LPSessionGroup(next(iter(self.models.values())).device)
        self._lp_rounds.batch_removes = bool(batch_removes)
        return self._lp_rounds, sessions

    def score_rounds(self, keys, sessions, rounds, rank=False, appends=None, return_exceptions=False, removes=None, batch_removes=False):
        """`LPSessionGroup.score` over sessions opened on this set's models (`models[keys[i]].open_lp(...)`): the rounds of up to 8
        sessions per call, whatever their models; entry i has the bits of `sessions[i].score(rounds[i], rank, append=appends[i],
        remove=removes[i])`.  A member with a removal takes its solo call unless `batch_removes` (gcnn_lp_rounds_edit)."""
        group, sessions = self._rounds(keys, sessions, batch_removes)
        return group.score(sessions, rounds, rank, appends, return_exceptions, removes=removes)

    def select_cuts_rounds(self, keys, sessions, rounds, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, appends=None,
                           return_exceptions=False, removes=None, batch_removes=False):
        """`LPSessionGroup.select_cuts` over sessions opened on this set's models; entry i has the bits of
        `sessions[i].select_cuts(rounds[i], forced[i], ..., append=appends[i], remove=removes[i])`; removals as in `score_rounds`."""
        group, sessions = self._rounds(keys, sessions, batch_removes)
        return group.select_cuts(sessions, rounds, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected, appends=appends,
                                 return_exceptions=return_exceptions, removes=removes)

    # ---- ensembles: ONE state scored by several of the set's models, the mean ranked or selected once ----------------------------
    def ensemble_session(self, lp=False):
        """The session behind the `*_ensemble` methods (`_EnsembleSession`; with `lp`, `_LPEnsembleSession`): its `calls` and
        `upload_bytes` count the one-call path's C calls and state uploads."""
        first = next(iter(self.models.values()))
        if lp:
            if self._lp_ensemble is None:
                self._lp_ensemble = _LPEnsembleSession(first._sess("_lp_batch_session", _LPBatchSession))
            return self._lp_ensemble
        if self._ensemble is None:
            self._ensemble = _EnsembleSession(first._sess("_batch_session", _BatchSession))
        return self._ensemble

    def _ensemble_models(self, keys):
        """The models of an ensemble in the caller's order; ValueError before any device work for zero or more than 8 keys, a
        duplicate key and an unknown key."""
        keys = list(keys)
        if not 1 <= len(keys) <= self.MAX_MODELS:
            raise ValueError(f"an ensemble holds 1..{self.MAX_MODELS} models, got {len(keys)}")
        if len(set(keys)) != len(keys):
            raise ValueError(f"an ensemble names every model once, got {keys!r}")
        for k in keys:
            if k not in self.models:
                raise ValueError(f"no model {k!r}")
        return [self.models[k] for k in keys]

    def open_lp_ensemble(self, keys, rows, *, deep=True):
        """`GCNN.open_lp` for an ensemble: keep `rows` (`lpstate.LPRows`) on the device across the separation rounds of one node
        and let the models `keys` (1..8, each once, in this order) score every round together.  Returns an `LPEnsembleSession`
        (infer.py): `score` and `select_cuts` give what `score_lp_ensemble` / `select_cuts_lp_ensemble` give for `keys` on
        `lpstate.assemble(rows, round)`, bit for bit, from the plain session's upload of the round (gcnn_lp_round_ensemble);
        rows are appended and removed as in an `LPSession`.  ValueError before any device work for zero or more than 8 keys, a
        duplicate or unknown key and models on different devices.  The session takes its device from the first model and
        reads each model's current parameters every round."""
        return LPEnsembleSession(self._ensemble_models(keys), rows, deep)

    @staticmethod
    def _ensemble_general(models, state, packed, p_max, p_max_ub, n_cuts):
        """The general path of an ensemble -- `prepare` once, `trainer.forward_group` over the models with that one batch,
        `ops.ensemble_mean`, and with `packed` forced rows gcnn_select_cuts over the mean: (mean, order | None, n_kept | None,
        members) as host values, with the bits of the one-call path."""
        from . import trainer
        first = models[0]
        with torch.no_grad():
            batch = first.prepare(state)
            rows = trainer.forward_group(models, [batch] * len(models))
            mean = ops.ensemble_mean(rows)
            order = n_kept = None
            if packed is not None:
                forced_dev = tuple(torch.from_numpy(a).to(first.device) for a in packed)
                order, n_kept = ops.select_cuts(mean, batch.cut_graph, None, forced_dev, p_max=p_max, p_max_ub=p_max_ub, max_cuts=n_cuts)
                order, n_kept = order.cpu().numpy(), int(n_kept.cpu()[0])
            members = torch.stack(rows).cpu().numpy() if rows else np.zeros((0, n_cuts), np.float32)
            return mean.cpu().numpy().view(ScoreArray), order, n_kept, members

    @staticmethod
    def _empty_ensemble(n_models, select, max_selected=None, cut_index=None):
        """The answer for a state without cuts."""
        scores = np.zeros(0, np.float32).view(ScoreArray)
        members = np.zeros((n_models, 0), np.float32)
        if select:
            res = SelectResult(np.zeros(0, np.int32), 0, n_selected(0, max_selected), scores, cut_index)
            res.members = members
            return res
        scores.members, scores.cut_index = members, cut_index
        return scores

    def _score_ensemble(self, models, state, rank, lp, timings=None):
        first = models[0]
        if lp:
            n_cuts = int(np.asarray(state.cut_lhs).shape[0])
        else:
            n_cuts = state.dims.n_cuts if isinstance(state, Batch) else int(state[4].shape[0])
        on_device = first._rank_on_device(rank, n_cuts) and n_cuts <= ops.SELECT_MAX_CUTS
        cut_index = None
        if n_cuts == 0:
            if lp:
                self.ensemble_session(True).base.check(state)
            scores = self._empty_ensemble(len(models), False, cut_index=np.zeros(0, np.int32) if lp else None)
            if rank:
                scores.rankings = np.zeros(0, np.int32)
            return scores
        got = None
        if lp or is_host_state(state):
            try:
                got = self.ensemble_session(lp).run(state, None, _lib.IBATCH_RANK if on_device else _lib.IBATCH_SCORES, models,
                                                    timings=timings)
            except _UseGeneralPath:
                pass
        if got is None:
            on_device = False
            if lp:
                state, cut_index = first._lp().build_state(state)
                cut_index = cut_index.cpu().numpy()
            got = self._ensemble_general(models, state, None, 0.0, 0.0, n_cuts)
        elif lp:
            cut_index = got[4]
        scores, order, _, members = got[:4]
        scores.members, scores.cut_index = members, cut_index
        if rank:
            scores.rankings = order if on_device else stable_ranking(scores)
        return scores

    def _select_ensemble(self, models, state, forced, p_max, p_max_ub, max_selected, lp, timings=None):
        ops.check_thresholds(p_max, p_max_ub)
        first = models[0]
        if lp:
            n_cuts, n_vars = int(np.asarray(state.cut_lhs).shape[0]), _snapshot_vars(state)
        else:
            n_cuts = state.dims.n_cuts if isinstance(state, Batch) else int(state[4].shape[0])
            n_vars = state.dims.n_vars if isinstance(state, Batch) else int(state[3].shape[0])
        first._check_select_size("select_cuts_lp_ensemble" if lp else "select_cuts_ensemble", "snapshot" if lp else "state", n_cuts)
        packed = normalize_forced(forced, n_vars)
        cut_index = None
        if n_cuts == 0:
            if lp:
                self.ensemble_session(True).base.check(state)
            return self._empty_ensemble(len(models), True, max_selected, np.zeros(0, np.int32) if lp else None)
        got = None
        if lp or is_host_state(state):
            try:
                got = self.ensemble_session(lp).run(state, packed, _lib.IBATCH_SELECT, models, p_max, p_max_ub, timings=timings)
            except _UseGeneralPath:
                pass
        if got is None:
            if lp:
                state, cut_index = first._lp().build_state(state)
                cut_index = cut_index.cpu().numpy()
            got = self._ensemble_general(models, state, packed, p_max, p_max_ub, n_cuts)
        elif lp:
            cut_index = got[4]
        scores, order, n_kept, members = got[:4]
        result = SelectResult(order, n_kept, n_selected(n_kept, max_selected), scores, cut_index)
        result.members = members
        return result

    def score_ensemble(self, keys, state, rank=False, timings=None):
        """ONE state scored by the models `keys` (1..8, each once, in this order) and averaged: the reference trains five seeds per
        problem (model_trainer.py:38-49) and this lets all of them score the same round.  Returns a `ScoreArray` holding the mean
        -- acc = member[0], acc += member[m] in the order of `keys`, acc / float32(M), all in fp32 --, with `.members` (float32
        [M, K]: row m has the bits of `score_states(keys, [state] * M)[m]`) and, with `rank`, `.rankings` of the mean as
        `GCNN.score_state` gives them.  A host state takes ONE gcnn_infer_ensemble call: one upload of the state, one graph plan,
        the M forward passes as one group, one download.  States that call declines, device tensors and prepared `Batch`es take
        `prepare` once + `trainer.forward_group` + `ops.ensemble_mean`; the bits are the same."""
        return self._score_ensemble(self._ensemble_models(keys), state, rank, False, timings)

    def select_cuts_ensemble(self, keys, state, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, timings=None):
        """`GCNN.select_cuts` over the mean of the models `keys` (as `score_ensemble` defines it): the plugin's ranking and
        parallelism filter (model_evaluator.py:109-154) run once, on the device, in the same call as the M forward passes.  Returns
        a `SelectResult` whose `scores` are the mean, with `.members`."""
        return self._select_ensemble(self._ensemble_models(keys), state, forced, p_max, p_max_ub, max_selected, False, timings)

    def score_lp_ensemble(self, keys, snapshot, rank=False, timings=None):
        """`score_ensemble` from an `LPSnapshot` (gcnn_lp_ensemble: one upload of the packed snapshot, the state built once on the
        device).  Results are in STATE order and carry `.cut_index`."""
        return self._score_ensemble(self._ensemble_models(keys), snapshot, rank, True, timings)

    def select_cuts_lp_ensemble(self, keys, snapshot, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, timings=None):
        """`select_cuts_ensemble` from an `LPSnapshot`; `order` is in STATE order and the result carries `.cut_index`."""
        return self._select_ensemble(self._ensemble_models(keys), snapshot, forced, p_max, p_max_ub, max_selected, True, timings)

    # ---- ensembles over many states: what waits at a farm's scoring server, scored by ONE ensemble in one call --------------------
    def ensemble_batch_session(self, lp=False):
        """The session behind the `*_ensemble_many` methods (`_EnsembleBatchSession`; with `lp`, `_LPEnsembleBatchSession`): its
        `calls`, `upload_bytes` and `max_states_per_call` count the one-call path's C calls, state uploads and widest call."""
        first = next(iter(self.models.values()))
        if lp:
            if self._lp_ensemble_batch is None:
                self._lp_ensemble_batch = _LPEnsembleBatchSession(first._sess("_lp_batch_session", _LPBatchSession))
            return self._lp_ensemble_batch
        if self._ensemble_batch is None:
            self._ensemble_batch = _EnsembleBatchSession(first._sess("_batch_session", _BatchSession))
        return self._ensemble_batch

    def _ensemble_many(self, models, states, mode, solo, forced=None, p_max=0.0, p_max_ub=0.0, lp=False):
        """`GCNN._many` for one ensemble: results per state -- ("ok", mean, order, n_kept[, cut_index], members), whatever `solo(i)`
        returned for a state the batched call declines, or an exception."""
        session = self.ensemble_batch_session(lp)

        def admit(i):
            if forced is not None and isinstance(forced[i], Exception):
                raise forced[i]
            if not lp:
                return GCNN._admit_state(states[i], mode)
            entry = session.base.check(states[i])
            n_cuts = entry[1]["n_cuts"]
            return None if n_cuts == 0 or (mode != _lib.IBATCH_SCORES and n_cuts > 4096) else entry

        def run(ids, checked):
            return session.run([checked[i] for i in ids], None if forced is None else [forced[i] for i in ids], mode, models, p_max,
                               p_max_ub)

        return _serve_many(len(states), admit, lambda ids: [ids[j:j + session.MAX] for j in range(0, len(ids), session.MAX)], run, solo)

    def _score_ensemble_many(self, keys, states, rank, return_exceptions, lp):
        keys = list(keys)
        models, states = self._ensemble_models(keys), list(states)
        mode = _lib.IBATCH_RANK if rank else _lib.IBATCH_SCORES
        one = self.score_lp_ensemble if lp else self.score_ensemble
        results = self._ensemble_many(models, states, mode, lambda i: one(keys, states[i], rank), lp=lp)
        for i, r in enumerate(results):
            if isinstance(r, tuple):
                scores = r[1]
                scores.members = r[-1]
                if lp:
                    scores.cut_index = r[4]
                if rank:
                    scores.rankings = r[2]
                results[i] = scores
        return GCNN._finish_many(results, return_exceptions)

    def _select_ensemble_many(self, keys, states, forced, p_max, p_max_ub, max_selected, return_exceptions, lp):
        keys = list(keys)
        models, states = self._ensemble_models(keys), list(states)
        ops.check_thresholds(p_max, p_max_ub)
        forced, packed = _packed_forced(states, forced, _snapshot_vars if lp else _state_vars, "snapshot" if lp else "state")
        one = self.select_cuts_lp_ensemble if lp else self.select_cuts_ensemble

        def solo(i):
            return one(keys, states[i], forced[i], p_max=p_max, p_max_ub=p_max_ub, max_selected=max_selected)

        results = self._ensemble_many(models, states, _lib.IBATCH_SELECT, solo, packed, p_max, p_max_ub, lp=lp)
        for i, r in enumerate(results):
            if isinstance(r, tuple):
                results[i] = SelectResult(r[2], r[3], n_selected(r[3], max_selected), r[1], r[4] if lp else None)
                results[i].members = r[-1]
        return GCNN._finish_many(results, return_exceptions)

    def score_ensemble_many(self, keys, states, rank=False, return_exceptions=False):
        """`score_ensemble` for many host states at once -- what waits at the scoring server of an evaluator farm
        (model_evaluator.py:157-241) that deploys the five seeds of a problem (model_trainer.py:38-49) as one ensemble.  `keys`: as
        `score_ensemble` takes them (1..8, each once, order kept; ValueError before any device work otherwise).  Up to 64 states
        per gcnn_infer_ensemble_batch call, more in several: one upload of the states as gcnn_infer_batch's union, one graph plan,
        the M forward passes over the union as one group, the mean, one download.  Returns a list of `ScoreArray` in the caller's
        order, each the mean over its state's cuts with `.members` (float32 [M, K_i]) and, with `rank`, `.rankings`.  For the
        states s_0..s_{S-1} one call admits, `.members[m]` of state i has the bits of `models[keys[m]].score_states([s_0..])[i]`;
        the mean and the ranking are `score_ensemble`'s definitions on them, so one state alone gives `score_ensemble`'s bits.
        Errors are per state as in `GCNN.score_states`.  States the call declines (no cuts, more than 4,096 cuts when ranking,
        device tensors, prepared `Batch`es) go through `score_ensemble` and come back in place."""
        return self._score_ensemble_many(keys, states, rank, return_exceptions, False)

    def select_cuts_ensemble_many(self, keys, states, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        """`select_cuts_ensemble` for many host states at once (gcnn_infer_ensemble_batch in selection mode).  `forced`: None, or one
        entry per state in the forms `select_cuts` accepts.  Returns a list of `SelectResult` whose `scores` are the mean, with
        `.members`; the selection of every state is `ops.select_cuts` over the union's mean with that state's forced rows."""
        return self._select_ensemble_many(keys, states, forced, p_max, p_max_ub, max_selected, return_exceptions, False)

    def score_lp_ensemble_many(self, keys, snapshots, rank=False, return_exceptions=False):
        """`score_ensemble_many` from `LPSnapshot`s (gcnn_lp_ensemble_batch: one upload of the packed snapshots, every state built
        once on the device; no variable limit).  Results are in STATE order and carry `.cut_index`; `.members[m]` has the bits of
        `models[keys[m]].score_lps(...)` on the snapshots one call admits.  A snapshot the device flags holds its own ValueError."""
        return self._score_ensemble_many(keys, snapshots, rank, return_exceptions, True)

    def select_cuts_lp_ensemble_many(self, keys, snapshots, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None,
                                     return_exceptions=False):
        """`select_cuts_ensemble_many` from `LPSnapshot`s; every `order` is in STATE order and the results carry `.cut_index`."""
        return self._select_ensemble_many(keys, snapshots, forced, p_max, p_max_ub, max_selected, return_exceptions, True)
