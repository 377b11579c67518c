"""Training-step counterpart of the reference's `model_trainer.py` for the HIP GCNN.

Mirrors (file:line in /root/reference):
  process(model, dataloader, fractions, loss_fn, optimizer)  model_trainer.py:239-316  -> process() (same positional order)
  pretrain(model, dataloader)                                 model_trainer.py:194-236  -> pretrain() (pretrain_many: a group)
  MeanSquaredError / Adam(learning_rate=lambda: lr)           model_trainer.py:131-132  -> mse_loss() / Adam
  ranking-prefix accuracy                                     model_trainer.py:280-302  -> ranking_fraction()
`train_step` is the fused fast path (no autograd graph): forward -> MSE head -> backward -> [RCCL all-reduce of ONE flat
gradient buffer] -> Keras-form Adam, all on the current HIP stream.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .graph import _ptr, _stream
from .model import GCNN, Batch, PRENORM_LAYERS, prenorm_count
from .store import StoreBatch


def mse_loss(scores: torch.Tensor, targets: torch.Tensor, scale: float | None = None, want_grad=True):
    """Keras `MeanSquaredError` on 1-D inputs (model_trainer.py:132,271).  Returns (loss[1], d_scores|None)."""
    n = scores.numel()
    scale = (1.0 / n if n else 0.0) if scale is None else scale
    loss = torch.empty(1, dtype=torch.float32, device=scores.device)
    d = torch.empty_like(scores, memory_format=torch.contiguous_format) if want_grad else None
    with torch.cuda.device(scores.device):
        _lib.check(_lib.lib().gcnn_mse_loss(_ptr(scores), _ptr(targets), n, scale, _ptr(loss), _ptr(d),
                                            _stream(scores.device)), "gcnn_mse_loss")
    return loss, d


class Adam:
    """Keras-2.7 Adam (model_trainer.py:131): lr_t = lr*sqrt(1-b2^t)/(1-b1^t); theta -= lr_t*m/(sqrt(v)+eps), eps=1e-7.
    One fused kernel over the model's flat parameter buffer.  `learning_rate` may be a float or a zero-arg callable
    (the reference passes `lambda: lr` so the plateau schedule can change it)."""

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon
        self.iterations = 0
        self.m = self.v = None
        self._dev = None   # device-resident {lr, b1, b2, eps, t, lr_t} for graph replay

    def _lr(self):
        return float(self.learning_rate() if callable(self.learning_rate) else self.learning_rate)

    def _moments(self, flat):
        if self.m is None:
            self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)

    def _tick(self):
        """Advance the step counter; returns this step's lr_t."""
        self.iterations += 1
        t = self.iterations
        return self._lr() * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def apply_flat(self, model: GCNN, flat_grad: torch.Tensor, grad_scale: torch.Tensor | None = None, divide=False):
        """grad_scale: optional device scalar multiplying (divide=False) or dividing (divide=True) every gradient."""
        flat = model.flat_parameters.detach()
        self._moments(flat)
        lr_t = self._tick()
        with torch.cuda.device(flat.device):
            _lib.check(_lib.lib().gcnn_adam_step(_ptr(flat), _ptr(flat_grad), _ptr(self.m), _ptr(self.v), flat.numel(),
                                                 lr_t, self.beta_1, self.beta_2, self.epsilon, _ptr(grad_scale),
                                                 int(divide), _stream(flat.device)), "gcnn_adam_step")

    def fused_args(self, model: GCNN):
        """Advance the step counter and return the `gcnn_adam_args` for `GCNN._backward_into(adam=...)`: the same update as
        `apply_flat`, executed by the backward pass's last launch instead of a launch of its own."""
        flat = model.flat_parameters.detach()
        self._moments(flat)
        return _lib.AdamArgs(flat.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self._tick(), self.beta_1, self.beta_2, self.epsilon)

    def apply_flat_dev(self, model: GCNN, flat_grad: torch.Tensor, grad_scale: torch.Tensor | None = None, divide=False):
        """The same update with hyper-parameters and step counter resident on the device (gcnn_adam_step_dev): nothing
        step-dependent crosses the host, so the call can sit inside a captured hipGraph and be replayed."""
        flat = model.flat_parameters.detach()
        self._moments(flat)
        if self._dev is None:
            self._dev = torch.tensor([self._lr(), self.beta_1, self.beta_2, self.epsilon, float(self.iterations), 0.0],
                                     dtype=torch.float32, device=flat.device)
        with torch.cuda.device(flat.device):
            _lib.check(_lib.lib().gcnn_adam_step_dev(_ptr(flat), _ptr(flat_grad), _ptr(self.m), _ptr(self.v), flat.numel(),
                                                     _ptr(self._dev), _ptr(grad_scale), int(divide), _stream(flat.device)),
                       "gcnn_adam_step_dev")

    def sync_from_device(self):
        """After graph replays: pull the step counter back; push the (possibly changed) learning rate."""
        if self._dev is not None:
            self.iterations = int(self._dev[4].item())
            self._dev[0] = self._lr()

    def apply_gradients(self, model: GCNN):
        """After `loss.backward()`: update from `model.flat_parameters.grad` (the reference's
        `optimizer.apply_gradients(zip(grads, model.trainable_variables))`, model_trainer.py:273)."""
        g = model.flat_parameters.grad
        if g is None:
            raise RuntimeError("no gradients: call loss.backward() first")
        self.apply_flat(model, g)


def _check_targets(y: torch.Tensor, n_cuts: int) -> torch.Tensor:
    """Targets as the kernels read them: contiguous fp32, one per cut."""
    if y.dtype != torch.float32 or not y.is_contiguous():
        y = y.to(torch.float32).contiguous()
    if y.numel() != n_cuts:
        raise ValueError(f"expected {n_cuts} targets, got {y.numel()}")
    return y


class TrainState:
    """Buffers reused across steps by `train_step` (flat gradient + the data-parallel count slot)."""

    def __init__(self, model: GCNN):
        n = model.flat_parameters.numel()
        # [gradients | local cut count | pad]: ONE buffer => ONE all-reduce per step
        self.buf = torch.zeros(n + 4, dtype=torch.float32, device=model.device)
        self.grads = self.buf[:n]
        self.count = self.buf[n:n + 1]


def train_step(model: GCNN, batch: Batch, targets: torch.Tensor, optimizer: Adam | None, state: TrainState,
               process_group=None, device_optimizer=False):
    """One training step on a prepared batch: forward + MSE + backward (+ all-reduce) (+ Adam).  Returns (loss, scores).

    Single GPU: loss = mean over this batch's cuts (model_trainer.py:271).  Data parallel (`process_group` given): each
    rank back-propagates the local SUM of squared errors; gradients and cut counts are summed with one RCCL all-reduce
    and Adam divides by the global cut count -- the mean over ALL cuts of the global batch, not a mean of per-rank means."""
    flat = model.flat_parameters.detach()
    ws = model._take_workspace(batch)
    n_cuts = batch.dims.n_cuts
    targets = _check_targets(targets, n_cuts)
    loss = torch.empty(1, dtype=torch.float32, device=model.device)
    # The MSE head rides in the forward's last launch (gcnn_forward_loss), so the backward starts at the readout's hidden layer
    if process_group is None:
        scores = model._forward_loss_into(flat, batch, ws, targets, 1.0 / max(n_cuts, 1))
        fuse = optimizer is not None and not device_optimizer   # host-parameterised Adam: rides in the backward's last launch
        model._backward_into(flat, batch, ws, None, state.grads, loss_out=loss, adam=optimizer.fused_args(model) if fuse else None)
        model._give_workspace(ws)
        if optimizer is not None and not fuse:
            optimizer.apply_flat_dev(model, state.grads)
        return loss, scores
    import torch.distributed as dist
    scores = model._forward_loss_into(flat, batch, ws, targets, 1.0)   # local SUM of squared errors
    model._backward_into(flat, batch, ws, None, state.grads, count_slot=state.count, loss_out=loss)  # also stores the local cut count
    model._give_workspace(ws)
    dist.all_reduce(state.buf, op=dist.ReduceOp.SUM, group=process_group)   # ONE collective: gradients + cut count
    if optimizer is not None:  # Adam divides by the global cut count: the mean over ALL cuts of the global batch
        (optimizer.apply_flat_dev if device_optimizer else optimizer.apply_flat)(model, state.grads, grad_scale=state.count,
                                                                              divide=True)
    return loss, scores


class GraphedTrainStep:
    """One training step on a FIXED prepared batch, captured once into a hipGraph and replayed.

    A step is 20 kernel launches on one stream; capture (torch.cuda.CUDAGraph over the same `train_step`) removes the host
    from the loop.  Everything step-dependent lives on the device (Adam's step counter and learning rate:
    `Adam.apply_flat_dev`).  Measured: no faster than eager issue -- the GPU-side launch sequence is the limit.
    The graph is tied to the batch's buffers and sizes: use it when batches have a fixed shape / are replayed (benchmarks,
    fixed-capacity loaders); variable-shape training uses the eager `train_step`."""

    def __init__(self, model: GCNN, batch: Batch, targets: torch.Tensor, optimizer: Adam | None, state: TrainState,
                 process_group=None, warmup=2):
        self.optimizer = optimizer
        args = (model, batch, targets, optimizer, state, process_group, True)
        cur = torch.cuda.current_stream(model.device)
        side = torch.cuda.Stream(device=model.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):           # eager warm-up: lazy HIP state (streams, events, attributes) and buffers
            for _ in range(warmup):
                train_step(*args)
        cur.wait_stream(side)
        torch.cuda.synchronize(model.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.scores = train_step(*args)
        self.steps = 0

    def __call__(self):
        self.graph.replay()
        self.steps += 1
        return self.loss, self.scores



# ---- groups: several independent models, one set of launches per step (gcnn_group_train_step / gcnn_group_forward) ----------
class _GroupTables:
    """Launch tables of group calls on one stream: a ring of pinned staging slots and one device buffer.  A call writes its tables
    into a slot and uploads them with one copy queued on the stream; the slot is written again only after an event recorded
    behind that call has passed, so group calls issued back to back without a host sync never overwrite a table still to be
    copied.  The device buffer needs no ring: the next call's upload is queued on the same stream, behind the previous call's
    launches (a call on another stream has tables of its own)."""
    SLOTS = 4

    def __init__(self, device):
        size = C.c_size_t()
        _lib.check(_lib.lib().gcnn_group_table_bytes(_lib.GROUP_MAX, C.byref(size)), "gcnn_group_table_bytes")
        self.bytes = size.value
        self.host = [torch.empty(self.bytes, dtype=torch.uint8).pin_memory() for _ in range(self.SLOTS)]
        self.events = [None] * self.SLOTS
        self.dev = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.pos = 0

    def call(self, fn, members, what, device):
        i = self.pos
        self.pos = (i + 1) % self.SLOTS
        if self.events[i] is not None:
            self.events[i].synchronize()
        arr = (_lib.GroupMember * len(members))(*members)
        with torch.cuda.device(device):
            _lib.check(fn(len(members), arr, C.c_void_p(self.host[i].data_ptr()), C.c_void_p(self.dev.data_ptr()), self.bytes,
                          _stream(device)), what)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
        self.events[i] = ev


_group_tables: dict = {}


def _tables(device) -> _GroupTables:
    key = (torch.device(device).index, torch.cuda.current_stream(device).cuda_stream)
    if key not in _group_tables:
        _group_tables[key] = _GroupTables(device)
    return _group_tables[key]


def _check_group(models, batches):
    if not 1 <= len(models) <= _lib.GROUP_MAX:
        raise ValueError(f"a group holds 1..{_lib.GROUP_MAX} models, got {len(models)}")
    if len(batches) != len(models):
        raise ValueError(f"{len(models)} models but {len(batches)} batches")
    if len({id(m) for m in models}) != len(models):
        raise ValueError("a model appears twice in the group")
    dev = models[0].device
    if any(m.device != dev for m in models):
        raise ValueError("the models of a group live on one device")
    return dev


def _group_member(model: GCNN, batch: Batch, ws: torch.Tensor, scores: torch.Tensor) -> _lib.GroupMember:
    g = _lib.GroupMember()
    g.dims = batch.dims
    g.params = model.flat_parameters.detach().data_ptr()
    g.cons_feats, g.var_feats, g.cut_feats = (_ptr(t).value for t in (batch.cons_feats, batch.var_feats, batch.cut_feats))
    g.cons_graph, g.cut_graph = batch.cons_graph.c, batch.cut_graph.c
    g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
    g.scores = _ptr(scores).value
    return g


def train_step_group(models, batches, targets, optimizers, states, process_group=None):
    """`train_step` for up to 8 independent models at once (gcnn_group_train_step): model i takes one step on batches[i] with
    targets[i], optimizers[i] (an `Adam`, or None: gradients only) and states[i] (its `TrainState`).  Same-shaped members share
    every launch: a group step issues as many launches as one solo step.  Each member's scores, loss, gradients, parameters
    and Adam moments are bit-identical to `train_step` on that member alone.  Returns [(loss, scores)] per member."""
    if process_group is not None:
        raise ValueError("train_step_group: data-parallel groups are not supported (process_group must be None)")
    dev = _check_group(models, batches)
    if not len(targets) == len(optimizers) == len(states) == len(models):
        raise ValueError("train_step_group: one target vector, optimizer and state per model")
    # every member is checked before any optimizer's step counter moves
    ys = [_check_targets(y, batch.dims.n_cuts) for batch, y in zip(batches, targets)]
    members, keep, out, taken, steps = [], [], [], [], []
    try:
        for model, batch, y, opt, state in zip(models, batches, ys, optimizers, states):
            n_cuts = batch.dims.n_cuts
            ws = model._take_workspace(batch)
            taken.append((model, ws))
            scores = torch.empty(n_cuts, dtype=torch.float32, device=dev)
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            g = _group_member(model, batch, ws, scores)
            g.targets, g.loss_scale = _ptr(y).value, 1.0 / max(n_cuts, 1)
            g.grads, g.loss_out = state.grads.data_ptr(), loss.data_ptr()
            if opt is not None:
                adam = opt.fused_args(model)
                steps.append(opt)
                keep.append(adam)
                g.adam = C.pointer(adam)
            members.append(g)
            keep.append(y)
            out.append((loss, scores))
        _tables(dev).call(_lib.lib().gcnn_group_train_step, members, "gcnn_group_train_step", dev)
    except BaseException:
        for opt in steps:   # refused: no step was taken
            opt.iterations -= 1
        raise
    finally:
        for model, ws in taken:
            model._give_workspace(ws)
    return out


def forward_group(models, batches, out=None):
    """Scores of every model on its batch (gcnn_group_forward): what `model(batch)` returns, bit for bit, for up to 8 models in
    one set of launches.  Nothing is kept for a backward pass.  The batches may be the same object (validation).
    `out`: optional list of contiguous 1-D fp32 device tensors, one per model with one element per cut of its batch, that the
    scores are written into (e.g. rows of one buffer); they must not overlap (the call refuses it).  Returns the score tensors."""
    dev = _check_group(models, batches)
    if out is not None and len(out) != len(models):
        raise ValueError(f"{len(models)} models but {len(out)} output tensors")
    members, result, taken, prepared = [], [], [], []
    try:
        for i, (model, batch) in enumerate(zip(models, batches)):
            if not isinstance(batch, Batch):
                batch = model.prepare(batch)
            prepared.append(batch)   # alive until the call has enqueued its reads: the allocator would hand its memory on
            if out is None:
                scores = torch.empty(batch.dims.n_cuts, dtype=torch.float32, device=dev)
            else:
                scores = out[i]
                if (scores.dtype != torch.float32 or scores.dim() != 1 or not scores.is_contiguous() or scores.device != dev
                        or scores.numel() != batch.dims.n_cuts):
                    raise ValueError(f"out[{i}] must be a contiguous 1-D float32 tensor of {batch.dims.n_cuts} elements on {dev}")
            ws = model._take_workspace(batch)
            taken.append((model, ws))
            members.append(_group_member(model, batch, ws, scores))
            result.append(scores)
        _tables(dev).call(_lib.lib().gcnn_group_forward, members, "gcnn_group_forward", dev)
    finally:
        for model, ws in taken:
            model._give_workspace(ws)
    return result


def ranking_fraction(pred: np.ndarray, true: np.ndarray) -> float:
    """model_trainer.py:288-301: length of the ranking prefix on which prediction and truth agree, over #cuts.
    Python's `sorted(..., reverse=True)` is stable, i.e. ties keep index order: a stable argsort of the negated key.
    The device metric's rule (k_ranking) holds here too, so that a sample is credited the same whichever path its batch takes:
    NaN ranks as -inf, and a sample without cuts has fraction 0."""
    def order(key):
        key = np.array(key, dtype=np.float64)
        key[np.isnan(key)] = -np.inf
        return np.argsort(-key, kind="stable")

    pr, tr = order(pred), order(true)
    if len(pr) == 0:
        return 0.0
    diff = pr != tr
    return (int(np.argmax(diff)) if diff.any() else len(pr)) / len(pr)


def ranking_metric(pred: torch.Tensor, true: torch.Tensor, n_cuts, fractions_dev: torch.Tensor, acc: torch.Tensor,
                   loss: torch.Tensor | None = None, loss_acc: torch.Tensor | None = None, loss_weight: float | None = None):
    """Device-side ranking-prefix accuracy (gcnn_ranking_metric): acc[f] += #samples with frac >= fractions[f]; optionally
    loss_acc += loss * loss_weight (default: total_cuts, the cut-weighted loss of model_trainer.py:304).  Returns per-sample
    fractions (device)."""
    n_cuts = np.asarray(n_cuts, dtype=np.int64).reshape(-1)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(n_cuts)]).astype(np.int32)).to(pred.device, non_blocking=True)
    frac = torch.empty(len(n_cuts), dtype=torch.float32, device=pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().gcnn_ranking_metric(_ptr(pred), _ptr(true), _ptr(offsets), len(n_cuts),
                                                  int(n_cuts.max()) if len(n_cuts) else 0, _ptr(fractions_dev),
                                                  fractions_dev.numel(), _ptr(acc), _ptr(frac), _ptr(loss),
                                                  float(n_cuts.sum()) if loss_weight is None else float(loss_weight), _ptr(loss_acc),
                                                  _stream(pred.device)),
                   "gcnn_ranking_metric")
    return frac


class _EpochTotals:
    """One model's loss and ranking accuracy over an epoch.  They accumulate ON THE DEVICE and the host reads them once, in
    `result`; only a batch with a sample too large for the device metric (more than 4,096 cuts) is ranked on the host."""

    def __init__(self, fractions: np.ndarray, device):
        self.fractions, self.device = fractions, device
        self.frac_dev = torch.from_numpy(fractions).to(device)
        self.acc = torch.zeros(len(fractions), dtype=torch.float32, device=device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=device)
        self.host_acc, self.host_loss = np.zeros(len(fractions)), 0.0
        self.n_samples = self.cut_count = 0

    def add(self, pred: torch.Tensor, y: torch.Tensor, n_cuts: np.ndarray, loss: torch.Tensor, weight: float):
        """One batch: predictions and targets of its cuts, per-sample cut counts, its loss and the weight the loss enters with."""
        if len(n_cuts) == 0:
            pass
        elif n_cuts.max() <= 4096:
            ranking_metric(pred, y, n_cuts, self.frac_dev, self.acc, loss, self.loss, weight)
        else:
            p, t = pred.cpu().numpy(), y.cpu().numpy()
            start = 0
            for nk in n_cuts:
                self.host_acc += ranking_fraction(p[start:start + nk], t[start:start + nk]) >= self.fractions
                start += nk
            self.host_loss += float(loss) * weight
        self.n_samples += len(n_cuts)
        self.cut_count += int(n_cuts.sum())

    def result(self, process_group=None):
        """(cut-weighted mean loss, accuracy per fraction), over all ranks of `process_group` when one is given."""
        dev = self.device
        totals = torch.cat([self.loss.double() + self.host_loss, self.acc.double() + torch.from_numpy(self.host_acc).to(dev),
                            torch.tensor([float(self.n_samples), float(self.cut_count)], dtype=torch.float64, device=dev)])
        if process_group is not None:
            import torch.distributed as dist
            dist.all_reduce(totals, op=dist.ReduceOp.SUM, group=process_group)
        totals = totals.cpu().numpy()
        return float(totals[0]) / max(totals[-1], 1.0), totals[1:-2] / max(totals[-2], 1.0)


def _model_inputs(item):
    """A loader item -- `utils.load_batch` 11-tuple or `SampleStore` batch -- as the model takes it: the prepared `Batch`, or the
    10-tuple with the per-sample counts summed."""
    if isinstance(item, StoreBatch):     # collated on the device by a SampleStore: nothing left to move
        return item.batch
    return tuple(item[:7]) + (int(np.sum(item[7])), int(np.sum(item[8])), int(np.sum(item[9])))


def _unpack_batch(model: GCNN, batch):
    """A loader item -> (prepared Batch, per-sample n_cuts, device targets)."""
    prepared = model.prepare(_model_inputs(batch))
    if isinstance(batch, StoreBatch):
        return prepared, np.asarray(batch.n_cuts).reshape(-1), batch.improvements
    y = torch.as_tensor(np.asarray(batch[10]), dtype=torch.float32).to(model.device, non_blocking=True)
    return prepared, np.asarray(batch[9]).reshape(-1), y


def process(model: GCNN, dataloader, fractions: np.ndarray, loss_fn=None, optimizer: Adam | None = None, *,
            process_group=None):
    """Counterpart of model_trainer.process (model_trainer.py:239-316), same positional order:
    `process(model, dataloader, fractions, loss_fn, optimizer=None)`.  `loss_fn` keeps the reference's slot so its call sites
    (model_trainer.py:156,161,182) bind unchanged; the loss is always the reference's `MeanSquaredError`
    (model_trainer.py:132) evaluated by the fused loss head, so a callable (or None) is accepted and not called.
    `dataloader` yields the 11-tuples of `utils.load_batch` (per-sample count vectors + improvements) or `SampleStore`
    batches.  Returns (cut-weighted mean loss, accuracy per fraction).  Loss and ranking accuracy accumulate ON THE DEVICE;
    the host reads them once at the end (no per-batch sync).

    Data parallel (`process_group` given, keyword only): every rank iterates over ITS shard of each global batch (e.g.
    `store.batches(ids, batch_size, rank, world_size)`, the same number of batches on every rank, empty shards included);
    gradients are all-reduced per step (`train_step`) and the returned loss / accuracies are those of the GLOBAL data."""
    if isinstance(loss_fn, Adam):
        raise TypeError("process(model, dataloader, fractions, loss_fn, optimizer): the fourth positional argument is the "
                        "reference's loss_fn slot; pass the optimizer fifth (or optimizer=...)")
    if loss_fn is not None and not callable(loss_fn):
        raise TypeError("loss_fn must be None or a callable (it is accepted for call compatibility and not called)")
    totals = _EpochTotals(np.asarray(fractions, dtype=np.float32), model.device)
    state = TrainState(model) if optimizer is not None else None
    for batch in dataloader:
        try:
            prepared, n_cuts, y = _unpack_batch(model, batch)
            total = int(n_cuts.sum())
            if optimizer is not None:
                # data parallel: `loss` is the local SUM of squared errors (train_step), else the mean over this batch
                loss, predictions = train_step(model, prepared, y, optimizer, state, process_group=process_group)
                weight = 1.0 if process_group is not None else float(total)
            else:
                with torch.no_grad():
                    predictions = model(prepared, False)
                loss, _ = mse_loss(predictions, y, want_grad=False)
                weight = float(total)
            totals.add(predictions.detach().as_subclass(torch.Tensor), y, n_cuts, loss, weight)
        except torch.OutOfMemoryError:  # the reference skips batches that exhaust memory (model_trainer.py:308-311)
            if process_group is not None:
                # Data parallel: the peers are in (or heading for) this step's all-reduce; a rank that skipped on its own
                # would pair that collective with its next batch.  Agreeing on a skip costs a blocking collective per batch,
                # so the error propagates instead (with the store resident in HBM a batch that does not fit is a sizing bug).
                raise
            print("WARNING: batch skipped.")
    return totals.result(process_group)


def pretrain(model: GCNN, dataloader, process_group=None):
    """Counterpart of model_trainer.pretrain (model_trainer.py:194-236): fit PreNorm layers one at a time.  `dataloader` is
    iterated once per layer (a list, or any re-iterable).  Data parallel (`process_group` given): every rank passes ITS shard of
    the pretraining batches (possibly none); after each pass the ranks merge their streaming statistics with one small
    all-gather (`GCNN.pretrain_sync`), so all ranks freeze identical shift / scale values -- 11 passes over 1/N of the data
    each instead of every rank redoing all of it."""
    model.pretrain_init()
    i = 0
    while True:
        for batch in dataloader:
            try:
                if not model.pretrain(_model_inputs(batch), True):
                    break
            except torch.OutOfMemoryError:
                print("WARNING: batch skipped.")
        model.pretrain_sync(process_group)
        if model.pretrain_next() is None:
            break
        i += 1
    return i


def pretrain_many(models, loaders, process_group=None):
    """`pretrain` for up to 8 models in lockstep (gcnn_group_prenorm_merge): model i fits its PreNorm layers on loaders[i]
    (re-iterable, yielding `SampleStore` batches or `load_batch` 11-tuples), one layer per pass, and each step of a pass sends
    the models' batches out as one group call.  The streaming merge of the statistics runs on the device, into a small state
    per model that the host reads once, at the end of the pass: store batches need no host read in between (tuples still go
    through `prepare`, which checks them on the host).  A model whose loader ends waits for the others.  Returns one
    fitted-layer count per model; model i's parameters, PreNorm state and count are those of `pretrain(models[i], loaders[i])`."""
    if process_group is not None:
        raise ValueError("pretrain_many: data-parallel groups are not supported (process_group must be None)")
    n = len(models)
    if len(loaders) != n:
        raise ValueError(f"pretrain_many: {n} models but {len(loaders)} loaders")
    dev = _check_group(models, loaders)
    lib = _lib.lib()
    words = _lib.PRENORM_STATE_BYTES // 4
    mean0, var0 = _lib.PRENORM_STATE_MEAN // 4, _lib.PRENORM_STATE_VAR // 4
    states = torch.empty((n, words), dtype=torch.float32, device=dev)
    for m in models:
        m.pretrain_init()
    fitted = [0] * n
    live = list(range(n))
    while True:
        layer = {}   # the layer each model fits in this pass: its first waiting one (none left: that model is done)
        for i in live:
            waiting = models[i]._waiting_layer()
            if waiting is not None:
                layer[i] = waiting
        live = [i for i in live if i in layer]
        if not live:
            break
        states.zero_()
        received = dict.fromkeys(live, False)
        iters = {i: iter(loaders[i]) for i in live}
        going = list(live)
        while going:
            step = []
            for i in list(going):
                try:
                    step.append((i, next(iters[i])))
                except StopIteration:
                    going.remove(i)
            members, idx, taken, prepared = [], [], [], []
            try:
                for i, b in step:
                    m = models[i]
                    try:
                        batch = m.prepare(_model_inputs(b))
                        received[i] = True
                        if prenorm_count(batch.dims, layer[i]) == 0:
                            continue
                        ws = m._take_workspace(batch)
                    except torch.OutOfMemoryError:   # as `pretrain`: the batch is skipped
                        print("WARNING: batch skipped.")
                        continue
                    taken.append((m, ws))
                    prepared.append(batch)   # alive until the call has enqueued its reads
                    members.append(_group_member(m, batch, ws, None))
                    idx.append(i)
                if members:
                    layers = (C.c_int32 * len(idx))(*[layer[i] for i in idx])
                    ptrs = (C.c_void_p * len(idx))(*[states[i].data_ptr() for i in idx])
                    _tables(dev).call(lambda k, arr, host, table, nbytes, stream: lib.gcnn_group_prenorm_merge(
                        k, arr, layers, ptrs, host, table, nbytes, stream), members, "gcnn_group_prenorm_merge", dev)
            finally:
                for m, ws in taken:
                    m._give_workspace(ws)
        host = states.cpu().numpy()   # the pass's one read
        for i in live:
            units = PRENORM_LAYERS[layer[i]][2]
            st = models[i]._prenorm_state[layer[i]]
            st["count"] = np.float32(host[i, 0])
            st["mean"], st["var"] = host[i, mean0:mean0 + units].copy(), host[i, var0:var0 + units].copy()
            st["received"] = received[i]
            if models[i].pretrain_next() is None:
                layer.pop(i)
            else:
                fitted[i] += 1
        live = [i for i in live if i in layer]
    return fitted


def process_many(models, loaders, fractions: np.ndarray, optimizers=None):
    """`process` for a group of models in lockstep: model i iterates loaders[i] (training with optimizers[i] when optimizers is
    given, else validation), and the models' steps go out as group calls (`train_step_group`, `forward_group`).  A model whose
    loader ends leaves the group.  Returns [(loss, accuracies)] per model, each what `process(models[i], loaders[i], fractions,
    None, optimizers[i])` returns for that model alone."""
    n = len(models)
    if len(loaders) != n or (optimizers is not None and len(optimizers) != n):
        raise ValueError("process_many: one loader (and optimizer) per model")
    if not 1 <= n <= _lib.GROUP_MAX or len({id(m) for m in models}) != n:
        raise ValueError(f"process_many: 1..{_lib.GROUP_MAX} distinct models")
    fractions = np.asarray(fractions, dtype=np.float32)
    totals = [_EpochTotals(fractions, models[0].device) for _ in models]
    states = [TrainState(m) for m in models] if optimizers is not None else None
    iters = [iter(ld) for ld in loaders]
    live = list(range(n))
    while live:
        step = []
        for i in list(live):
            try:
                step.append((i, next(iters[i])))
            except StopIteration:
                live.remove(i)
        if not step:
            break
        idx = [i for i, _ in step]
        unpacked = [_unpack_batch(models[i], b) for i, b in step]
        if optimizers is not None:
            out = train_step_group([models[i] for i in idx], [u[0] for u in unpacked], [u[2] for u in unpacked],
                                   [optimizers[i] for i in idx], [states[i] for i in idx])
            losses, preds = [o[0] for o in out], [o[1] for o in out]
        else:
            preds = forward_group([models[i] for i in idx], [u[0] for u in unpacked])
            losses = [mse_loss(p, u[2], want_grad=False)[0] for p, u in zip(preds, unpacked)]
        for i, (_, n_cuts, y), loss, pred in zip(idx, unpacked, losses, preds):
            totals[i].add(pred, y, n_cuts, loss, float(n_cuts.sum()))
    return [t.result() for t in totals]


class _StoreBatches:
    """Re-iterable `store.batches(ids, batch_size)` (pretraining walks its batches once per PreNorm layer)."""

    def __init__(self, store, ids, batch_size):
        self.store, self.ids, self.batch_size = store, ids, batch_size

    def __iter__(self):
        return self.store.batches(self.ids, self.batch_size)


def train_models(models, seeds, train_stores, valid_stores, best_paths, fractions=(0.25, 0.5, 0.75, 1.0), max_epochs=1000,
                 epoch_size=2500, batch_size=4, pretrain_batch_size=2, valid_batch_size=4, lr=0.0001, patience=10,
                 early_stopping=20):
    """The reference's `train_model` (model_trainer.py:52-185) for up to 8 models at once, e.g. the five seeds of a problem.
    Model i trains on `train_stores[i]` and validates on `valid_stores[i]` (`SampleStore`s; the same store may serve several
    models), with its own `np.random.default_rng(seeds[i])`, learning rate, plateau counter and best checkpoint
    (`best_paths[i]`, written by `save_state`).  Epoch 0 pretrains the models together (`pretrain_many`) and validates; every later epoch draws
    `epoch_size * batch_size` training samples with replacement, trains and validates the models still running in lockstep
    groups.  A model leaves the group at its early stop.  At the end every model is restored to its best state and validated.
    A model's history and best parameters are those of a run with that model alone.  Returns one history dict per model."""
    n = len(models)
    if not (len(seeds) == len(train_stores) == len(valid_stores) == len(best_paths) == n):
        raise ValueError("train_models: one seed, training store, validation store and checkpoint path per model")
    fractions = np.asarray(fractions, dtype=np.float32)
    rngs = [np.random.default_rng(s) for s in seeds]
    for rng in rngs:   # model_trainer.py:104-105: the first draw seeds TensorFlow; consumed so that the epoch draws match
        rng.integers(np.iinfo(int).max)
    lrs = list(map(float, [lr] * n))
    opts = [Adam(learning_rate=(lambda i=i: lrs[i])) for i in range(n)]
    valid = [_StoreBatches(v, np.arange(len(v)), valid_batch_size) for v in valid_stores]
    hist = [dict(train_loss=[], train_acc=[], valid_loss=[], valid_acc=[], lr_changes=[], best_epoch=None,
                 stopped_epoch=None, pretrained_layers=None) for _ in range(n)]
    best, plateau = [np.inf] * n, [0] * n
    live = list(range(n))
    for epoch in range(max_epochs + 1):
        if not live:
            break
        if epoch == 0:
            loaders = []
            for i in live:
                ids = np.arange(len(train_stores[i]))
                loaders.append(_StoreBatches(train_stores[i], ids[ids % 10 == 0], pretrain_batch_size))
            for i, k in zip(live, pretrain_many([models[i] for i in live], loaders)):
                hist[i]["pretrained_layers"] = k
        else:
            loaders = [train_stores[i].batches(rngs[i].choice(len(train_stores[i]), epoch_size * batch_size, replace=True),
                                               batch_size) for i in live]
            for i, (loss, acc) in zip(live, process_many([models[i] for i in live], loaders, fractions,
                                                         [opts[i] for i in live])):
                hist[i]["train_loss"].append(loss)
                hist[i]["train_acc"].append(acc)
        results = process_many([models[i] for i in live], [valid[i] for i in live], fractions)
        for i, (loss, acc) in zip(list(live), results):
            hist[i]["valid_loss"].append(loss)
            hist[i]["valid_acc"].append(acc)
            if loss < best[i]:
                plateau[i], best[i] = 0, loss
                models[i].save_state(best_paths[i])
                hist[i]["best_epoch"] = epoch
            else:
                plateau[i] += 1
                if plateau[i] % early_stopping == 0:
                    hist[i]["stopped_epoch"] = epoch
                    live.remove(i)
                elif plateau[i] % patience == 0:
                    lrs[i] *= 0.2
                    hist[i]["lr_changes"].append((epoch, lrs[i]))
    for i in range(n):
        models[i].restore_state(best_paths[i])
    for i, (loss, acc) in enumerate(process_many(models, valid, fractions)):
        hist[i]["best_valid_loss"], hist[i]["best_valid_acc"] = loss, acc
    return hist
