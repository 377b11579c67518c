"""A scoring server: any number of CPU-only worker processes (the evaluators' task farms, model_evaluator.py:157-241: SCIP in every
worker, one selector call per separation round) share ONE process that owns the GPU.

    server = ScoringServer({"setcov": model}, "/tmp/gcnn.sock"); server.start()          # the GPU process
    client = ScoringClient("/tmp/gcnn.sock", "setcov")                                    # a worker: NumPy only, no torch
    CustomCutsel(function=client.get_concrete_function(), ...)                            # model_evaluator.py:310-314
    client.select_cuts_lp(lpstate.LPSnapshot(...), max_selected=10)                       # or: the raw LP, get_state left to the GPU

The server takes every request that is waiting and groups them by kind.  The host-state requests of ALL models share one
`ModelSet.score_states` / `ModelSet.select_cuts_many` call: the farm's queue runs `seed` innermost (model_evaluator.py:211-219), so
the workers that wait hold different models -- one upload, the models' forward passes as a group, one download.  A group that
holds one model's requests takes that model's own call.  The LP requests of all models share one `ModelSet.score_lps` /
`ModelSet.select_cuts_lp_many` call, which also builds the states on the device (`cross_model_lp`).  With `cross_model=False` the
server groups by model and kind and answers each group with one `GCNN.score_states` / `GCNN.select_cuts_many` call (one forward
pass over the disjoint union of the group's states), for the LP kinds one `GCNN.score_lps` / `GCNN.select_cuts_lp_many` call.
Then it goes back for whatever queued up meanwhile; it never waits for a batch to fill: a lone request is served at once.  Hybrid
requests (SCIP's hybrid quality from the cut rows, `client.select_cuts_hybrid`) need no model: those that are waiting are grouped
by thresholds and answered with one `HybridSelector.select_cuts_many`.  The data collector's expert rounds (`client.collect_lp`:
the sample's state and the selection over the expert's quality, `collect.Collector`) need no model either; each is answered alone.

What the codec and the server's reader know about a request kind stands in its row of `_KINDS`.  A new kind is a number, a row, an
`encode_*_request` over `_message` and, unless it answers with one of the two shapes there are (`_scores_reply`, `_selection_reply`
and their readers), a function that makes its reply; the server answers it through `_answer_group`.

Wire format (AF_UNIX stream; little-endian; no pickle -- nothing a peer sends is ever executed): a message is a uint32 byte count
followed by that many bytes: a fixed header, the model key, then arrays, each a 24-byte descriptor (dtype code, ndim, two
dimensions, byte count) followed by its raw buffer.  This module imports no torch: workers stay light."""

from __future__ import annotations

import os
import selectors
import socket
import struct
import threading
from functools import partial

import numpy as np

from . import lpstate      # NumPy only

MAGIC = b"GCS1"
KIND_SCORE, KIND_RANK, KIND_SELECT = 0, 1, 2
# the same three from a raw LP snapshot (lpstate.LPSnapshot): its 21 arrays (19 without an incumbent), one float64 array of the
# scalars (infinity, sum_epsilon, n_model_vars, obj_norm), then the optional forced pair; the header's n_cons slot says whether
# there is an incumbent.  Replies carry cut_index as one more array.
KIND_LP_SCORE, KIND_LP_RANK, KIND_LP_SELECT = 3, 4, 5
_LP_BASE = {KIND_LP_SCORE: KIND_SCORE, KIND_LP_RANK: KIND_RANK, KIND_LP_SELECT: KIND_SELECT}
_ENSEMBLE_KINDS = (KIND_SCORE, KIND_RANK, KIND_SELECT, KIND_LP_SCORE, KIND_LP_RANK, KIND_LP_SELECT)   # what an ensemble's name may ask for
# SCIP's hybrid selection from the cut rows alone (hybrid.HybridSelector; no model: the model key is ignored): the eight arrays of a
# lpstate.CutSnapshot, one float64 array with `infinity`, then the optional forced pair.  Replies carry the float64 quality, order,
# cut_index (the identity) and the features [K, 3].
KIND_HYBRID_SELECT = 6
_HYBRID_ARRAYS = len(lpstate.CUT_FIELDS) + 1
# An LP resident on the server's device across a worker's separation rounds (`ScoringClient.open_lp` -> `RemoteLPSession`; the
# server holds an `infer.LPSession` per id and serves the rounds that wait together through one `infer.LPSessionGroup` call per 8):
#   open   the seven arrays of a `lpstate.LPRows` and one float64 array of its scalars; the n_cons slot says whether the server
#          checks the O(nnz) facts on the host too.  The reply's n_kept slot carries the session id.
#   round  n_cons: the session id; n_vars: mode | presence mask of the four optional arrays << 8 | has a block << 12 |
#          has_incumbent (0 None, 1 False, 2 True) << 13 | incremental << 15.  Arrays: the round's in `lpstate.ROUND_FIELDS` order
#          without the absent optional ones, then the five arrays of an `LPRowBlock`, then the forced pair.  n_cuts (the
#          header's last word, 0 in every other session request): 1 when the round removes rows; it then carries one more array,
#          the removed rows' indices (int32, one dimension, numbered after the block's append), behind the block's arrays and in
#          front of the forced pair.  Mode SESSION_APPEND is an edit alone: a block (`append_rows`), a list (`remove_rows`) or
#          both, but at least one.  The reply is that of the KIND_LP_* kinds, cut_index included.
#   close  n_cons: the session id.
KIND_LP_OPEN, KIND_LP_ROUND, KIND_LP_CLOSE = 7, 8, 9
SESSION_SCORE, SESSION_RANK, SESSION_SELECT, SESSION_APPEND = 0, 1, 2, 3
_SESSION_KINDS = (KIND_LP_OPEN, KIND_LP_ROUND, KIND_LP_CLOSE)
_ROUND_BASE = len(lpstate.ROUND_FIELDS) - len(lpstate.OPTIONAL)
_PRIMAL = (14, 15)         # positions of col_primal / col_primal_avg among lpstate.FIELDS
# An expert round of the data collector (collect.Collector.collect_lp; no model: the model key is ignored): KIND_LP_SELECT's arrays,
# then one float64 array [K] with the expert's quality in input cut order, in front of the optional forced pair.  The reply carries
# the seven state arrays, cut_index, improvements, order, the hybrid quality and the features; n_kept and n_selected in its header.
# Kind 10 stays unknown.  There is no session mode: a collector has no use for a resident LP.
KIND_COLLECT = 11
MAX_MESSAGE = 1 << 30
# request: magic, kind, n_arrays, key length, p_max, p_max_ub, max_selected (-1: none), n_forced (-1: no forced rows), n_cons, n_vars, n_cuts
_REQ = struct.Struct("<4sBBHddiiiii")
# reply: magic, status (0 ok, else an error class), n_arrays, pad, n_kept, n_selected
_REP = struct.Struct("<4sBBHii")
_ARR = struct.Struct("<BBHIIQ4x")      # dtype code, ndim, pad, dim0, dim1, bytes
_DTYPES = ("<f4", "<f8", "<i4", "<i8", "|u1", "|i1")
_CODES = {np.dtype(d): i for i, d in enumerate(_DTYPES)}
ERR_VALUE, ERR_GCNN, ERR_OTHER = 1, 2, 3


class ServerError(RuntimeError):
    """The server answered a request with an error that is not a ValueError of the request's own data."""


class ProtocolError(ValueError):
    pass


def _wire_array(a):
    a = np.asarray(a)
    if a.dtype not in _CODES:
        if a.dtype.kind in "iub":
            a = a.astype(np.int64)
        elif a.dtype.kind == "f":
            a = a.astype(np.float64)
        else:
            raise ValueError(f"cannot send an array of dtype {a.dtype}")
    if a.ndim > 2:
        raise ValueError(f"cannot send an array of {a.ndim} dimensions")
    return np.ascontiguousarray(a)


def _put_arrays(parts, arrays):
    for a in arrays:
        a = _wire_array(a)
        shape = tuple(a.shape) + (0,) * (2 - a.ndim)
        parts.append(_ARR.pack(_CODES[a.dtype], a.ndim, 0, shape[0], shape[1], a.nbytes))
        parts.append(a.tobytes())


def _get_arrays(buf, at, count):
    out = []
    for _ in range(count):
        if at + _ARR.size > len(buf):
            raise ProtocolError("truncated array descriptor")
        code, ndim, _, d0, d1, nbytes = _ARR.unpack_from(buf, at)
        at += _ARR.size
        if code >= len(_DTYPES) or ndim > 2:
            raise ProtocolError("unknown dtype code or rank")
        dt = np.dtype(_DTYPES[code])
        shape = (d0, d1)[:ndim]
        if int(np.prod(shape, dtype=np.int64)) * dt.itemsize != nbytes or at + nbytes > len(buf):
            raise ProtocolError("array size does not match its descriptor")
        out.append(np.frombuffer(buf, dt, int(nbytes // dt.itemsize), at).reshape(shape).copy())
        at += nbytes
    return out, at


def encode_request(model_key, kind, state, forced=None, p_max=0.1, p_max_ub=0.5, max_selected=None):
    """-> the message's bytes (without the length prefix).  `state`: the model's 10-tuple of host arrays (an LP snapshot goes
    through `encode_lp_request`); `forced`: None or (edge_inds [2,E], values [E][, n_forced]) as `GCNN.select_cuts` takes it."""
    if len(state) != 10:
        raise ValueError(f"expected the 10-tuple state, got {len(state)} items")
    return _message(kind, model_key, state[:7], forced, p_max, p_max_ub, max_selected, *state[7:])


def _message(kind, model_key, arrays=(), forced=None, p_max=0.0, p_max_ub=0.0, max_selected=None, a=0, b=0, c=0):
    """Every request's bytes: the header with the kind's three words `a, b, c`, the key, the kind's arrays and, behind them, the
    forced rows as `GCNN.select_cuts` takes them (the header then says how many)."""
    n_forced = -1
    if forced is not None:
        fi = np.asarray(forced[0])
        n_forced = int(forced[2]) if len(forced) > 2 else (int(fi[0].max()) + 1 if fi.size else 0)
        arrays = list(arrays) + [fi, np.asarray(forced[1])]
    key = model_key.encode("utf-8")
    parts = [_REQ.pack(MAGIC, kind, len(arrays), len(key), float(p_max), float(p_max_ub), -1 if max_selected is None else int(max_selected),
                       n_forced, int(a), int(b), int(c)), key]
    _put_arrays(parts, arrays)
    return b"".join(parts)


def _scalars(dims):
    return np.array([dims["infinity"], dims["sum_epsilon"], dims["n_model_vars"], dims["obj_norm"]], np.float64)


def _take_scalars(a, what):          # the four scalars behind a snapshot's or an open's arrays -> keywords of `LPSnapshot` / `LPRows`
    if a.dtype != np.float64 or a.shape != (4,) or not np.isfinite(a[2]):
        raise ProtocolError(f"malformed {what} scalars")
    return dict(infinity=float(a[0]), sum_epsilon=float(a[1]), n_model_vars=int(a[2]), obj_norm=float(a[3]))


# the LP payload: the snapshot's arrays in lpstate.FIELDS order, without the primal pair when there is no incumbent, then the scalars
_LP_FIELDS = {inc: [(i, n) for i, (n, _) in enumerate(lpstate.FIELDS) if inc or i not in _PRIMAL] for inc in (0, 1)}


def _lp_payload(snapshot):
    """-> (the arrays an LP message carries, dims); the snapshot is checked as the server will check it, so it raises in the worker."""
    arrays, dims = lpstate.check_snapshot(snapshot, deep=False)
    return [arrays[i] for i, _ in _LP_FIELDS[dims["has_incumbent"]]] + [_scalars(dims)], dims


def _lp_snapshot(inc, arrays):       # the inverse of `_lp_payload`; the arrays behind the payload are not looked at
    fields = _LP_FIELDS[inc]
    return lpstate.LPSnapshot(**{n: a for (_, n), a in zip(fields, arrays)}, **_take_scalars(arrays[len(fields)], "snapshot"),
                              has_incumbent=bool(inc))


def encode_lp_request(model_key, kind, snapshot, forced=None, p_max=0.1, p_max_ub=0.5, max_selected=None):
    """-> the message's bytes of an LP request (kind KIND_LP_*); a snapshot `lpstate.check_snapshot` refuses raises here."""
    arrays, dims = _lp_payload(snapshot)
    return _message(kind, model_key, arrays, forced, p_max, p_max_ub, max_selected, dims["has_incumbent"])


def encode_hybrid_request(model_key, snapshot, forced=None, p_max=0.1, p_max_ub=0.5, max_selected=None):
    """-> the message's bytes of a hybrid selection request.  `snapshot`: a `lpstate.CutSnapshot` or `LPSnapshot`, checked here as
    the server will check it again (without the O(nnz) facts), so its ValueError is raised in the worker."""
    arrays, dims = lpstate.check_cut_snapshot(snapshot, deep=False)
    return _message(KIND_HYBRID_SELECT, model_key, list(arrays) + [np.array([dims["infinity"]], np.float64)], forced, p_max, p_max_ub,
                    max_selected)


def encode_collect_request(model_key, snapshot, quality, forced=None, p_max=0.1, p_max_ub=0.5, max_selected=None):
    """-> the message's bytes of an expert round.  The snapshot and the quality are checked here as the server will check them
    again (`lpstate.check_snapshot` without the O(nnz) facts, `lpstate.check_quality`), so their ValueError is raised in the worker."""
    arrays, dims = _lp_payload(snapshot)
    arrays.append(lpstate.check_quality(quality, dims["n_cuts"]))
    return _message(KIND_COLLECT, model_key, arrays, forced, p_max, p_max_ub, max_selected, dims["has_incumbent"])


def encode_open_request(model_key, rows, deep=True):
    """-> the message's bytes of an open request.  `rows`: a `lpstate.LPRows`, checked here as the server will check it again
    (without the O(nnz) facts), so its ValueError is raised in the worker."""
    arrays, dims = lpstate.check_rows(rows, deep=False)
    return _message(KIND_LP_OPEN, model_key, list(arrays) + [_scalars(dims)], a=bool(deep))


def _round_word(mode, mask=0, has_block=False, has_incumbent=None, incremental=False):
    inc = 0 if has_incumbent is None else 2 if has_incumbent else 1
    return mode | mask << 8 | int(bool(has_block)) << 12 | inc << 13 | int(bool(incremental)) << 15


def encode_round_request(model_key, session, mode, rnd=None, forced=None, p_max=0.1, p_max_ub=0.5, max_selected=None, append=None,
                         incremental=False, remove=None):
    """-> the message's bytes of a round of session `session`.  `mode`: SESSION_SCORE / _RANK / _SELECT with `rnd` (a
    `lpstate.LPRound`) and optionally `append` (a `lpstate.LPRowBlock`), `remove` (row indices, numbered after the append) and
    `forced`; SESSION_APPEND with `append`, `remove` or both alone.  A request without a removal has the bytes it always had."""
    arrays, mask, inc = [], 0, None
    if mode != SESSION_APPEND:
        inc = rnd.has_incumbent
        for name, _ in lpstate.ROUND_FIELDS:
            a = getattr(rnd, name)
            if name in lpstate.OPTIONAL:
                if a is None:
                    continue
                mask |= 1 << lpstate.OPTIONAL.index(name)
            elif a is None:
                raise ValueError(f"{name}: a round must give it")
            arrays.append(np.asarray(a))
    elif append is None and remove is None:
        raise ValueError("an edit needs a block to append or rows to remove")
    if append is not None:
        arrays += [np.asarray(a) for a in append.arrays()]
    if remove is not None:
        arrays.append(np.ascontiguousarray(np.asarray(remove).ravel(), dtype=np.int32))
    return _message(KIND_LP_ROUND, model_key, arrays, forced if mode == SESSION_SELECT else None, p_max, p_max_ub, max_selected, session,
                    _round_word(mode, mask, append is not None, inc, incremental), remove is not None)


def encode_close_request(model_key, session):
    return _message(KIND_LP_CLOSE, model_key, a=session)


# ---- the request kinds, decoded: (the header's three words, the arrays in front of the forced pair) -> the kind's fields -------------
def _lp_arrays(inc, behind=1):       # how many arrays an LP payload of this n_cons slot has, the scalars (and the quality) included
    return len(_LP_FIELDS[inc]) + behind if inc in _LP_FIELDS else -1


def _decode_collect(words, arrays):
    snap, quality = _lp_snapshot(words[0], arrays), arrays[_lp_arrays(words[0])]
    if quality.dtype != np.float64 or quality.ndim != 1:
        raise ProtocolError("malformed quality")
    return dict(snapshot=snap, quality=quality)


def _decode_hybrid(words, arrays):
    scalars = arrays[_HYBRID_ARRAYS - 1]
    if scalars.dtype != np.float64 or scalars.shape != (1,):
        raise ProtocolError("malformed snapshot scalars")
    return dict(snapshot=lpstate.CutSnapshot(**dict(zip((n for n, _ in lpstate.CUT_FIELDS), arrays)), infinity=float(scalars[0])))


def _round_bits(word):
    """The inverse of `_round_word`: (mode, presence mask, has a block, has_incumbent's code, incremental)."""
    return word & 255, word >> 8 & 15, word >> 12 & 1, word >> 13 & 3, word >> 15 & 1


def _round_arrays(session, word, removes):
    """How many arrays a well-formed round of these words carries in front of the forced pair; -1 for words that are none."""
    mode, mask, has_block, inc, _ = _round_bits(word)
    if removes not in (0, 1) or word < 0 or word >> 16 or mode > SESSION_APPEND or inc == 3:
        return -1
    if mode == SESSION_APPEND:
        return 5 * has_block + removes if (has_block or removes) and not mask else -1
    return _ROUND_BASE + bin(mask).count("1") + 5 * has_block + removes


def _decode_round(words, arrays):
    session, word, removes = words
    mode, mask, has_block, inc, incremental = _round_bits(word)
    rnd, at = None, 0
    if mode != SESSION_APPEND:
        fields = {}
        for name, _ in lpstate.ROUND_FIELDS:
            if name in lpstate.OPTIONAL and not mask >> lpstate.OPTIONAL.index(name) & 1:
                continue
            fields[name] = arrays[at]
            at += 1
        rnd = lpstate.LPRound(**fields, has_incumbent=None if inc == 0 else inc == 2)
    block = lpstate.LPRowBlock(*arrays[at:at + 5]) if has_block else None
    remove = None
    if removes:
        remove = arrays[at + 5 * has_block]
        if remove.dtype != np.int32 or remove.ndim != 1:
            raise ProtocolError("malformed list of removed rows")
    return dict(session=session, mode=mode, round=rnd, block=block, remove=remove, incremental=bool(incremental))


def _kind(decode, arrays, model=False, forced=lambda a, b, c: True):
    return dict(decode=decode, arrays=arrays, model=model, forced=forced)


# One row per request kind -- all that the codec and the server's reader know about it; a kind without a row is unknown (10 is).
#   decode  (the three words, the arrays) -> the kind's fields of the decoded dict
#   arrays  (the three words) -> how many arrays a well-formed request carries in front of the forced pair, -1 for words it refuses
#   model   the request names a model that the server must hold
#   forced  (the three words) -> whether forced rows may follow (the dict then has `forced`); None: the header's slot is not looked at
_STATE = _kind(lambda words, arrays: dict(state=tuple(arrays[:7]) + tuple(words)), lambda a, b, c: 7, model=True)
_LP = _kind(lambda words, arrays: dict(snapshot=_lp_snapshot(words[0], arrays)), lambda a, b, c: _lp_arrays(a), model=True)
_KINDS = {
    KIND_SCORE: _STATE, KIND_RANK: _STATE, KIND_SELECT: _STATE,
    KIND_LP_SCORE: _LP, KIND_LP_RANK: _LP, KIND_LP_SELECT: _LP,
    KIND_HYBRID_SELECT: _kind(_decode_hybrid, lambda a, b, c: _HYBRID_ARRAYS),
    KIND_LP_OPEN: _kind(lambda words, arrays: dict(rows=lpstate.LPRows(*arrays[:7], **_take_scalars(arrays[7], "row")), deep=bool(words[0])),
                        lambda a, b, c: 8, model=True, forced=None),
    KIND_LP_ROUND: _kind(_decode_round, _round_arrays, forced=lambda a, b, c: b & 255 == SESSION_SELECT),
    KIND_LP_CLOSE: _kind(lambda words, arrays: dict(session=words[0]), lambda a, b, c: 0, forced=None),
    KIND_COLLECT: _kind(_decode_collect, lambda a, b, c: _lp_arrays(a, 2)),
}
_NO_KIND = _kind(None, lambda a, b, c: -1, forced=None)      # what an unknown kind number looks up: refused with the count check


def decode_request(buf):
    """-> dict(model_key, kind, p_max, p_max_ub, max_selected and the kind's fields); raises ProtocolError on anything malformed."""
    if len(buf) < _REQ.size:
        raise ProtocolError("truncated header")
    magic, kind, n_arrays, key_len, p_max, p_max_ub, max_selected, n_forced, *words = _REQ.unpack_from(buf, 0)
    row = _KINDS.get(kind, _NO_KIND)
    expected, has_forced = row["arrays"](*words), row["forced"] is not None and n_forced >= 0
    if magic != MAGIC or expected < 0 or (has_forced and not row["forced"](*words)) or n_arrays != expected + 2 * has_forced:
        raise ProtocolError("not a request of this protocol")
    at = _REQ.size + key_len
    if at > len(buf):
        raise ProtocolError("truncated model key")
    key = bytes(buf[_REQ.size:at]).decode("utf-8", "replace")
    arrays, at = _get_arrays(buf, at, n_arrays)
    if at != len(buf):
        raise ProtocolError("trailing bytes")
    req = row["decode"](words, arrays)
    req.update(model_key=key, kind=kind, p_max=p_max, p_max_ub=p_max_ub, max_selected=None if max_selected < 0 else max_selected)
    if row["forced"] is not None:
        req["forced"] = (arrays[-2], arrays[-1], n_forced) if has_forced else None
    return req


def encode_reply(arrays=(), n_kept=-1, n_selected=-1, error=None):
    status = 0
    if error is not None:
        status = ERR_VALUE if isinstance(error, ValueError) else ERR_GCNN if type(error).__name__ == "GcnnError" else ERR_OTHER
        arrays = [np.frombuffer(f"{type(error).__name__}: {error}".encode("utf-8", "replace"), np.uint8)]
    parts = [_REP.pack(MAGIC, status, len(arrays), 0, n_kept, n_selected)]
    _put_arrays(parts, arrays)
    return b"".join(parts)


def decode_reply(buf):
    """-> (arrays, n_kept, n_selected); raises what the server reported."""
    if len(buf) < _REP.size:
        raise ProtocolError("truncated reply")
    magic, status, n_arrays, _, n_kept, n_selected = _REP.unpack_from(buf, 0)
    if magic != MAGIC:
        raise ProtocolError("not a reply of this protocol")
    arrays, _ = _get_arrays(buf, _REP.size, n_arrays)
    if status:
        text = arrays[0].tobytes().decode("utf-8", "replace") if arrays else "error"
        raise (ValueError if status == ERR_VALUE else ServerError)(text)
    return arrays, n_kept, n_selected


def _n_selected(n_kept, max_selected):   # `infer.n_selected`, restated: this module imports nothing that imports torch
    return n_kept if max_selected is None else min(n_kept, max_selected)


def _recv_exact(sock, n):
    chunks, got = [], 0
    while got < n:
        c = sock.recv(min(n - got, 1 << 20))
        if not c:
            raise ConnectionError("the scoring server closed the connection")
        chunks.append(c)
        got += len(c)
    return b"".join(chunks)


# ---- client: NumPy only ------------------------------------------------------------------------------------------------------------
class Scores(np.ndarray):
    """Scores as the plugins use them: an ndarray that answers `.numpy()` (model_evaluator.py:103); `rankings` when asked for."""
    rankings = None
    cut_index = None      # the LP calls: state position -> input cut (scores are in STATE order)

    def numpy(self):
        return np.asarray(self)


class Selection:
    """`order` (kept cuts first, best first, then the removed ones), `n_kept`, `n_selected` = min(n_kept, max_selected), `scores`;
    from `select_cuts_lp` also `cut_index`: `cut_index[order[:n_selected]]` are the selected input cuts."""

    features = None       # from `select_cuts_hybrid`: [K, 3] float64 efficacy, integer support, objective parallelism

    def __init__(self, order, n_kept, n_selected, scores, cut_index=None):
        self.order, self.n_kept, self.n_selected, self.scores, self.cut_index = order, n_kept, n_selected, scores, cut_index


# The two reply shapes, each as the server makes it from a result -- `encode_reply`'s (arrays, n_kept, n_selected) -- and as the client
# reads it from what `decode_reply` returns.  `lp`: the result comes from an LP and carries cut_index.
def _scores_reply(res, rank, lp):
    """[scores, rankings?, cut_index?]"""
    arrays = [np.asarray(res)] + ([np.asarray(res.rankings, np.int32)] if rank else [])
    return arrays + ([np.asarray(res.cut_index, np.int32)] if lp else []), -1, -1


def _scores_of(reply, rank, lp):
    scores = reply[0][0].view(Scores)
    scores.rankings, scores.cut_index = reply[0][1] if rank else None, reply[0][-1] if lp else None
    return scores


def _selection_reply(res, max_selected, lp, features=False):
    """[scores, order, cut_index?, features?], n_kept and n_selected in the header"""
    arrays = [np.asarray(res.scores), np.asarray(res.order, np.int32)] + ([np.asarray(res.cut_index, np.int32)] if lp else [])
    return arrays + ([np.asarray(res.features, np.float64)] if features else []), res.n_kept, _n_selected(res.n_kept, max_selected)


def _selection_of(reply, lp, features=False):
    arrays, n_kept, n_selected = reply
    res = Selection(arrays[1], n_kept, n_selected, arrays[0].view(Scores), arrays[2] if lp else None)
    res.features = arrays[3] if features else None
    return res


def _reply_of(base, lp, features=False):
    """(request, result) -> `encode_reply`'s arguments; `base`: KIND_ or, the same numbers, SESSION_SCORE / _RANK / _SELECT."""
    if base == KIND_SELECT:
        return lambda req, res: _selection_reply(res, req["max_selected"], lp, features)
    return lambda req, res: _scores_reply(res, base == KIND_RANK, lp)


class _Closing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class ScoringClient(_Closing):
    def __init__(self, address, model_key, timeout=None):
        self.model_key = model_key
        self.sock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        self.sock.settimeout(timeout)
        self.sock.connect(address)

    def _call(self, message):
        self.sock.sendall(struct.pack("<I", len(message)) + message)
        (n,) = struct.unpack("<I", _recv_exact(self.sock, 4))
        return decode_reply(_recv_exact(self.sock, n))

    def score_state(self, state, rank=False):
        return _scores_of(self._call(encode_request(self.model_key, KIND_RANK if rank else KIND_SCORE, state)), rank, False)

    def select_cuts(self, state, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        return _selection_of(self._call(encode_request(self.model_key, KIND_SELECT, state, forced, p_max, p_max_ub, max_selected)), False)

    def score_lp(self, snapshot, rank=False):
        """`GCNN.score_lp` behind the server: the raw LP goes over the wire, get_state's arithmetic runs on the GPU."""
        return _scores_of(self._call(encode_lp_request(self.model_key, KIND_LP_RANK if rank else KIND_LP_SCORE, snapshot)), rank, True)

    def select_cuts_lp(self, snapshot, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        return _selection_of(self._call(encode_lp_request(self.model_key, KIND_LP_SELECT, snapshot, forced, p_max, p_max_ub, max_selected)), True)

    def select_cuts_hybrid(self, snapshot, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        """`HybridSelector.select_cuts` behind the server: SCIP's hybrid quality (float64, input cut order) and the parallelism
        filter from a `lpstate.CutSnapshot` or `LPSnapshot`.  The `Selection` also carries `.features` [K, 3]."""
        return _selection_of(self._call(encode_hybrid_request(self.model_key, snapshot, forced, p_max, p_max_ub, max_selected)), True, True)

    def collect_lp(self, snapshot, quality, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None):
        """`collect.Collector.collect_lp` behind the server: an expert round of the data collector -- the sample's state and the
        plugin's selection over the expert's float64 `quality` (input cut order) -- as a `lpstate.CollectResult`.  A quality of
        the wrong length or dtype kind, or with a value that is not finite, is refused here, in the worker."""
        arrays, n_kept, n_selected = self._call(encode_collect_request(self.model_key, snapshot, quality, forced, p_max, p_max_ub,
                                                                       max_selected))
        state = tuple(arrays[:7]) + (arrays[0].shape[0], arrays[3].shape[0], arrays[4].shape[0])
        return lpstate.CollectResult(state, arrays[7], arrays[8], arrays[9], n_kept, n_selected, arrays[10], arrays[11])

    def open_lp(self, rows, *, deep=True):
        """`GCNN.open_lp` behind the server: `rows` (`lpstate.LPRows`) goes over the wire once and stays on the server's device;
        returns a `RemoteLPSession`, whose rounds send only the solve, the candidate cuts and the rows to append.  The session
        belongs to this connection: the server closes it when the connection drops."""
        _, sid, _ = self._call(encode_open_request(self.model_key, rows, deep))
        return RemoteLPSession(self, sid, int(np.asarray(rows.row_lhs).shape[0]), int(np.asarray(rows.col_type).shape[0]))

    def get_concrete_function(self):
        """The `(state10, training) -> scores` callable `CustomCutsel(function=...)` stores (model_evaluator.py:310-314)."""
        def get_improvements(state, training=False, rank=False):
            return self.score_state(state, rank)
        return get_improvements

    def close(self):
        self.sock.close()



class RemoteLPSession(_Closing):
    """An `infer.LPSession` held by a scoring server, as a worker sees it (NumPy only): `score`, `select_cuts` (with `append=` and
    `remove=`), `append_rows`, `remove_rows`, `close`, `n_rows`, `n_cols` and use as a context manager, with `LPSession`'s
    signatures and results (`Scores` / `Selection` with `cut_index`); `n_rows` follows the edits the server accepted.  The
    server answers the rounds of different workers that wait at the same time with one call on the device; every reply has the
    bits of the session's own call.  `timings` is accepted for the signature's sake and left alone."""

    def __init__(self, client, session, n_rows, n_cols):
        self.client, self.session, self._n_rows, self.n_cols, self.closed = client, session, n_rows, n_cols, False

    @property
    def n_rows(self):
        return self._n_rows

    def _round(self, mode, rnd, append, remove=None, **kw):
        if self.closed:
            raise ServerError("the LP session is closed")
        n_block = 0 if append is None else int(np.asarray(append.row_lhs).shape[0])
        idx = lpstate.check_remove(remove, self._n_rows + n_block)      # (a bad index raises here, in the worker)
        if idx.size and idx.size == self._n_rows + n_block:
            raise ValueError("remove: the removal would leave no row at all; open a new session instead")
        reply = self.client._call(encode_round_request(self.client.model_key, self.session, mode, rnd, append=append,
                                                       remove=idx if idx.size else None, **kw))
        self._n_rows += n_block - int(idx.size)                           # (the call raised if the server did not adopt the edits)
        return reply

    def score(self, rnd, rank=False, timings=None, append=None, remove=None):
        return _scores_of(self._round(SESSION_RANK if rank else SESSION_SCORE, rnd, append, remove), rank, True)

    def select_cuts(self, rnd, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, timings=None, append=None, remove=None):
        return _selection_of(self._round(SESSION_SELECT, rnd, append, remove, forced=forced, p_max=p_max, p_max_ub=p_max_ub,
                                         max_selected=max_selected), True)

    def append_rows(self, row_ptr, row_col, row_val, row_lhs, row_rhs, incremental=False):
        block = lpstate.LPRowBlock(row_ptr, row_col, row_val, row_lhs, row_rhs)
        if np.asarray(row_lhs).shape[0]:
            self._round(SESSION_APPEND, None, block, incremental=incremental)

    def remove_rows(self, remove):
        """`LPSession.remove_rows` behind the server: only the indices go over the wire.  Removing zero rows is a no-op."""
        if remove is not None and np.asarray(remove).size:
            self._round(SESSION_APPEND, None, None, remove)

    def close(self):
        if not self.closed:
            self.closed = True
            self.client._call(encode_close_request(self.client.model_key, self.session))



# ---- server ------------------------------------------------------------------------------------------------------------------------
class ScoringServer:
    """Owns the models (and with them the GPU).  `address`: path of the AF_UNIX socket, bound and listening from construction on, so
    that requests sent before `start()` simply wait.  `start()` serves in a thread of this process; `serve_forever()` in the
    calling thread.  `stats`: requests, calls (one per group served) and batched_calls (calls that served more than one request),
    max_batch, max_models_per_call (the most models one batched call served: what the `ModelSet` reports, which splits a group of
    more than 8 models; 1 for a call on one model).  `cross_model`: host-state requests of all models share one group per kind
    (and thresholds), served by a `ModelSet` over the models -- a group that holds requests of ONE model still takes that model's
    own call, which is the faster one for it (profiles/mixed_models.txt); False, or models on more than one device, groups by
    model.  `cross_model_lp`: with `cross_model`, the LP kinds share across models in the same way (`ModelSet.score_lps` /
    `select_cuts_lp_many`; profiles/lp_models.txt); False keeps them grouped by model.  `model_set`: the set to use instead of
    `ModelSet(models)` (built on first use).
    Resident LPs (`ScoringClient.open_lp`): at most `max_sessions` at a time, each owned by the connection that opened it and
    closed when that connection drops.  The rounds that wait together are grouped by mode and thresholds, across models, and each
    group goes to `session_group` (default: an `infer.LPSessionGroup` on the first model's device, built on first use) in calls
    of up to 8 sessions; two requests of one session are never in one call: they are served in arrival order in successive ones.
    Rounds with and without a removal share their calls: the default group is made with `batch_removes=True`
    (gcnn_lp_rounds_edit), and `removes=` is handed to the group only in a call where a member removes rows.
    Opens, closes, `append_rows` and `remove_rows` are served one by one.  `stats` counts sessions_open, session_rounds (rounds served),
    session_calls (batched calls the group made on the device: its own counter), max_sessions_per_call (the most sessions one of
    them served) and session_solo_rounds (rounds the group answered through the session's own call: a ranking left to the host, a
    member the batched call declined).
    Expert rounds of a data collector (`ScoringClient.collect_lp`) are served one by one by one `collect.Collector`, built on first
    use; `stats["collect_calls"]` counts them.  They and the hybrid kind need no model: `models` may be empty.
    `ensembles`: {name: [model keys]} -- a client opened with an ensemble's name uses the kinds 0-5 as they are and is answered with
    the MEAN of those models' scores, its ranking or the selection over it (`ModelSet.score_ensemble`, `select_cuts_ensemble` and
    their LP forms; the members' own scores stay on the server).  A name must not be a model key; its 1..8 keys must be loaded
    models, each named once, all on one device.  Every ensemble request is answered with its own call and `stats["ensemble_calls"]`
    counts them -- unless the server was made with `ensemble_batching=True`: then the requests of the kinds 0-5 under ensemble names
    that wait together are grouped by ensemble name, kind and, for selections, thresholds, and each group is answered with one
    `ModelSet.*_ensemble_many` call (gcnn_infer_ensemble_batch / gcnn_lp_ensemble_batch: up to 64 states per C call); the wire
    bytes are the same either way.  `stats["ensemble_calls"]` then counts those calls, `ensemble_batched_calls` the ones that served
    more than one request and `max_ensemble_batch` the most requests one of them served.  Requests of different ensembles never
    share a call.  Every other kind under an ensemble's name gets the error reply of an unknown
    model -- unless the server was made with `ensemble_sessions=True`: then a client opened with an ensemble's name can keep an LP
    resident as under a model key (kinds 7-9, the same wire bytes).  The open gives `ModelSet.open_lp_ensemble` and counts against
    `max_sessions`; each of the session's rounds is answered by its own call (gcnn_lp_round_ensemble), never through the session
    group, in the wave order of the other sessions' rounds, with the mean as the scores; `stats["ensemble_calls"]` and
    `stats["session_rounds"]` count them.  The hybrid and the collector's kinds stay refused."""
    SESSIONS_PER_CALL = 8

    def __init__(self, models, address, backlog=128, cross_model=True, model_set=None, cross_model_lp=True, max_sessions=64,
                 session_group=None, ensembles=None, ensemble_sessions=False, ensemble_batching=False):
        self.models = dict(models)
        self.address = address
        self.ensembles = self._checked_ensembles(ensembles, model_set)
        self.ensemble_sessions = bool(ensemble_sessions)
        self.ensemble_batching = bool(ensemble_batching)
        # a ModelSet needs all models on one device: models spread over several devices are served per model, as before
        one_device = len({str(getattr(m, "device", None)) for m in self.models.values()}) <= 1
        self.cross_model = bool(cross_model) and (model_set is not None or one_device)
        self.cross_model_lp = bool(cross_model_lp)
        self._model_set = model_set
        self.stats = dict(requests=0, calls=0, batched_calls=0, max_batch=0, errors=0, max_models_per_call=0, sessions_open=0,
                          session_rounds=0, session_calls=0, session_solo_rounds=0, max_sessions_per_call=0, collect_calls=0,
                          ensemble_calls=0, ensemble_batched_calls=0, max_ensemble_batch=0)
        self.max_sessions = int(max_sessions)
        self._sessions = {}            # id -> (the connection that owns it, the LPSession)
        self._ensemble_sids = set()    # the ids among them whose session an ensemble scores (`ensemble_sessions`)
        self._next_session = 1
        self._session_group = session_group
        self._listen = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        self._listen.bind(address)
        self._listen.listen(backlog)
        self._wake_r, self._wake_w = socket.socketpair()
        self._closing = False
        self._thread = None
        self._buffers = {}
        self._hybrid = None            # the HybridSelector, built on first use on the device of the first model
        self._collector = None         # the Collector of the expert rounds, built on first use on the same device

    def _checked_ensembles(self, ensembles, model_set):
        """{name: [keys]} as the server keeps it; ValueError for a name that is a model key, for keys that are not loaded models or
        named twice, for fewer than 1 or more than 8 of them, and for models on more than one device."""
        out = {}
        for name, keys in dict(ensembles or {}).items():
            keys = list(keys)
            if name in self.models:
                raise ValueError(f"ensemble {name!r}: the name is a model key")
            if not 1 <= len(keys) <= 8 or len(set(keys)) != len(keys):
                raise ValueError(f"ensemble {name!r}: 1..8 model keys, each once, expected, got {keys!r}")
            missing = [k for k in keys if k not in self.models]
            if missing:
                raise ValueError(f"ensemble {name!r}: no model {missing[0]!r}")
            out[name] = keys
        if out and model_set is None and len({str(getattr(m, "device", None)) for m in self.models.values()}) > 1:
            raise ValueError("ensembles need all models of the server on one device")
        return out

    def _ensemble_one(self, conn, req):
        """A request of the kinds 0-5 under an ensemble's name, answered with its own `ModelSet.*_ensemble` call."""
        kind = req["kind"]
        lp, base, keys = kind in _LP_BASE, _LP_BASE.get(kind, kind), self.ensembles[req["model_key"]]
        self.stats["calls"] += 1
        self.stats["ensemble_calls"] += 1

        def call():
            mset, arg = self._set(), req["snapshot" if lp else "state"]
            if base == KIND_SELECT:
                select = mset.select_cuts_lp_ensemble if lp else mset.select_cuts_ensemble
                return [select(keys, arg, req["forced"], p_max=req["p_max"], p_max_ub=req["p_max_ub"], max_selected=req["max_selected"])]
            return [(mset.score_lp_ensemble if lp else mset.score_ensemble)(keys, arg, rank=base == KIND_RANK)]
        self._answer_group([(conn, req)], call, _reply_of(base, lp))

    def _ensemble_groups(self, pending):
        """The requests of the kinds 0-5 under ensemble names -> {(ensemble name, kind[, p_max, p_max_ub]): [(conn, request)]}, groups
        and members in arrival order (`ensemble_batching`)."""
        groups = {}
        for conn, req in pending:
            kind = req["kind"]
            if req["model_key"] in self.ensembles and kind in _ENSEMBLE_KINDS:
                selects = _LP_BASE.get(kind, kind) == KIND_SELECT
                gkey = (req["model_key"], kind) + ((req["p_max"], req["p_max_ub"]) if selects else ())
                groups.setdefault(gkey, []).append((conn, req))
        return groups

    def _ensemble_many(self, gkey, items):
        """A group of `_ensemble_groups`, answered with one `ModelSet.*_ensemble_many` call: every member gets the reply
        `_ensemble_one` gives for the same result, or its own error."""
        kind = gkey[1]
        lp, base, keys = kind in _LP_BASE, _LP_BASE.get(kind, kind), self.ensembles[gkey[0]]
        self.stats["calls"] += 1
        self.stats["ensemble_calls"] += 1
        self.stats["ensemble_batched_calls"] += len(items) > 1
        self.stats["max_ensemble_batch"] = max(self.stats["max_ensemble_batch"], len(items))

        def call():
            mset, args = self._set(), [r["snapshot" if lp else "state"] for _, r in items]
            if base == KIND_SELECT:
                select = mset.select_cuts_lp_ensemble_many if lp else mset.select_cuts_ensemble_many
                return select(keys, args, [r["forced"] for _, r in items], p_max=gkey[2], p_max_ub=gkey[3], return_exceptions=True)
            return (mset.score_lp_ensemble_many if lp else mset.score_ensemble_many)(keys, args, rank=base == KIND_RANK,
                                                                                     return_exceptions=True)
        self._answer_group(items, call, _reply_of(base, lp))

    def _device(self):
        """The device of the first model; None (the current device) for a server that holds no model: the kinds without one."""
        first = next(iter(self.models.values()), None)
        return None if first is None else first.device

    def _hybrid_selector(self):
        if self._hybrid is None:
            from .hybrid import HybridSelector
            self._hybrid = HybridSelector(self._device())
        return self._hybrid

    def _collect_one(self, conn, req):
        """An expert round (KIND_COLLECT), answered on its own: they are 5 % of a collector's rounds and rarely wait together."""
        self.stats["collect_calls"] += 1

        def call():
            if self._collector is None:
                from .collect import Collector
                self._collector = Collector(self._device())
            return [self._collector.collect_lp(req["snapshot"], req["quality"], req["forced"], p_max=req["p_max"],
                                               p_max_ub=req["p_max_ub"], max_selected=req["max_selected"])]

        def reply_of(req, res):
            arrays = list(res.state[:7]) + [np.asarray(res.cut_index, np.int32), np.asarray(res.improvements, np.float64),
                                            np.asarray(res.order, np.int32), np.asarray(res.hybrid_quality, np.float64),
                                            np.asarray(res.features, np.float64)]
            return arrays, res.n_kept, res.n_selected
        self._answer_group([(conn, req)], call, reply_of)

    def _set(self):
        if self._model_set is None:
            from .model import ModelSet
            self._model_set = ModelSet(self.models)
        return self._model_set

    def start(self):
        self._thread = threading.Thread(target=self.serve_forever, name="gcnn-scoring-server", daemon=True)
        self._thread.start()
        return self

    def close(self):
        """Ends the loop (after the group being served), closes every connection and removes the socket file."""
        self._closing = True
        try:
            self._wake_w.send(b"x")
        except OSError:
            pass
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        else:
            self._shutdown()

    def _shutdown(self):
        for s in list(self._buffers) + [self._listen, self._wake_r, self._wake_w]:
            try:
                s.close()
            except OSError:
                pass
        self._buffers.clear()
        try:
            os.unlink(self.address)
        except OSError:
            pass

    def _reply(self, conn, message):
        try:
            conn.sendall(struct.pack("<I", len(message)) + message)
        except OSError:
            self._drop(conn)

    def _group(self):
        if self._session_group is None:
            from .infer import LPSessionGroup
            self._session_group = LPSessionGroup(next(iter(self.models.values())).device, batch_removes=True)
        return self._session_group

    def _close_session(self, sid):
        _, sess = self._sessions.pop(sid)
        self._ensemble_sids.discard(sid)
        self.stats["sessions_open"] = len(self._sessions)
        sess.close()

    def _drop(self, conn):
        for sid in [sid for sid, (owner, _) in self._sessions.items() if owner is conn]:
            self._close_session(sid)              # a session belongs to the connection that opened it
        if conn in self._buffers:
            del self._buffers[conn]
            try:
                self._sel.unregister(conn)
            except (KeyError, ValueError):
                pass
            conn.close()

    def _read(self, conn, pending):
        try:
            data = conn.recv(1 << 20)
        except OSError:
            data = b""
        if not data:
            self._drop(conn)
            return
        buf = self._buffers[conn]
        buf += data
        while len(buf) >= 4:
            (n,) = struct.unpack_from("<I", buf, 0)
            if n > MAX_MESSAGE:            # the framing itself cannot be trusted any more: answer and hang up
                self.stats["errors"] += 1
                self._reply(conn, encode_reply(error=ProtocolError("message too large")))
                self._drop(conn)
                return
            if len(buf) < 4 + n:
                break
            message = bytes(buf[4:4 + n])
            del buf[:4 + n]
            self.stats["requests"] += 1
            try:
                req = decode_request(message)
                if req["model_key"] in self.ensembles:
                    # hybrid and collector rounds know no ensemble; sessions only where the server was made with `ensemble_sessions`
                    if req["kind"] not in _ENSEMBLE_KINDS and not (self.ensemble_sessions and req["kind"] in _SESSION_KINDS):
                        raise KeyError(f"no model {req['model_key']!r}")
                elif _KINDS[req["kind"]]["model"] and req["model_key"] not in self.models:
                    raise KeyError(f"no model {req['model_key']!r}")
                pending.append((conn, req))
            except Exception as exc:  # noqa: BLE001 -- a bad request gets its error; the server keeps serving
                self.stats["errors"] += 1
                self._reply(conn, encode_reply(error=exc))

    def _fail(self, conn, exc):
        self.stats["errors"] += 1
        if conn in self._buffers:
            self._reply(conn, encode_reply(error=exc))

    def _owned(self, conn, req):
        """The session a round or close request names, if `conn` owns it; else the request gets its error reply."""
        entry = self._sessions.get(req["session"])
        if entry is None or entry[0] is not conn:
            self._fail(conn, KeyError(f"no LP session {req['session']} on this connection"))
            return None
        return entry[1]

    def _serve_sessions(self, items):
        """The session requests that are waiting, in waves: wave k holds every session's k-th request, so that a session's requests
        are served in arrival order and never two in one call.  Within a wave opens, closes and appends are served one by one, the
        rounds grouped by mode and thresholds and handed to the group in calls of up to SESSIONS_PER_CALL sessions."""
        waves, seen = [], {}
        for conn, req in items:
            k = 0
            if req["kind"] != KIND_LP_OPEN:
                k = seen.get(req["session"], 0)
                seen[req["session"]] = k + 1
            while len(waves) <= k:
                waves.append([])
            waves[k].append((conn, req))
        for wave in waves:
            groups = {}
            for conn, req in wave:
                if conn not in self._buffers:
                    continue
                try:
                    if req["kind"] == KIND_LP_OPEN:
                        if len(self._sessions) >= self.max_sessions:
                            raise RuntimeError(f"the server holds {len(self._sessions)} LP sessions already (max_sessions)")
                        keys = self.ensembles.get(req["model_key"])
                        if keys is None:
                            sess = self.models[req["model_key"]].open_lp(req["rows"], deep=req["deep"])
                        else:
                            sess = self._set().open_lp_ensemble(keys, req["rows"], deep=req["deep"])
                        sid, self._next_session = self._next_session, self._next_session + 1
                        self._sessions[sid] = (conn, sess)
                        if keys is not None:
                            self._ensemble_sids.add(sid)
                        self.stats["sessions_open"] = len(self._sessions)
                        self._reply(conn, encode_reply(n_kept=sid))
                        continue
                    sess = self._owned(conn, req)
                    if sess is None:
                        continue
                    if req["kind"] == KIND_LP_CLOSE:
                        self._close_session(req["session"])
                        self._reply(conn, encode_reply())
                    elif req["mode"] == SESSION_APPEND:
                        self._edit_alone(sess, req)
                        self._reply(conn, encode_reply())
                    elif req["session"] in self._ensemble_sids:
                        self._ensemble_round(conn, req, sess)
                    else:
                        gkey = (req["mode"],) + ((req["p_max"], req["p_max_ub"]) if req["mode"] == SESSION_SELECT else ())
                        groups.setdefault(gkey, []).append((conn, req, sess))
                except Exception as exc:  # noqa: BLE001 -- the request gets its error; the server keeps serving
                    self._fail(conn, exc)
            for gkey, members in groups.items():
                for lo in range(0, len(members), self.SESSIONS_PER_CALL):
                    self._serve_rounds(gkey, members[lo:lo + self.SESSIONS_PER_CALL])

    def _ensemble_round(self, conn, req, sess):
        """A round of a session that an ensemble scores, answered with the session's own call: a plain round's reply, the mean as
        the scores."""
        mode = req["mode"]
        self.stats["session_rounds"] += 1
        self.stats["ensemble_calls"] += 1

        def call():
            if mode == SESSION_SELECT:
                return [sess.select_cuts(req["round"], req["forced"], p_max=req["p_max"], p_max_ub=req["p_max_ub"],
                                         max_selected=req["max_selected"], append=req["block"], remove=req.get("remove"))]
            return [sess.score(req["round"], rank=mode == SESSION_RANK, append=req["block"], remove=req.get("remove"))]
        self._answer_group([(conn, req, sess)], call, _reply_of(mode, True))

    @staticmethod
    def _edit_alone(sess, req):
        """An edit without a round: the block appended, then the rows removed that the list names (numbered after the append;
        those that point into the block never reach the device).  Everything the host can refuse is refused before either."""
        block, remove = req["block"], req.get("remove")
        if remove is None:
            sess.append_rows(*block.arrays(), incremental=req["incremental"])
            return
        idx, block = lpstate.split_remove(remove, sess.n_rows, block)
        if block is not None:
            sess.append_rows(*block.arrays(), incremental=req["incremental"])
        if idx.size:
            sess.remove_rows(idx)

    def _serve_rounds(self, gkey, members):
        mode = gkey[0]
        sessions, rounds = [m[2] for m in members], [m[1]["round"] for m in members]
        appends, removes = [m[1]["block"] for m in members], [m[1].get("remove") for m in members]
        more = dict(removes=removes) if any(r is not None for r in removes) else {}      # (a group without the keyword keeps working)
        self.stats["session_rounds"] += len(members)
        group = self._group()

        def call():
            before = (group.calls, group.solo_rounds)
            try:
                if mode == SESSION_SELECT:
                    return group.select_cuts(sessions, rounds, [m[1]["forced"] for m in members], p_max=gkey[1], p_max_ub=gkey[2],
                                             appends=appends, return_exceptions=True, **more)
                return group.score(sessions, rounds, rank=mode == SESSION_RANK, appends=appends, return_exceptions=True, **more)
            finally:
                # the group's own counters: a hand-off whose members the host rejects, or that goes to solo calls, makes no batched call
                self.stats["session_calls"] += group.calls - before[0]
                self.stats["session_solo_rounds"] += group.solo_rounds - before[1]
                self.stats["max_sessions_per_call"] = max(self.stats["max_sessions_per_call"], group.max_sessions_per_call)
        self._answer_group(members, call, _reply_of(mode, True))

    def _answer_group(self, members, call, reply_of):
        """One call for `members` ([(connection, request, ...)]): `call()` returns a result or an exception per member, and one that
        it raises is every member's; a member whose connection dropped meanwhile is skipped."""
        try:
            results = call()
        except Exception as exc:  # noqa: BLE001 -- e.g. thresholds that are not finite: the whole group shares them
            results = [exc] * len(members)
        for (conn, req, *_), res in zip(members, results):
            if conn not in self._buffers:
                continue
            if isinstance(res, Exception):
                self._fail(conn, res)
            else:
                self._reply(conn, encode_reply(*reply_of(req, res)))

    def _grouped(self, pending):
        """The requests of the kinds 0-6, which can share a call -> {(model key or None, kind[, p_max, p_max_ub]): [(conn, request)]}."""
        groups = {}
        for conn, req in pending:
            kind = req["kind"]
            if kind in _SESSION_KINDS or kind == KIND_COLLECT or req["model_key"] in self.ensembles:
                continue
            hybrid = kind == KIND_HYBRID_SELECT       # no model: requests of every model key share a group
            selects = hybrid or _LP_BASE.get(kind, kind) == KIND_SELECT
            # one ModelSet call for all models: host states with `cross_model`, LP snapshots with `cross_model_lp` as well
            shared = hybrid or (self.cross_model and (self.cross_model_lp or kind not in _LP_BASE))
            gkey = (None if shared else req["model_key"], kind) + ((req["p_max"], req["p_max_ub"]) if selects else ())
            groups.setdefault(gkey, []).append((conn, req))
        return groups

    def _callables(self, gkey, mkeys, lp):       # -> (score_many, select_many, the `ModelSet` behind them or None)
        if gkey[1] == KIND_HYBRID_SELECT:
            return None, self._hybrid_selector().select_cuts_many, None
        if gkey[0] is None and len(set(mkeys)) > 1:
            mset = self._set()
            score_many, select_many = (mset.score_lps, mset.select_cuts_lp_many) if lp else (mset.score_states, mset.select_cuts_many)
            return partial(score_many, mkeys), partial(select_many, mkeys), mset
        model = self.models[mkeys[0]]
        return ((model.score_lps, model.select_cuts_lp_many) if lp else (model.score_states, model.select_cuts_many)) + (None,)

    def _serve(self, pending):
        self._serve_sessions([(conn, req) for conn, req in pending if req["kind"] in _SESSION_KINDS])
        for conn, req in pending:
            if req["kind"] == KIND_COLLECT and conn in self._buffers:
                self._collect_one(conn, req)
            elif req["model_key"] in self.ensembles and req["kind"] in _ENSEMBLE_KINDS and not self.ensemble_batching:
                self._ensemble_one(conn, req)
        if self.ensemble_batching:
            for gkey, items in self._ensemble_groups(pending).items():
                self._ensemble_many(gkey, items)
        for gkey, items in self._grouped(pending).items():
            hybrid = gkey[1] == KIND_HYBRID_SELECT
            lp = gkey[1] in _LP_BASE or hybrid
            base = KIND_SELECT if hybrid else _LP_BASE.get(gkey[1], gkey[1])
            self.stats["calls"] += 1
            self.stats["batched_calls"] += len(items) > 1
            self.stats["max_batch"] = max(self.stats["max_batch"], len(items))

            def call():
                states, mkeys, mset = [r["snapshot" if lp else "state"] for _, r in items], [r["model_key"] for _, r in items], None
                try:
                    score_many, select_many, mset = self._callables(gkey, mkeys, lp)
                    if base == KIND_SELECT:
                        return select_many(states, [r["forced"] for _, r in items], p_max=gkey[2], p_max_ub=gkey[3], return_exceptions=True)
                    return score_many(states, rank=base == KIND_RANK, return_exceptions=True)
                finally:
                    if not hybrid:
                        served = 1 if mset is None else getattr(mset, "max_models_per_call", len(set(mkeys)))
                        self.stats["max_models_per_call"] = max(self.stats["max_models_per_call"], served)
            self._answer_group(items, call, _reply_of(base, lp, hybrid))

    def _accept(self):               # a worker has connected: its connection joins those the loop reads
        conn, _ = self._listen.accept()
        self._buffers[conn] = bytearray()
        self._sel.register(conn, selectors.EVENT_READ)

    def serve_forever(self):
        self._sel = sel = selectors.DefaultSelector()
        sel.register(self._listen, selectors.EVENT_READ)
        sel.register(self._wake_r, selectors.EVENT_READ)
        pending = []
        try:
            while not self._closing:
                # block only when nothing is waiting; otherwise sweep up what has arrived and serve -- no timer, no fill target
                events = sel.select(None if not pending else 0)
                for key, _ in events:
                    s = key.fileobj
                    if s is self._listen:
                        self._accept()
                    elif s is self._wake_r:
                        s.recv(16)
                    else:
                        self._read(s, pending)
                if pending and not events:
                    batch, pending = pending, []
                    self._serve(batch)
        finally:
            sel.close()
            self._shutdown()
