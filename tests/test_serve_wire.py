"""The bytes of every request kind of the scoring server (serve.py), pinned independently of its encoders: each `encode_*_request`
against a message assembled by hand from the documented layout (`servecommon.by_hand`), the hand-built bytes decoded and every field
of the dict compared, and a table of malformed messages that `decode_request` must refuse with `ProtocolError`.  The round kind's
bytes are pinned in test_lpedits_host.py; here it takes part in the malformed table."""
import struct

import numpy as np
import pytest

from gcnn_cut_selector_amd import lpstate, serve, synthetic, utils
from servecommon import BLOCK, FORCED, by_hand, snap

COMMON = {"model_key", "kind", "p_max", "p_max_ub", "max_selected"}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _state():
    return utils.state_to_inputs(synthetic.make_sample("setcov", 1, scale=0.2)[0])


def _state_forced(state):
    """Three forced rows over the first columns of the state: (edge_inds [2, E], values [E])."""
    return np.array([[0, 0, 1, 2], [0, 3, 1, state[8] - 1]], np.int32), np.array([1.0, -1.0, 0.5, 2.0], np.float32)


def _without_incumbent(s):
    return lpstate.LPSnapshot(**{**{k: getattr(s, k) for k in s.__dataclass_fields__}, "col_primal": None, "col_primal_avg": None})


def _lp_arrays(s, inc):
    """The LP payload from the layout's description: the snapshot's arrays in `lpstate.FIELDS` order with their packed dtypes,
    without the primal pair when there is no incumbent, then the float64 scalars infinity, sum_epsilon, n_model_vars, obj_norm."""
    arrays = [np.asarray(getattr(s, n)).astype(dt) for n, dt in lpstate.FIELDS if inc or not n.startswith("col_primal")]
    return arrays + [np.array([1e20, 1e-6, 3.0, np.sqrt(5.0)])]


def _cut_arrays(s):
    return [np.asarray(getattr(s, n)).astype(dt) for n, dt in lpstate.CUT_FIELDS] + [np.array([1e20])]


def _row_arrays(s):
    return [np.asarray(getattr(s, n)).astype(dt) for n, dt in lpstate.ROW_FIELDS] + [np.array([1e20, 1e-6, 3.0, np.sqrt(5.0)])]


def _round_arrays(s):
    return [np.asarray(getattr(s, n)).astype(dt) for n, dt in lpstate.ROUND_FIELDS]


def _check_common(req, kind, key, p_max, p_max_ub, max_selected):
    assert (req["model_key"], req["kind"], req["p_max"], req["p_max_ub"], req["max_selected"]) == (key, kind, p_max, p_max_ub, max_selected)


def _check_forced(got, want, n_forced):
    if want is None:
        assert got is None
    else:
        assert len(got) == 3 and _same(got[0], want[0]) and _same(got[1], want[1]) and got[2] == n_forced


def _check_snapshot(got, s, inc):
    assert isinstance(got, lpstate.LPSnapshot)
    for n, dt in lpstate.FIELDS:
        if n.startswith("col_primal") and not inc:
            assert getattr(got, n) is None
        else:
            assert _same(getattr(got, n), np.asarray(getattr(s, n)).astype(dt)), n
    assert (got.infinity, got.sum_epsilon, got.n_model_vars, got.obj_norm, got.has_incumbent) == (1e20, 1e-6, 3, np.sqrt(5.0), inc)
    assert type(got.n_model_vars) is int and type(got.has_incumbent) is bool


# ---- kinds 0-2: host states --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_host_state_kinds(kind):
    state = _state()
    seven, sizes = list(state[:7]), tuple(int(x) for x in state[7:])
    assert [a.dtype.name for a in seven] == ["float32", "int32", "float32", "float32", "float32", "int32", "float32"]
    fi, fv = _state_forced(state)
    # (forced as the encoder takes it, thresholds and max_selected, n_forced on the wire)
    for forced, more, n_forced in ((None, (), -1), (None, (None, 0.2, 0.6, 3), -1), ((fi, fv, 5), (0.2, 0.6), 5), ((fi, fv), (0.25, 0.75, 0), 3)):
        args = more if forced is None else (forced,) + more
        p_max, p_max_ub = (args[1], args[2]) if len(args) > 2 else (0.1, 0.5)
        max_selected = args[3] if len(args) > 3 else None
        message = by_hand(kind, b"setcov/0", seven + ([fi, fv] if forced else []), p_max, p_max_ub,
                          -1 if max_selected is None else max_selected, n_forced, *sizes)
        assert serve.encode_request("setcov/0", kind, state, *args) == message
        req = serve.decode_request(message)
        assert set(req) == COMMON | {"state", "forced"}
        _check_common(req, kind, "setcov/0", p_max, p_max_ub, max_selected)
        assert len(req["state"]) == 10 and all(_same(a, b) for a, b in zip(req["state"][:7], seven)) and req["state"][7:] == sizes
        _check_forced(req["forced"], forced, n_forced)
    assert (serve.KIND_SCORE, serve.KIND_RANK, serve.KIND_SELECT) == (0, 1, 2)


# ---- kinds 3-5: LP snapshots -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inc", (True, False))
@pytest.mark.parametrize("kind", (3, 4, 5))
def test_lp_kinds(kind, inc):
    s = snap() if inc else _without_incumbent(snap())
    arrays = _lp_arrays(s, inc)
    assert len(arrays) == (22 if inc else 20)
    for forced, more, head in ((None, (), (0.1, 0.5, -1, -1)), (FORCED, (0.2, 0.6, 3), (0.2, 0.6, 3, 1))):
        message = by_hand(kind, b"m", arrays + ([FORCED[0], FORCED[1]] if forced else []), *head, a=int(inc))
        assert serve.encode_lp_request("m", kind, s, forced, *more) == message
        req = serve.decode_request(message)
        assert set(req) == COMMON | {"snapshot", "forced"}
        _check_common(req, kind, "m", head[0], head[1], None if head[2] < 0 else head[2])
        _check_snapshot(req["snapshot"], s, inc)
        _check_forced(req["forced"], forced, 1)
    assert (serve.KIND_LP_SCORE, serve.KIND_LP_RANK, serve.KIND_LP_SELECT) == (3, 4, 5)


# ---- kind 6: the hybrid selection --------------------------------------------------------------------------------------------------
def test_hybrid_kind():
    s = snap()
    arrays = _cut_arrays(s)
    assert len(arrays) == 9 and serve.KIND_HYBRID_SELECT == 6
    for forced, more, head in ((None, (), (0.1, 0.5, -1, -1)), (FORCED, (0.2, 0.6, 3), (0.2, 0.6, 3, 1))):
        message = by_hand(6, b"any", arrays + ([FORCED[0], FORCED[1]] if forced else []), *head)
        assert serve.encode_hybrid_request("any", s, forced, *more) == message
        req = serve.decode_request(message)
        assert set(req) == COMMON | {"snapshot", "forced"}
        _check_common(req, 6, "any", head[0], head[1], None if head[2] < 0 else head[2])
        assert isinstance(req["snapshot"], lpstate.CutSnapshot) and req["snapshot"].infinity == 1e20
        assert all(_same(getattr(req["snapshot"], n), a) for (n, _), a in zip(lpstate.CUT_FIELDS, arrays))
        _check_forced(req["forced"], forced, 1)


# ---- kind 7: opening a resident LP -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deep", (True, False))
def test_open_kind(deep):
    rows = lpstate.LPRows.from_snapshot(snap())
    arrays = _row_arrays(snap())
    assert len(arrays) == 8 and serve.KIND_LP_OPEN == 7
    message = by_hand(7, b"setcov/0", arrays, a=int(deep))
    assert serve.encode_open_request("setcov/0", rows, deep) == message
    if deep:
        assert serve.encode_open_request("setcov/0", rows) == message
    req = serve.decode_request(message)
    assert set(req) == COMMON | {"rows", "deep"}
    _check_common(req, 7, "setcov/0", 0.0, 0.0, None)
    assert req["deep"] is deep and isinstance(req["rows"], lpstate.LPRows)
    assert all(_same(getattr(req["rows"], n), a) for (n, _), a in zip(lpstate.ROW_FIELDS, arrays))
    assert (req["rows"].infinity, req["rows"].sum_epsilon, req["rows"].n_model_vars, req["rows"].obj_norm) == (1e20, 1e-6, 3, np.sqrt(5.0))
    assert type(req["rows"].n_model_vars) is int


# ---- kind 11: an expert round ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inc", (True, False))
def test_collect_kind(inc):
    s = snap() if inc else _without_incumbent(snap())
    quality = np.array([0.25, -0.0])
    arrays = _lp_arrays(s, inc) + [quality]
    assert serve.KIND_COLLECT == 11
    for forced, more, head in ((None, (), (0.1, 0.5, -1, -1)), (FORCED, (0.2, 0.6, 3), (0.2, 0.6, 3, 1))):
        message = by_hand(11, b"", arrays + ([FORCED[0], FORCED[1]] if forced else []), *head, a=int(inc))
        assert serve.encode_collect_request("", s, quality, forced, *more) == message
        assert serve.encode_collect_request("", s, [0.25, -0.0], forced, *more) == message
        req = serve.decode_request(message)
        assert set(req) == COMMON | {"snapshot", "quality", "forced"}
        _check_common(req, 11, "", head[0], head[1], None if head[2] < 0 else head[2])
        _check_snapshot(req["snapshot"], s, inc)
        assert _same(req["quality"], quality)
        _check_forced(req["forced"], forced, 1)


def test_round_and_close_decode_to_their_fields():
    """Their bytes are pinned in test_lpedits_host.py; here the decoded dicts' keys, which every kind above has pinned too."""
    rnd = lpstate.LPRound.from_snapshot(snap())
    word = 2 | 15 << 8 | 1 << 12                      # mode, all four optional arrays, a block; has_incumbent left None
    message = by_hand(8, b"m", _round_arrays(snap()) + list(BLOCK.arrays()) + [np.array([3, 0], np.int32), FORCED[0], FORCED[1]],
                      0.2, 0.6, 3, 1, 41, word, 1)
    assert serve.encode_round_request("m", 41, serve.SESSION_SELECT, rnd, FORCED, 0.2, 0.6, 3, append=BLOCK, remove=[3, 0]) == message
    req = serve.decode_request(message)
    assert set(req) == COMMON | {"session", "mode", "round", "block", "remove", "incremental", "forced"}
    _check_common(req, 8, "m", 0.2, 0.6, 3)
    assert (req["session"], req["mode"], req["incremental"]) == (41, 2, False) and req["round"].has_incumbent is None
    assert all(_same(getattr(req["round"], n), a) for (n, _), a in zip(lpstate.ROUND_FIELDS, _round_arrays(snap())))
    assert all(_same(a, b) for a, b in zip(req["block"].arrays(), BLOCK.arrays())) and _same(req["remove"], np.array([3, 0], np.int32))
    _check_forced(req["forced"], FORCED, 1)
    req = serve.decode_request(by_hand(9, b"m", [], a=12))
    assert set(req) == COMMON | {"session"} and req["session"] == 12
    _check_common(req, 9, "m", 0.0, 0.0, None)


# ---- malformed messages ------------------------------------------------------------------------------------------------------------
def _well_formed():
    """kind -> [(header arguments of `by_hand` behind the arrays, arrays)], one or two well-formed requests of every kind."""
    state, s = _state(), snap()
    sizes = dict(zip("abc", (int(x) for x in state[7:])))
    fi, fv = _state_forced(state)
    pair = [FORCED[0], FORCED[1]]
    word = 15 << 8 | 2 << 13                          # all four optional arrays, has_incumbent True
    out = {k: [(dict(p_max=0.1, p_max_ub=0.5, **sizes), list(state[:7])),
               (dict(p_max=0.1, p_max_ub=0.5, n_forced=3, **sizes), list(state[:7]) + [fi, fv])] for k in (0, 1, 2)}
    for k in (3, 4, 5):
        out[k] = [(dict(p_max=0.1, p_max_ub=0.5, a=1), _lp_arrays(s, True)),
                  (dict(p_max=0.1, p_max_ub=0.5, n_forced=1, a=0), _lp_arrays(s, False) + pair)]
    out[6] = [(dict(p_max=0.1, p_max_ub=0.5), _cut_arrays(s)), (dict(p_max=0.1, p_max_ub=0.5, n_forced=1), _cut_arrays(s) + pair)]
    out[7] = [(dict(a=1), _row_arrays(s))]
    out[8] = [(dict(p_max=0.1, p_max_ub=0.5, a=7, b=word), _round_arrays(s)),
              (dict(p_max=0.1, p_max_ub=0.5, n_forced=1, a=7, b=2 | word | 1 << 12, c=1),
               _round_arrays(s) + list(BLOCK.arrays()) + [np.array([1], np.int32)] + pair),
              (dict(a=7, b=3 | 1 << 12), list(BLOCK.arrays()))]
    out[9] = [(dict(a=7), [])]
    out[11] = [(dict(p_max=0.1, p_max_ub=0.5, a=1), _lp_arrays(s, True) + [np.zeros(2)]),
               (dict(p_max=0.1, p_max_ub=0.5, n_forced=1, a=0), _lp_arrays(s, False) + [np.zeros(2)] + pair)]
    return out


def _malformed():
    """[(what is wrong, the message)]."""
    good = _well_formed()
    assert sorted(good) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]
    bad = []
    for kind, forms in good.items():
        for i, (head, arrays) in enumerate(forms):
            message = by_hand(kind, b"key", arrays, **head)
            assert serve.decode_request(message)["kind"] == kind                  # (the table spoils messages that are accepted)
            bad.append((f"kind {kind}/{i}: one array too many", by_hand(kind, b"key", arrays + [np.zeros(1)], **head)))
            if arrays:
                bad.append((f"kind {kind}/{i}: one array too few", by_hand(kind, b"key", arrays[:-1], **head)))
            bad.append((f"kind {kind}/{i}: a trailing byte", message + b"\0"))
            bad.append((f"kind {kind}/{i}: a truncated key", message[:serve._REQ.size + 2]))
            bad.append((f"kind {kind}/{i}: a truncated header", message[:serve._REQ.size - 1]))
            bad.append((f"kind {kind}/{i}: a truncated last array", message[:-1]) if arrays else ("a wrong magic", b"GCS2" + message[4:]))
            for other in [10] + list(range(12, 256)):
                if i == 0 and kind in (0, 8, 9, 11):
                    bad.append((f"kind {kind} relabelled {other}", message[:4] + bytes([other]) + message[5:]))
    # the n_cons slot of an LP kind says whether there is an incumbent: 0 or 1
    for kind in (3, 4, 5, 11):
        head, arrays = good[kind][0]
        bad.append((f"kind {kind}: n_cons of 2", by_hand(kind, b"key", arrays, **{**head, "a": 2})))
        bad.append((f"kind {kind}: n_cons of -1", by_hand(kind, b"key", arrays, **{**head, "a": -1})))
    # the scalars: one float64 array of four values (one for the hybrid kind), n_model_vars finite
    four = np.array([1e20, 1e-6, 3.0, 1.0])
    for kind in (3, 4, 5, 7, 11):
        for i, (head, arrays) in enumerate(good[kind]):
            at = 7 if kind == 7 else 21 if head["a"] else 19
            assert _same(arrays[at], np.array([1e20, 1e-6, 3.0, np.sqrt(5.0)]))
            for what, scalars in (("float32", four.astype(np.float32)), ("int64", np.array([1, 1, 3, 1], np.int64)), ("five values", np.append(four, 0.0)),
                                  ("three values", four[:3]), ("shape (4, 1)", four.reshape(4, 1)), ("shape (1, 4)", four.reshape(1, 4)),
                                  ("n_model_vars nan", np.array([1e20, 1e-6, np.nan, 1.0])), ("n_model_vars inf", np.array([1e20, 1e-6, np.inf, 1.0])),
                                  ("n_model_vars -inf", np.array([1e20, 1e-6, -np.inf, 1.0]))):
                bad.append((f"kind {kind}/{i}: scalars {what}", by_hand(kind, b"key", arrays[:at] + [scalars] + arrays[at + 1:], **head)))
    for i, (head, arrays) in enumerate(good[6]):
        for what, scalars in (("float32", np.array([1e20], np.float32)), ("two values", np.array([1e20, 1.0])), ("shape (1, 1)", np.full((1, 1), 1e20))):
            bad.append((f"kind 6/{i}: scalars {what}", by_hand(6, b"key", arrays[:8] + [scalars] + arrays[9:], **head)))
    # the expert's quality: a float64 vector
    for i, (head, arrays) in enumerate(good[11]):
        at = 22 if head["a"] else 20
        assert _same(arrays[at], np.zeros(2))
        for what, q in (("int64", np.zeros(2, np.int64)), ("float32", np.zeros(2, np.float32)), ("shape (2, 1)", np.zeros((2, 1))),
                        ("shape (1, 2)", np.zeros((1, 2)))):
            bad.append((f"kind 11/{i}: quality {what}", by_hand(11, b"key", arrays[:at] + [q] + arrays[at + 1:], **head)))
    # an array descriptor that does not describe its buffer
    head, arrays = good[7][0]
    message = by_hand(7, b"key", arrays, **head)
    at = len(message) - 32 - 24                                                    # the scalars' descriptor: float64, rank 1, (4,), 32 bytes
    assert struct.unpack_from("<BBHIIQ4x", message, at) == (1, 1, 0, 4, 0, 32)
    for what, desc in (("an unknown dtype", (6, 1, 0, 4, 0, 32)), ("rank 3", (1, 3, 0, 4, 0, 32)), ("more values than bytes", (1, 1, 0, 5, 0, 32)),
                       ("more bytes than the message", (1, 1, 0, 5, 0, 40))):
        bad.append((f"a descriptor of {what}", message[:at] + struct.pack("<BBHIIQ4x", *desc) + message[at + 24:]))
    bad.append(("an empty message", b""))
    return bad


MALFORMED = _malformed()


def test_the_table_covers_what_it_claims():
    names = [n for n, _ in MALFORMED]
    assert len(names) == len(set(names))
    for other in [10] + list(range(12, 256)):
        assert f"kind 0 relabelled {other}" in names and f"kind 9 relabelled {other}" in names
    for kind in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11):
        assert f"kind {kind}/0: one array too many" in names and f"kind {kind}/0: a trailing byte" in names
        assert (f"kind {kind}/0: one array too few" in names) == (kind != 9)             # a close carries no array to drop


def test_malformed_messages_are_refused():
    accepted = []
    for what, message in MALFORMED:
        try:
            serve.decode_request(message)
        except serve.ProtocolError:
            continue
        except Exception as exc:  # noqa: BLE001 -- anything else is reported with its name, not raised at the first
            accepted.append(f"{what}: {type(exc).__name__}: {exc}")
            continue
        accepted.append(f"{what}: accepted")
    assert not accepted, accepted[:20]


def test_n_selected_agrees_with_infer():
    from gcnn_cut_selector_amd import infer
    for n_kept, max_selected in ((0, None), (3, None), (3, 1), (3, 7), (0, 0)):
        assert serve._n_selected(n_kept, max_selected) == infer.n_selected(n_kept, max_selected)
