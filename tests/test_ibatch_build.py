"""CPU checks of the batched single-call path (gcnn_infer_batch) and the scoring server's client half: declared, exported and bound;
launch names of their own; a sane layout; limits returned, not asserted; kernels that cross-compile for gfx950 without scratch; a
client half that imports no torch; a wire format that returns a state bit for bit."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
SYMBOLS = ("gcnn_infer_batch_layout_for", "gcnn_infer_batch_fill_table", "gcnn_infer_batch")


def test_symbols_in_header_library_and_binding():
    from gcnn_cut_selector_amd import _lib
    header = buildsupport.declared_everywhere(SYMBOLS)
    for name, value in (("MAX", _lib.IBATCH_MAX), ("TABLE_COLS", _lib.IBATCH_TABLE_COLS), ("TABLE_STRIDE", _lib.IBATCH_TABLE_STRIDE),
                        ("SCORES", _lib.IBATCH_SCORES), ("RANK", _lib.IBATCH_RANK), ("SELECT", _lib.IBATCH_SELECT)):
        assert f"#define GCNN_IBATCH_{name} {value}\n" in header
    assert _lib.IBATCH_MAX == 64


def test_launch_names_are_their_own():
    new = launchnames.launch_names(os.path.join(CSRC, "gcnn_ibatch.hpp"))
    assert new == {"k_ib_unpack", "k_ib_by_variable", "k_ib_rank"}
    old = launchnames.launch_names()
    assert len(old) == 28 and not new & old
    for f in ("gcnn_select.hpp", "gcnn_group.hpp", "gcnn_rank.hpp", "gcnn_prenorm.hpp"):
        assert not new & launchnames.launch_names(os.path.join(CSRC, f))
    buildsupport.included_once_after("gcnn_ibatch.hpp", "gcnn_select.hpp")


def _layout(shapes, forced=None, mode=0):
    from gcnn_cut_selector_amd import _lib
    n = len(shapes)
    dims = (_lib.Dims * max(n, 1))(*(_lib.Dims(*s) for s in shapes))
    nf = (C.c_int32 * max(n, 1))(*(f[0] for f in forced)) if forced else None
    nfe = (C.c_int32 * max(n, 1))(*(f[1] for f in forced)) if forced else None
    L = _lib.IbatchLayout()
    return _lib.lib().gcnn_infer_batch_layout_for(n, dims, nf, nfe, mode, C.byref(L)), L, (dims, nf, nfe)


def test_layout_and_limits_need_no_device():
    from gcnn_cut_selector_amd import _lib
    shapes = [(50, 100, 10, 400, 90), (7, 9, 1, 0, 3), (500, 1000, 100, 25000, 9000)]
    forced = [(0, 0), (1, 5), (40, 800)]
    for mode in (0, 1, 2):
        rc, L, (dims, nf, nfe) = _layout(shapes, forced, mode)
        assert rc == 0
        in_off, out_off, dev_off = list(L.in_off), list(L.out_off), list(L.dev_off)[:14]
        assert all(o % 16 == 0 for o in in_off + out_off) and all(o % 256 == 0 for o in dev_off)
        assert in_off == sorted(in_off) and in_off[0] == 0 and L.in_bytes >= in_off[-1] and L.in_bytes % 16 == 0
        assert all(b > a for a, b in zip(in_off[:9], in_off[1:9]))            # every block of these shapes holds something
        assert out_off == sorted(out_off) and L.out_bytes == out_off[3] + 16 * len(shapes)
        assert dev_off == sorted(dev_off) and dev_off[0] >= L.in_bytes and L.arena_bytes >= dev_off[-1]
        tot = L.total
        assert (tot.n_cons, tot.n_vars, tot.n_cuts, tot.n_cons_edges, tot.n_cut_edges) == tuple(sum(s[i] for s in shapes) for i in range(5))
        assert (L.n_forced, L.n_forced_entries) == ((41, 805) if mode == 2 else (0, 0)) and L.max_cuts == 100 and L.n_states == 3
        # the zero block holds the flags and both by-left offset arrays; the table one column per offset kind
        assert in_off[2] - in_off[1] >= 16 * 3 + 4 * (tot.n_cons + 1) + 4 * (tot.n_cuts + 1)
        assert in_off[1] - in_off[0] >= 4 * _lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE
    table = np.full(_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE, -1, np.int32)
    assert _lib.lib().gcnn_infer_batch_fill_table(3, dims, nf, nfe, table.ctypes.data) == 0
    t = table.reshape(_lib.IBATCH_TABLE_COLS, _lib.IBATCH_TABLE_STRIDE)
    want = np.cumsum([[0] * 7] + [list(s) + list(f) for s, f in zip(shapes, forced)], axis=0).T
    assert np.array_equal(t[:, :4], want)
    # limits are returned, before anything could be enqueued
    one = (5, 5, 5, 5, 5)
    assert _layout([], mode=0)[0] == -1 and _layout([one] * 65)[0] == -1 and _layout([one] * 64)[0] == 0
    assert _layout([one], mode=3)[0] == -1 and _layout([(5, 5, -1, 5, 5)])[0] == -1
    assert _layout([one, one], [(0, 0), (0, 3)], 2)[0] == -1                 # entries without a row
    assert _layout([((1 << 23) + 1, 5, 5, 5, 5)] * 2)[0] == -4                # more than 2^24 rows in the union
    assert _layout([(5, 5, 5, 1 << 29, 5)] * 3)[0] == -4
    assert _layout([one, (0, 5, 5, 3, 5)])[0] == -4 and _layout([one, (5, 0, 5, 0, 2)])[0] == -4   # edges with nothing to point at
    assert _layout([one, (0, 0, 0, 0, 0), (5, 5, 4097, 5, 5)], mode=1)[0] == 0   # an empty state and one too large to rank may ride along
    fake = 1 << 20
    lib = _lib.lib()
    dims1 = (_lib.Dims * 1)(_lib.Dims(*one))
    rc, L, _ = _layout([one], mode=2)
    assert lib.gcnn_infer_batch(1, dims1, None, None, 2, fake, fake, fake, fake * 256, L.arena_bytes, float("nan"), 0.5, None) == -1
    assert lib.gcnn_infer_batch(1, dims1, None, None, 2, fake, fake, fake, fake * 256, L.arena_bytes - 1, 0.1, 0.5, None) == -1
    assert lib.gcnn_infer_batch(1, dims1, None, None, 2, fake, fake, fake, fake * 256 + 16, L.arena_bytes, 0.1, 0.5, None) == -1
    assert lib.gcnn_infer_batch(1, dims1, None, None, 0, None, fake, fake, fake * 256, L.arena_bytes, 0.1, 0.5, None) == -1


@pytest.fixture(scope="module")
def device_asm():
    return buildsupport.device_build()


def test_kernels_compile_without_scratch(device_asm):
    rows = device_asm.rows
    new = {k: v for k, v in rows.items() if "k_ib_" in k}
    assert len(new) == 2 and any("k_ib_unpack" in k for k in new) and any("k_ib_rank" in k for k in new), sorted(new)
    for name, v in new.items():
        assert v["scratch"] == 0 and v["lds"] <= 64 * 1024, (name, v)
    for name in new:   # wave64 code objects, and no float atomics in the new kernels
        body = device_asm.body(name)
        assert not re.search(r"atomic_(add|pk_add)_f(16|32|64)", body), name
        assert device_asm.wavefront_size(name) == 64, name


def test_client_half_imports_no_torch():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gcnn_cut_selector_amd.serve as s\n"
            "assert s.ScoringClient and s.encode_request and s.decode_reply\n"
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.')]\n"
            "assert not bad, bad\n"
            "assert 'gcnn_cut_selector_amd._lib' not in sys.modules and 'gcnn_cut_selector_amd.model' not in sys.modules\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_wire_format_round_trips_bit_for_bit():
    from gcnn_cut_selector_amd import serve, synthetic, utils
    state, _ = synthetic.make_sample("setcov", 1, scale=0.2)
    inp = utils.state_to_inputs(state)
    inp[0][0, 0] = np.nan
    inp[3][1, 4] = -0.0
    inp[6][0, 0] = np.float32(1e-42)                                     # a subnormal survives
    req = serve.decode_request(serve.encode_request("setcov/0", serve.KIND_SCORE, inp))
    assert req["model_key"] == "setcov/0" and req["kind"] == serve.KIND_SCORE and req["forced"] is None and req["max_selected"] is None
    assert all(_same(a, b) for a, b in zip(req["state"][:7], inp[:7])) and req["state"][7:] == tuple(int(x) for x in inp[7:])
    # float64 / int64 arrays as get_state produces them cross as they are
    wide = tuple(np.asarray(a, np.float64) if np.asarray(a).dtype.kind == "f" else np.asarray(a, np.int64) for a in inp[:7]) + inp[7:]
    req = serve.decode_request(serve.encode_request("m", serve.KIND_RANK, wide))
    assert all(_same(a, b) for a, b in zip(req["state"][:7], wide[:7]))
    forced = (np.array([[0, 0, 2], [3, 1, 0]], np.int32), np.array([0.5, -0.5, 1.0], np.float32))
    req = serve.decode_request(serve.encode_request("m", serve.KIND_SELECT, inp, forced, 0.25, 0.75, 7))
    assert (req["p_max"], req["p_max_ub"], req["max_selected"], req["forced"][2]) == (0.25, 0.75, 7, 3)
    assert _same(req["forced"][0], forced[0]) and _same(req["forced"][1], forced[1])
    # replies: arrays, counters, and errors that come back as exceptions
    scores = np.array([0.5, np.nan, -1.0], np.float32)
    arrays, n_kept, n_sel = serve.decode_reply(serve.encode_reply([scores, np.array([0, 2, 1], np.int32)], 2, 1))
    assert _same(arrays[0], scores) and arrays[1].tolist() == [0, 2, 1] and (n_kept, n_sel) == (2, 1)
    with pytest.raises(ValueError, match="out of range"):
        serve.decode_reply(serve.encode_reply(error=ValueError("edge index out of range")))
    with pytest.raises(serve.ServerError, match="KeyError"):
        serve.decode_reply(serve.encode_reply(error=KeyError("no model")))
    # malformed messages are refused, never executed
    good = serve.encode_request("m", serve.KIND_SCORE, inp)
    for bad in (b"", good[:10], b"XXXX" + good[4:], good[:-1], good + b"\0", good[:4] + bytes([9]) + good[5:]):
        with pytest.raises(serve.ProtocolError):
            serve.decode_request(bad)
    assert b"pickle" not in open(serve.__file__, "rb").read().replace(b"no pickle", b"")
