"""CPU checks of the hybrid selection's native side (gcnn_hybrid_select) and of its request kind in the scoring server: declared,
exported and bound at ABI 13; four launch names of its own file only; three kernels that cross-compile for gfx950 as wave64 without
scratch or float atomics, the fp64 filter inside the LDS that keeps two blocks per CU; the LP path's and the selection's kernels
keep their names; a self-consistent layout; limits returned, not asserted; a wire format that returns a snapshot bit for bit."""
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
HYBRID = os.path.join(CSRC, "gcnn_hybrid.hpp")
NAMES = {"k_hyb_stats", "k_hyb_emit", "k_hyb_pairs", "k_hyb_filter"}       # k_hyb_pairs: the record of k_sel_pairs on the hybrid rows
KERNELS = {"k_hyb_stats", "k_hyb_emit", "k_hyb_filter"}
SYMBOLS = ("gcnn_hybrid_layout_for", "gcnn_hybrid_fill_table", "gcnn_hybrid_select")


def test_symbols_in_header_binding_and_library_abi_13():
    header = buildsupport.declared_everywhere(SYMBOLS)
    assert "gcnn_hybrid_dims" in header and "gcnn_hybrid_layout" in header
    from gcnn_cut_selector_amd import _lib
    assert int(re.search(r"#define GCNN_HYBRID_ARRAYS (\d+)", header).group(1)) == _lib.HYBRID_ARRAYS
    for name, value in (("QUALITY", _lib.HYBRID_QUALITY), ("RANK", _lib.HYBRID_RANK), ("SELECT", _lib.HYBRID_SELECT)):
        assert int(re.search(rf"#define GCNN_HYBRID_{name} (\d+)", header).group(1)) == value


def test_launch_names_are_its_own():
    names = launchnames.launch_names(HYBRID)
    assert names == NAMES
    assert len(launchnames.launch_names()) == 28 and not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_hybrid.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_hybrid.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp")


def test_kernels_compile_wave64_without_scratch_or_float_atomics():
    build = buildsupport.device_build()
    new = {k: v for k, v in build.rows.items() if "k_hyb_" in k}
    assert len(new) == 3 and all(any(n in k for k in new) for n in KERNELS), sorted(new)
    for name, v in new.items():
        assert v["scratch"] == 0, (name, v)
        assert not re.search(r"atomic_(add|pk_add)_f(16|32|64)", build.body(name)), name
        assert build.wavefront_size(name) == 64, name
        if "filter" in name:      # keys 32 KiB + order 16 + temporary 16 + low flags 4: two blocks per CU (160 KiB)
            assert 68 * 1024 <= v["lds"] <= 80 * 1024, v
        else:
            assert v["lds"] <= 16 * 1024, (name, v)
    # the kernels whose bodies moved into shared device functions keep their names (and so their argument structs)
    rows = list(build.rows)
    for name, struct in (("k_lp_stats", "LpArgs"), ("k_lp_emit", "LpArgs"), ("k_sel_pairs", "SelArgs"), ("k_sel_filter", "SelArgs")):
        assert sum(bool(re.search(rf"{name}\d*{struct}", r)) for r in rows) == 1, name
    assert sum("k_lp_" in r for r in rows) == 2 and sum("k_sel_" in r for r in rows) == 2 and sum("k_lpset_" in r for r in rows) == 2
    sel = next(v for r, v in build.rows.items() if "k_sel_filter" in r)
    assert sel["lds"] <= 56 * 1024          # the fp32 instance did not grow with the template


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_cols=50, n_cuts=7, cut_nnz=33, reserved=0, infinity=1e20)
    f.update(over)
    return _lib.HybridDims(**f)


def _layout(dims, forced=None, mode=2):
    from gcnn_cut_selector_amd import _lib
    n = len(dims)
    d = (_lib.HybridDims * max(n, 1))(*dims)
    nf = (C.c_int32 * max(n, 1))(*(f[0] for f in forced)) if forced else None
    nfe = (C.c_int32 * max(n, 1))(*(f[1] for f in forced)) if forced else None
    L = _lib.HybridLayout()
    return _lib.lib().gcnn_hybrid_layout_for(n, d, nf, nfe, mode, C.byref(L)), L, (d, nf, nfe)


def test_layout_is_self_consistent():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    dims = [_dims(), _dims(n_cuts=0, cut_nnz=0), _dims(n_cols=300), _dims(n_cuts=600, cut_nnz=5000)]
    forced = [(0, 0), (2, 9), (1, 1), (0, 0)]
    n, K, E = len(dims), 7 + 0 + 7 + 600, 33 + 0 + 33 + 5000
    for mode in (0, 1, 2):
        rc, L, (d, nf, nfe) = _layout(dims, forced if mode == 2 else None, mode)
        assert rc == 0 and (L.n_snapshots, L.total_cuts, L.total_nnz, L.max_cuts, L.max_cols) == (n, K, E, 600, 300)
        F, FE = (3, 10) if mode == 2 else (0, 0)
        assert (L.n_forced, L.n_forced_entries) == (F, FE)
        end = L.table_bytes
        assert L.table_bytes % 16 == 0
        for s, x in enumerate(dims):
            sizes = [4 * (x.n_cuts + 1), 4 * x.cut_nnz, 8 * x.cut_nnz, 8 * x.n_cuts, 8 * x.n_cuts, x.n_cols, 8 * x.n_cols, 8 * x.n_cols]
            for off, size in zip(L.snap_off[s], sizes):
                assert off % 16 == 0 and off >= end
                end = off + size
        f = list(L.forced_off)
        assert end <= f[0] and f[0] + 4 * (F + 1) <= f[1] and f[1] + 4 * FE <= f[2] and f[2] + 4 * FE <= L.in_bytes
        out = list(L.out_off)
        assert out[0] == 0 and out[0] + 8 * K <= out[1] and out[1] + 24 * K <= out[2] and out[2] + 4 * K <= out[3]
        assert out[3] + 4 * n <= out[4] and out[4] + 16 * n <= L.out_bytes and all(o % 16 == 0 for o in out)
        rows = list(L.rows_off)
        assert L.in_bytes <= L.out_dev_off and L.out_dev_off + L.out_bytes <= rows[0] and rows[0] + 4 * (K + 1) <= rows[1]
        assert rows[1] + 4 * E <= rows[2] and rows[2] + 4 * E <= L.ws_off
        ws = lib.gcnn_select_workspace_bytes(K, F, 600) if mode == 2 else 0
        assert L.ws_off + ws <= L.scratch_off and L.scratch_off + L.scratch_base[n - 1] < L.arena_bytes
        assert all(o % 256 == 0 for o in (L.out_dev_off, *rows, L.ws_off, L.scratch_off, L.arena_bytes))
        # the table: block prefixes, cut and forced offsets, and descriptors that stay inside the arena
        table = np.full(L.table_bytes // 4, -1, np.int32)
        assert lib.gcnn_hybrid_fill_table(n, d, nf, nfe, mode, table.ctypes.data) == 0
        stride = _lib.IBATCH_TABLE_STRIDE
        head = table[:4 + 4 * stride]
        chunks = lambda x: -(-x // 256)  # noqa: E731
        assert head[0] == n
        assert head[4:4 + n + 1].tolist() == np.cumsum([0] + [chunks(x.n_cols) + chunks(x.n_cuts) for x in dims]).tolist()
        assert head[4 + stride:][:n + 1].tolist() == np.cumsum([0] + [chunks(x.n_cuts) + 1 for x in dims]).tolist()
        assert head[4 + 2 * stride:][:n + 1].tolist() == np.cumsum([0] + [x.n_cuts for x in dims]).tolist()
        assert head[4 + 3 * stride:][:n + 1].tolist() == np.cumsum([0] + [f[0] if mode == 2 else 0 for f in forced]).tolist()
        entry = (L.table_bytes - 4 * head.size) // n
        assert entry % 16 == 0
        k0 = e0 = 0
        for s, x in enumerate(dims):
            pos = table[head.size + s * entry // 4:][:2 * 18].view(np.int64)
            assert (pos >= 0).all() and (pos < L.arena_bytes).all() and pos[:8].tolist() == list(L.snap_off[s])
            assert (pos[8:12] >= L.scratch_off + L.scratch_base[s]).all()
            assert pos[12] == L.out_dev_off + out[0] + 8 * k0 and pos[13] == L.out_dev_off + out[1] + 24 * k0
            assert pos[14:17].tolist() == [rows[0] + 4 * k0, rows[1] + 4 * e0, rows[2] + 4 * e0]
            assert pos[17] == L.out_dev_off + out[4] + 16 * s
            k0, e0 = k0 + x.n_cuts, e0 + x.cut_nnz


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    one = _dims()
    assert _layout([])[0] == -1 and _layout([one] * 65)[0] == -1 and _layout([one] * 64)[0] == 0
    assert _layout([one], mode=3)[0] == -1 and _layout([one], mode=-1)[0] == -1
    for over in (dict(n_cols=-1), dict(n_cuts=-1), dict(cut_nnz=-1), dict(infinity=0.0), dict(infinity=float("nan"))):
        assert _layout([one, _dims(**over)])[0] == -1, over
    assert _layout([one, one], [(0, 0), (0, 3)])[0] == -1                               # entries without a row
    many = _dims(n_cuts=4097, cut_nnz=5000)
    assert _layout([one, many], mode=0)[0] == 0                                          # the quality alone has no limit
    assert _layout([one, many], mode=1)[0] == -4 and _layout([one, many], mode=2)[0] == -4
    assert _layout([one, _dims(n_cuts=4096, cut_nnz=5000)], mode=2)[0] == 0
    fake = 1 << 20
    rc, L, (d, _, _) = _layout([one, one])
    args = lambda arena, size, p, mode=2: (2, d, None, None, mode, fake, fake, arena, size, p, 0.5, None)  # noqa: E731
    assert lib.gcnn_hybrid_select(*args(fake * 256, L.arena_bytes - 1, 0.1)) == -1          # arena too small
    assert lib.gcnn_hybrid_select(*args(fake * 256 + 16, L.arena_bytes, 0.1)) == -1         # arena misaligned
    assert lib.gcnn_hybrid_select(*args(fake * 256, L.arena_bytes, float("nan"))) == -1     # a threshold that is not finite
    assert lib.gcnn_hybrid_select(*args(fake * 256, L.arena_bytes, float("inf"))) == -1
    assert lib.gcnn_hybrid_select(0, d, None, None, 2, fake, fake, fake * 256, 1 << 40, 0.1, 0.5, None) == -1
    assert lib.gcnn_hybrid_select(2, d, None, None, 2, None, fake, fake * 256, L.arena_bytes, 0.1, 0.5, None) == -1
    assert lib.gcnn_hybrid_select(2, d, None, None, 2, fake, None, fake * 256, L.arena_bytes, 0.1, 0.5, None) == -1
    assert lib.gcnn_hybrid_fill_table(2, d, None, None, 2, None) == -1
    big = (_lib.HybridDims * 2)(one, many)
    assert lib.gcnn_hybrid_select(2, big, None, None, 2, fake, fake, fake * 256, 1 << 40, 0.1, 0.5, None) == -4


def test_client_half_imports_neither_torch_nor_the_binding():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gcnn_cut_selector_amd.serve as s\n"
            "import gcnn_cut_selector_amd.lpstate as l\n"
            "assert s.ScoringClient.select_cuts_hybrid and s.encode_hybrid_request and l.CutSnapshot and l.check_cut_snapshot\n"
            "assert s.KIND_HYBRID_SELECT == 6\n"
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.')]\n"
            "assert not bad, bad\n"
            "assert 'gcnn_cut_selector_amd._lib' not in sys.modules and 'gcnn_cut_selector_amd.hybrid' not in sys.modules\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_hybrid_wire_format_round_trips_bit_for_bit():
    from gcnn_cut_selector_amd import lpstate, serve, synthetic
    forced = (np.array([[0, 0, 2], [3, 1, 0]], np.int32), np.array([0.5, -0.5, 1.0], np.float32))
    snap = synthetic.make_lp_snapshot("setcov", 1, scale=0.2)
    snap.cut_val, snap.col_lp = snap.cut_val.copy(), snap.col_lp.copy()
    snap.cut_val[0], snap.col_lp[1], snap.infinity = np.nan, -0.0, 1e30
    sent, dims = lpstate.check_cut_snapshot(snap, deep=False)
    for f in (None, forced):
        message = serve.encode_hybrid_request("whatever", snap, f, 0.25, 0.75, 7)
        req = serve.decode_request(message)
        assert (req["kind"], req["p_max"], req["p_max_ub"], req["max_selected"]) == (serve.KIND_HYBRID_SELECT, 0.25, 0.75, 7)
        assert isinstance(req["snapshot"], lpstate.CutSnapshot)
        got, got_dims = lpstate.check_cut_snapshot(req["snapshot"], deep=False)
        assert got_dims == dims and len(got) == 8 and all(_same(a, b) for a, b in zip(got, sent))
        assert np.signbit(got[7][1]) and np.isnan(got[2][0]) and req["snapshot"].infinity == 1e30
        n_arrays = message[5]
        assert n_arrays == (9 if f is None else 11)
        if f is None:
            assert req["forced"] is None
        else:
            assert _same(req["forced"][0], forced[0]) and _same(req["forced"][1], forced[1]) and req["forced"][2] == 3
        head = message[:4]
        for bad in (message[:30], message[:-1], message + b"\0", head + bytes([7]) + message[5:], head + bytes([9]) + message[5:],
                    head + bytes([serve.KIND_LP_SELECT]) + message[5:], head + bytes([serve.KIND_SELECT]) + message[5:],
                    message[:5] + bytes([message[5] - 1]) + message[6:]):
            with pytest.raises(serve.ProtocolError):
                serve.decode_request(bad)
    # a full LP message relabelled as a hybrid request has 20-24 arrays: the count check refuses it as before
    lp = serve.encode_lp_request("m", serve.KIND_LP_SELECT, snap, forced)
    assert 20 <= lp[5] <= 24
    with pytest.raises(serve.ProtocolError):
        serve.decode_request(lp[:4] + bytes([serve.KIND_HYBRID_SELECT]) + lp[5:])
    # replies carry the float64 quality and the features
    q, order, index, feats = np.array([0.5, np.nan]), np.array([1, 0], np.int32), np.arange(2, dtype=np.int32), np.zeros((2, 3))
    arrays, n_kept, n_sel = serve.decode_reply(serve.encode_reply([q, order, index, feats], 2, 1))
    assert len(arrays) == 4 and _same(arrays[0], q) and _same(arrays[3], feats) and (n_kept, n_sel) == (2, 1)
    broken = synthetic.make_lp_snapshot("setcov", 1, scale=0.2)
    broken.cut_ptr = broken.cut_ptr.copy()
    broken.cut_ptr[1] = broken.cut_ptr[0]
    with pytest.raises(ValueError, match="at least one entry"):
        serve.encode_hybrid_request("m", broken)
