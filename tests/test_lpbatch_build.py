"""CPU checks of the batched LP-snapshot path (gcnn_lp_batch) and of the LP requests of the scoring server: declared, exported
and bound at ABI 13; launch names of its own file only; two kernels that cross-compile for gfx950 as wave64 without scratch or float
atomics inside the LDS of their solo twins; a layout that agrees with gcnn_lp_layout_for and gcnn_infer_batch_layout_for; limits
returned, not asserted; a client half that imports neither torch nor the binding; a wire format that returns a snapshot bit for bit."""
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
LPBATCH = os.path.join(CSRC, "gcnn_lpbatch.hpp")
NAMES = {"k_lpset_stats", "k_lpset_emit"}
SYMBOLS = ("gcnn_lp_batch_layout_for", "gcnn_lp_batch_fill_table", "gcnn_lp_batch")
FAMILIES = ("k_lp_", "k_ib_", "k_sel_", "k_rank", "k_group_", "k_pgroup_")      # what the older build tests count kernels by


def test_symbols_in_header_binding_and_library_abi_13():
    header = buildsupport.declared_everywhere(SYMBOLS)
    assert "gcnn_lp_batch_layout" in header


def test_launch_names_are_its_own():
    names = launchnames.launch_names(LPBATCH)
    assert names == NAMES
    assert not any(n.startswith(f) for n in names for f in FAMILIES)
    assert len(launchnames.launch_names()) == 28 and not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_lpbatch.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_lpbatch.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp", "gcnn_ibatch.hpp")


def test_kernels_compile_wave64_without_scratch_or_float_atomics():
    build = buildsupport.device_build()
    new = {k: v for k, v in build.rows.items() if "k_lpset_" in k}
    assert len(new) == 2 and all(any(n in k for k in new) for n in NAMES), sorted(new)
    solo = {n: v for k, v in build.rows.items() for n in ("k_lp_stats", "k_lp_emit") if n in k}
    assert len(solo) == 2
    for name, v in new.items():
        assert "LpArgs" not in name                                   # the argument struct has a name of its own
        twin = solo["k_lp_stats" if "stats" in name else "k_lp_emit"]
        assert v["scratch"] == 0 and v["lds"] <= 16 * 1024 and v["lds"] == twin["lds"], (name, v, twin)
        assert not re.search(r"atomic_(add|pk_add)_f(16|32|64)", build.body(name)), name
        assert build.wavefront_size(name) == 64, name


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=100, n_cols=50, n_cuts=7, row_nnz=400, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=130,
             n_state_edges=520, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.0)
    f.update(over)
    return _lib.LpDims(**f)


def _layout(dims, forced=None, mode=0):
    from gcnn_cut_selector_amd import _lib
    n = len(dims)
    d = (_lib.LpDims * max(n, 1))(*dims)
    nf = (C.c_int32 * max(n, 1))(*(f[0] for f in forced)) if forced else None
    nfe = (C.c_int32 * max(n, 1))(*(f[1] for f in forced)) if forced else None
    L = _lib.LpBatchLayout()
    return _lib.lib().gcnn_lp_batch_layout_for(n, d, nf, nfe, mode, C.byref(L)), L, (d, nf, nfe)


def test_layout_is_self_consistent():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    dims = [_dims(), _dims(n_rows=0, row_nnz=0, n_state_rows=0, n_state_edges=0), _dims(has_incumbent=0, n_cols=300, n_model_vars=300),
            _dims(n_cuts=600, cut_nnz=5000)]
    forced = [(0, 0), (2, 9), (1, 1), (0, 0)]
    n = len(dims)
    for mode in (0, 1, 2):
        rc, L, (d, nf, nfe) = _layout(dims, forced, mode)
        assert rc == 0 and L.n_snapshots == n
        # every snapshot's block: the offsets of gcnn_lp_layout_for, 16-byte aligned, one behind the other behind the tables
        end = L.table_bytes
        assert L.table_bytes % 16 == 0 and L.table_bytes >= 4 * _lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE
        for s in range(n):
            one = _lib.LpLayout()
            assert lib.gcnn_lp_layout_for(C.byref(dims[s]), -1, 0, C.byref(one)) == 0
            assert L.snap_base[s] % 16 == 0 and L.snap_base[s] >= end and all(o % 16 == 0 for o in one.snap_off)
            end = L.snap_base[s] + one.snap_bytes
        f = list(L.forced_off)
        F, FE = (3, 10) if mode == 2 else (0, 0)
        assert end <= f[0] and f[0] + 4 * (F + 1) <= f[1] and f[1] + 4 * FE <= f[2] and f[2] + 4 * FE <= L.in_bytes
        # the state region: gcnn_infer_batch's own layout for the built states' sizes
        sd = (_lib.Dims * n)(*(_lib.Dims(x.n_state_rows, x.n_cols, x.n_cuts, x.n_state_edges, x.cut_nnz) for x in dims))
        plain = _lib.IbatchLayout()
        assert lib.gcnn_infer_batch_layout_for(n, sd, nf, nfe, mode, C.byref(plain)) == 0
        assert list(L.state.in_off) == list(plain.in_off) and list(L.state.dev_off) == list(plain.dev_off)
        assert L.state.arena_bytes == plain.arena_bytes and L.state.total.n_cuts == 7 * 3 + 600
        out = list(L.out_off)
        assert out[:4] == list(plain.out_off) and out == sorted(out) and all(o % 16 == 0 for o in out)
        assert out[4] >= out[3] + 16 * n and out[5] >= out[4] + 16 * n and L.out_bytes >= out[5] + 4 * L.state.total.n_cuts
        # the arena: the union's layout | the upload | the outputs | the scratch of every snapshot
        assert plain.arena_bytes <= L.up_off and L.up_off % 256 == 0 and L.up_off + L.in_bytes <= L.out_dev_off
        assert L.out_dev_off + L.out_bytes <= L.scratch_off
        end = L.scratch_off
        for s in range(n):
            one = _lib.LpLayout()
            lib.gcnn_lp_layout_for(C.byref(dims[s]), -1, 0, C.byref(one))
            assert L.scratch_off + L.scratch_base[s] >= end
            end = L.scratch_off + L.scratch_base[s] + one.scratch_bytes
        assert end <= L.arena_bytes
        # the table: the union's table first, then block prefixes and descriptors that stay inside the arena
        table = np.full(L.table_bytes // 4, -1, np.int32)
        assert lib.gcnn_lp_batch_fill_table(n, d, nf, nfe, mode, table.ctypes.data) == 0
        ib = np.full(_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE, -1, np.int32)
        assert lib.gcnn_infer_batch_fill_table(n, sd, nf if mode == 2 else None, nfe if mode == 2 else None, ib.ctypes.data) == 0
        cols = ib.reshape(_lib.IBATCH_TABLE_COLS, -1)[:, :n + 1]
        assert np.array_equal(table[:ib.size].reshape(_lib.IBATCH_TABLE_COLS, -1)[:, :n + 1], cols)
        head = table[ib.size:ib.size + 4 + 2 * _lib.IBATCH_TABLE_STRIDE]
        chunks = lambda x: -(-x // 256)  # noqa: E731
        stats = [max(1, chunks(x.n_cols) + chunks(x.n_rows) + chunks(x.n_cuts)) for x in dims]
        emit = [chunks(x.n_rows) + chunks(x.n_cuts) + 1 for x in dims]
        assert head[0] == n
        assert head[4:4 + n + 1].tolist() == np.cumsum([0] + stats).tolist()
        assert head[4 + _lib.IBATCH_TABLE_STRIDE:][:n + 1].tolist() == np.cumsum([0] + emit).tolist()
        entry = (L.table_bytes - 4 * ib.size - 4 * head.size) // n
        assert entry % 16 == 0
        for s in range(n):
            pos = table[ib.size + head.size + s * entry // 4:][:2 * 38].view(np.int64)
            assert (pos[1:] >= 0).all() and (pos[1:] < L.arena_bytes).all() and (pos[1:22] >= L.up_off + L.snap_base[s]).all()
            assert pos[29] == L.state.in_off[2] + 16 * cols[0][s] and pos[36] == L.out_dev_off + out[5] + 4 * cols[2][s]


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    one = _dims()
    assert _layout([])[0] == -1 and _layout([one] * 65)[0] == -1 and _layout([one] * 64)[0] == 0
    assert _layout([one], mode=3)[0] == -1
    for over in (dict(n_rows=-1), dict(n_model_vars=0), dict(obj_norm=float("nan")), dict(infinity=0.0), dict(n_state_rows=201)):
        assert _layout([one, _dims(**over)])[0] == -1, over
    assert _layout([one, one], [(0, 0), (0, 3)], 2)[0] == -1                           # entries without a row
    wide = _dims(n_rows=(1 << 23) + 1, row_nnz=0, n_state_rows=(1 << 23) + 1, n_state_edges=0)
    assert _layout([wide, wide])[0] == -4                                             # more than 2^24 rows in the union
    assert _layout([one, _dims(n_cuts=0)])[0] == -4                                   # cut entries with no cut to point at
    assert _layout([one, _dims(n_cols=40000, n_model_vars=40000)])[0] == 0            # no variable limit
    assert _layout([one, _dims(n_cuts=0, cut_nnz=0), _dims(n_cuts=4097, cut_nnz=5000)], mode=1)[0] == 0
    fake = 1 << 20
    rc, L, (d, _, _) = _layout([one, one], mode=2)
    args = lambda arena, size, p: (2, d, None, None, 2, fake, fake, fake, arena, size, p, 0.5, None)  # noqa: E731
    assert lib.gcnn_lp_batch(*args(fake * 256, L.arena_bytes - 1, 0.1)) == -1             # arena too small
    assert lib.gcnn_lp_batch(*args(fake * 256 + 16, L.arena_bytes, 0.1)) == -1            # arena misaligned
    assert lib.gcnn_lp_batch(*args(fake * 256, L.arena_bytes, float("nan"))) == -1        # a threshold that is not finite
    assert lib.gcnn_lp_batch(0, d, None, None, 0, fake, fake, fake, fake * 256, 1 << 40, 0.1, 0.5, None) == -1
    assert lib.gcnn_lp_batch(2, d, None, None, 0, None, fake, fake, fake * 256, L.arena_bytes, 0.1, 0.5, None) == -1
    assert lib.gcnn_lp_batch_fill_table(2, d, None, None, 0, None) == -1


def test_client_half_imports_neither_torch_nor_the_binding():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gcnn_cut_selector_amd.serve as s\n"
            "import gcnn_cut_selector_amd.lpstate as l\n"
            "assert s.ScoringClient.score_lp and s.ScoringClient.select_cuts_lp and l.LPSnapshot and l.check_snapshot\n"
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.')]\n"
            "assert not bad, bad\n"
            "assert 'gcnn_cut_selector_amd._lib' not in sys.modules and 'gcnn_cut_selector_amd.model' not in sys.modules\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_lp_wire_format_round_trips_bit_for_bit():
    from gcnn_cut_selector_amd import lpstate, serve, synthetic
    forced = (np.array([[0, 0, 2], [3, 1, 0]], np.int32), np.array([0.5, -0.5, 1.0], np.float32))
    for incumbent in (True, False):
        snap = synthetic.make_lp_snapshot("setcov", 1, scale=0.2, incumbent=incumbent)
        snap.row_val, snap.col_redcost = snap.row_val.copy(), snap.col_redcost.copy()
        snap.row_val[0], snap.col_redcost[1], snap.n_model_vars, snap.sum_epsilon = np.nan, -0.0, 12345, 1e-7
        sent, dims = lpstate.check_snapshot(snap, deep=False)
        for kind, f in ((serve.KIND_LP_SCORE, None), (serve.KIND_LP_RANK, None), (serve.KIND_LP_SELECT, None), (serve.KIND_LP_SELECT, forced)):
            message = serve.encode_lp_request("setcov/0", kind, snap, f, 0.25, 0.75, 7)
            req = serve.decode_request(message)
            assert (req["model_key"], req["kind"], req["p_max"], req["p_max_ub"], req["max_selected"]) == ("setcov/0", kind, 0.25, 0.75, 7)
            got, got_dims = lpstate.check_snapshot(req["snapshot"], deep=False)
            assert got_dims == dims and len(got) == 21 and all(_same(a, b) for a, b in zip(got, sent))
            assert np.signbit(got[13][1]) and np.isnan(got[2][0])
            assert (req["snapshot"].col_primal is None) == (not incumbent)
            if f is None:
                assert req["forced"] is None
            else:
                assert _same(req["forced"][0], forced[0]) and _same(req["forced"][1], forced[1]) and req["forced"][2] == 3
        assert len(message) < sum(a.nbytes for a in sent) + 24 * 24 + 200              # int8 codes cross as int8
        head = message[:4]
        for bad in (message[:30], message[:-1], message + b"\0", head + bytes([9]) + message[5:], head + bytes([6]) + message[5:],
                    head + bytes([serve.KIND_SELECT]) + message[5:], message[:5] + bytes([message[5] - 1]) + message[6:]):
            with pytest.raises(serve.ProtocolError):
                serve.decode_request(bad)
    # replies carry cut_index as one more array
    scores, order, index = np.array([0.5, np.nan], np.float32), np.array([1, 0], np.int32), np.array([1, 0], np.int32)
    arrays, n_kept, n_sel = serve.decode_reply(serve.encode_reply([scores, order, index], 2, 1))
    assert len(arrays) == 3 and _same(arrays[0], scores) and _same(arrays[2], index) and (n_kept, n_sel) == (2, 1)
    # a snapshot that breaks its contract is refused in the worker, before anything is sent
    broken = synthetic.make_lp_snapshot("setcov", 1, scale=0.2)
    broken.cut_ptr = broken.cut_ptr.copy()
    broken.cut_ptr[1] = broken.cut_ptr[0]
    with pytest.raises(ValueError, match="at least one entry"):
        serve.encode_lp_request("m", serve.KIND_LP_SCORE, broken)
