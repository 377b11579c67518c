"""CPU checks of the cut selection's native side: its launch names come from its own file (gcnn_select.hpp) and stay apart from
the 28 of gcnn_capi.hip, its kernels cross-compile for gfx950 without scratch, and header, library and binding agree on ABI 13."""
import os
import re

import numpy as np
import pytest

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
SELECT = os.path.join(CSRC, "gcnn_select.hpp")
SELECT_NAMES = {"k_sel_pairs", "k_sel_filter"}


def test_selection_launch_names_are_its_own():
    names = launchnames.launch_names(SELECT)
    assert names == SELECT_NAMES
    assert not names & launchnames.launch_names()
    assert len(launchnames.launch_names()) == 28


def test_selection_kernels_compile_without_scratch():
    rows = {re.sub(r"^\S*(k_sel_\w+?)\d*SelArgs.*", r"\1", k): v for k, v in buildsupport.device_build().rows.items()}
    sel = {k: v for k, v in rows.items() if k.startswith("k_sel_")}
    assert set(sel) == SELECT_NAMES, sorted(rows)
    for name, v in sel.items():
        assert v["scratch"] == 0, (name, v)
        assert v["lds"] <= 80 * 1024, (name, v)   # two blocks per CU (160 KiB of LDS)


def test_abi_13_in_header_library_and_binding():
    from gcnn_cut_selector_amd import _lib
    header = open(os.path.join(ROOT, "include", "gcnn_hip.h")).read()
    for sym in ("gcnn_select_workspace_bytes", "gcnn_select_cuts", "gcnn_infer_select_layout_for", "gcnn_infer_select"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 13 and _lib.lib().gcnn_abi_version() == 13
    src = open(os.path.join(CSRC, "gcnn_capi.hip")).read()
    assert "gcnn_abi_version(void) { return 13; }" in src


def test_workspace_and_layout_queries():
    import ctypes as C
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    assert lib.gcnn_select_workspace_bytes(4096, 3, 4096) == (4096 + 3) * 64 * 16
    d = _lib.Dims(10, 20, 30, 40, 50)
    plain, sel = _lib.InferLayout(), _lib.SelectLayout()
    assert lib.gcnn_infer_layout_for(C.byref(d), C.byref(plain)) == 0
    assert lib.gcnn_infer_select_layout_for(C.byref(d), 2, 7, C.byref(sel)) == 0
    assert list(sel.infer.in_off) == list(plain.in_off) and list(sel.infer.out_off) == list(plain.out_off)
    assert sel.forced_off[0] == plain.in_bytes and sel.forced_off[2] + 4 * 7 <= sel.infer.in_bytes
    assert sel.n_kept_off == plain.out_bytes and sel.infer.out_bytes == plain.out_bytes + 16
    assert sel.ws_off + lib.gcnn_select_workspace_bytes(30, 2, 30) <= sel.infer.arena_bytes
    d.n_cuts = 4097
    assert lib.gcnn_infer_select_layout_for(C.byref(d), 0, 0, C.byref(sel)) == -4


def test_bad_arguments_are_refused_without_a_device():
    from gcnn_cut_selector_amd import _lib, ops
    lib = _lib.lib()
    dummy = 256
    for p_max, p_ub in ((float("nan"), 0.5), (0.1, float("inf")), (float("-inf"), 0.5)):
        rc = lib.gcnn_select_cuts(dummy, dummy, dummy, dummy, None, 1, 5, 5, 10, None, None, None, None, 0, p_max, p_ub,
                                  dummy, dummy, dummy, 1 << 20, None)
        assert rc == -1
        with pytest.raises(ValueError):
            ops.check_thresholds(p_max, p_ub)
    rc = lib.gcnn_select_cuts(dummy, dummy, dummy, dummy, None, 1, 4097, 4097, 10, None, None, None, None, 0, 0.1, 0.5,
                              dummy, dummy, dummy, 1 << 30, None)
    assert rc == -4
    ops.check_thresholds(0, 0.95)


def test_pack_rows_keeps_input_order_within_a_row():
    from gcnn_cut_selector_amd import ops
    ptr, col, val = ops.pack_rows(np.array([[2, 0, 2, 0], [5, 1, 3, 1]]), np.array([1, 2, 3, 4], np.float32), 4, 6)
    assert ptr.tolist() == [0, 2, 2, 4, 4] and col.tolist() == [1, 1, 5, 3] and val.tolist() == [2, 4, 1, 3]
    with pytest.raises(ValueError):
        ops.pack_rows(np.array([[0], [6]]), np.array([1.0]), 1, 6)
