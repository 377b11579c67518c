"""CPU checks of the LP-snapshot path's native side: its symbols are in the header, the binding and the built library, the ABI is
still 13, its launch names come from its own file (gcnn_lpstate.hpp) and stay apart from the 28 of gcnn_capi.hip, its kernels
cross-compile for gfx950 without scratch, and the layout queries are self-consistent."""
import ctypes as C
import os
import re

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
LPSTATE = os.path.join(CSRC, "gcnn_lpstate.hpp")
LP_NAMES = {"k_lp_stats", "k_lp_emit"}
SYMBOLS = ("gcnn_lp_layout_for", "gcnn_lp_state", "gcnn_lp_infer", "gcnn_lp_infer_select")


def test_symbols_in_header_binding_and_library_abi_13():
    from gcnn_cut_selector_amd import _lib
    header = open(os.path.join(ROOT, "include", "gcnn_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SIGNATURES
        assert getattr(_lib.lib(), sym) is not None
    assert "gcnn_lp_dims" in header and "gcnn_lp_layout" in header
    assert _lib.ABI_VERSION == 13 and _lib.lib().gcnn_abi_version() == 13
    assert int(re.search(r"#define GCNN_LP_ARRAYS (\d+)", header).group(1)) == _lib.LP_ARRAYS


def test_lp_launch_names_are_its_own():
    names = launchnames.launch_names(LPSTATE)
    assert names == LP_NAMES
    assert not names & launchnames.launch_names()
    assert len(launchnames.launch_names()) == 28
    for other in ("gcnn_select.hpp", "gcnn_ibatch.hpp", "gcnn_group.hpp"):
        assert not names & launchnames.launch_names(os.path.join(CSRC, other))


def test_lp_kernels_compile_without_scratch():
    rows = {re.sub(r"^\S*?(k_lp_[a-z]+)\d*LpArgs.*", r"\1", k): v for k, v in buildsupport.device_build().rows.items()}
    lp = {k: v for k, v in rows.items() if k.startswith("k_lp_")}
    assert set(lp) == LP_NAMES, sorted(rows)
    for name, v in lp.items():
        assert v["scratch"] == 0, (name, v)
        assert v["lds"] <= 16 * 1024, (name, v)


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=100, n_cols=50, n_cuts=7, row_nnz=400, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=130,
             n_state_edges=520, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.0)
    f.update(over)
    return _lib.LpDims(**f)


def test_layout_queries_are_self_consistent():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    d, L, S = _dims(), _lib.LpLayout(), _lib.LpLayout()
    assert lib.gcnn_lp_layout_for(C.byref(d), -1, 0, C.byref(L)) == 0 and L.call_supported == 1
    off = list(L.snap_off)
    sizes = [16, 404, 1600, 3200, 800, 800, 800, 100, 50, 400, 400, 400, 50, 400, 400, 400, 400, 32, 132, 264, 56, 56]
    assert off[0] == 0 and all(o % 16 == 0 for o in off)
    for i in range(_lib.LP_ARRAYS - 1):
        assert off[i] + sizes[i] <= off[i + 1]
    assert off[-1] + sizes[-1] <= L.snap_bytes <= L.in_bytes and L.scratch_bytes >= 16 * 100 + 40 * 7
    # the state lives where gcnn_infer keeps its uploaded arrays: the same offsets as its own layout for the state's sizes
    plain, sd = _lib.InferLayout(), _lib.Dims(130, 50, 7, 520, 33)
    assert lib.gcnn_infer_layout_for(C.byref(sd), C.byref(plain)) == 0
    assert list(L.state.in_off) == list(plain.in_off) and list(L.state.dev_off) == list(plain.dev_off)
    out = list(L.out_off)
    assert out[:3] == list(plain.out_off) and out[3:] == [out[2] + 16, out[2] + 32, out[2] + 48] and L.out_bytes >= out[5] + 4 * 7
    assert L.state.arena_bytes <= L.ws_off <= L.lp_off and L.lp_off % 256 == 0 and L.lp_off + L.in_bytes <= L.scratch_off
    assert L.scratch_off + L.scratch_bytes <= L.arena_bytes
    # with forced rows: the same snapshot offsets, the forced block behind the snapshot, a selection workspace
    assert lib.gcnn_lp_layout_for(C.byref(d), 2, 9, C.byref(S)) == 0 and S.call_supported == 1
    assert list(S.snap_off) == off and S.snap_bytes == L.snap_bytes
    f = list(S.forced_off)
    assert L.snap_bytes <= f[0] and f[0] + 12 <= f[1] and f[1] + 36 <= f[2] and f[2] + 36 <= S.in_bytes
    assert S.lp_off - S.ws_off >= lib.gcnn_select_workspace_bytes(7, 2, 7)
    # no incumbent: the primal arrays take no room
    N = _lib.LpLayout()
    assert lib.gcnn_lp_layout_for(C.byref(_dims(has_incumbent=0)), -1, 0, C.byref(N)) == 0
    assert N.snap_off[15] == N.snap_off[16] == N.snap_off[17] and N.snap_bytes == L.snap_bytes - 800


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    L = _lib.LpLayout()
    # past gcnn_infer's variable limit: the snapshot part is valid (gcnn_lp_state takes it), the single call is not offered
    big = _dims(n_cols=32769, n_model_vars=32769)
    assert lib.gcnn_lp_layout_for(C.byref(big), -1, 0, C.byref(L)) == 0 and L.call_supported == 0 and L.snap_bytes > 0
    assert lib.gcnn_lp_infer(C.byref(big), 256, 256, 256, 256, 1 << 30, 0, None) == -4
    many = _dims(n_cuts=4097, cut_nnz=5000)
    assert lib.gcnn_lp_layout_for(C.byref(many), -1, 0, C.byref(L)) == 0 and L.call_supported == 1
    assert lib.gcnn_lp_layout_for(C.byref(many), 0, 0, C.byref(L)) == 0 and L.call_supported == 0
    assert lib.gcnn_lp_infer(C.byref(many), 256, 256, 256, 256, 1 << 30, 1, None) == -4
    assert lib.gcnn_lp_infer_select(C.byref(many), 0, 0, 256, 256, 256, 256, 1 << 30, 0.1, 0.5, None) == -4
    for over in (dict(n_rows=-1), dict(n_model_vars=0), dict(obj_norm=0.0), dict(obj_norm=float("nan")), dict(infinity=0.0),
                 dict(sum_epsilon=-1.0), dict(n_state_rows=201), dict(n_state_edges=801)):
        assert lib.gcnn_lp_layout_for(C.byref(_dims(**over)), -1, 0, C.byref(L)) == -1, over
    d = _dims()
    assert lib.gcnn_lp_layout_for(C.byref(d), -1, 0, C.byref(L)) == 0
    assert lib.gcnn_lp_infer(C.byref(d), 256, 256, 256, 256, L.arena_bytes - 1, 0, None) == -1          # arena too small
    assert lib.gcnn_lp_infer(C.byref(d), 256, 256, 256, 128, L.arena_bytes, 0, None) == -1              # arena misaligned
    assert lib.gcnn_lp_infer_select(C.byref(d), 0, 0, 256, 256, 256, 256, 1 << 30, float("nan"), 0.5, None) == -1
    assert lib.gcnn_lp_infer_select(C.byref(d), -1, 0, 256, 256, 256, 256, 1 << 30, 0.1, 0.5, None) == -1
    assert lib.gcnn_lp_state(C.byref(d), 256, 256, L.scratch_bytes - 1, *([256] * 9), None) == -2
    assert lib.gcnn_lp_state(C.byref(d), 264, 256, L.scratch_bytes, *([256] * 9), None) == -1           # snapshot misaligned
