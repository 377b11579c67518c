"""CPU checks of the resident LP's native side (csrc/gcnn_lpres.hpp, csrc/k_lpres.hpp): its symbols are in the header, the binding
and the built library at ABI 13, its launch names are its own, its kernels cross-compile for gfx950 without scratch, and the two
layout queries are self-consistent and refuse what they must before anything could be enqueued."""
import ctypes as C
import os
import re

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
LPRES = os.path.join(CSRC, "gcnn_lpres.hpp")
NAMES = {"k_lpr_rows_stats", "k_lpr_rows_emit", "k_lpr_stats", "k_lpr_emit"}
SYMBOLS = ("gcnn_lp_rows_layout_for", "gcnn_lp_rows_build", "gcnn_lp_round_layout_for", "gcnn_lp_round", "gcnn_lp_round_select")


def test_symbols_in_header_binding_and_library_abi_13():
    from gcnn_cut_selector_amd import _lib
    header = buildsupport.declared_everywhere(SYMBOLS)
    for struct in ("gcnn_lp_rows_layout", "gcnn_lp_resident", "gcnn_lp_round_layout"):
        assert struct in header
    for name, value in (("GCNN_LPR_DERIVED", _lib.LPR_DERIVED), ("GCNN_LPR_ARRAYS", _lib.LPR_ARRAYS), ("GCNN_LPR_BLOCKS", _lib.LPR_BLOCKS),
                        ("GCNN_LPR_LB", _lib.LPR_LB), ("GCNN_LPR_UB", _lib.LPR_UB), ("GCNN_LPR_PRIMAL", _lib.LPR_PRIMAL),
                        ("GCNN_LPR_PRIMAL_AVG", _lib.LPR_PRIMAL_AVG)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    assert C.sizeof(_lib.LpResident) == 9 * C.sizeof(C.c_void_p) + C.sizeof(_lib.Graph)


def test_launch_names_are_its_own():
    names = launchnames.launch_names(LPRES)
    assert names == NAMES
    assert len(launchnames.launch_names()) == 28 and not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_lpres.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_lpres.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp")
    kernels = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "k_lpres.hpp")).read())
    assert set(re.findall(r"__global__[^\n;{]*?\bvoid (\w+)\(", kernels)) == NAMES


def test_kernels_compile_without_scratch():
    rows = {k: v for k, v in buildsupport.device_build().rows.items() if "k_lpr_" in k}
    got = {re.search(r"k_lpr_[a-z_]+?(?=\d*(?:6LpArgs|$))", k).group(0) for k in rows}
    assert got == NAMES and len(rows) == 4, sorted(rows)
    for name, v in rows.items():
        assert v["scratch"] == 0 and v["lds"] <= 16 * 1024, (name, v)


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=100, n_cols=50, n_cuts=7, row_nnz=400, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=130,
             n_state_edges=520, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.0)
    f.update(over)
    return _lib.LpDims(**f)


def test_layout_queries_are_self_consistent():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    R = _lib.LpRowsLayout()
    assert lib.gcnn_lp_rows_layout_for(C.byref(_dims()), C.byref(R)) == 0
    off, sizes = list(R.off), [16 * 130, 8 * 520, 4 * 520, 8 * 100, 8 * 100, 16, 16 * 100]
    assert off[0] == 0 and all(o % 256 == 0 for o in off)
    for i in range(_lib.LPR_DERIVED):
        assert off[i] + sizes[i] <= (off[i + 1] if i + 1 < _lib.LPR_DERIVED else R.bytes)
    # the cut fields do not matter to the rows' layout
    R2 = _lib.LpRowsLayout()
    assert lib.gcnn_lp_rows_layout_for(C.byref(_dims(n_cuts=0, cut_nnz=0, has_incumbent=0)), C.byref(R2)) == 0
    assert list(R2.off) == off and R2.bytes == R.bytes
    # a round: present arrays take their room, absent ones none; the forced block closes the upload
    d, L = _dims(), _lib.LpRoundLayout()
    assert lib.gcnn_lp_round_layout_for(C.byref(d), 15, -1, 0, C.byref(L)) == 0
    sizes = [16, 800, 100, 50, 400, 400, 400, 400, 400, 400, 32, 132, 264, 56, 56]
    off = list(L.in_off)
    assert off[0] == 0 and all(o % 16 == 0 for o in off)
    for i in range(_lib.LPR_ARRAYS - 1):
        assert off[i] + sizes[i] <= off[i + 1]
    assert off[-1] + sizes[-1] <= L.forced_off[0] <= L.in_bytes
    out = list(L.out_off)
    assert out == [0, 32, 64, 80, 96, 112] and L.out_bytes >= out[5] + 28
    dev = list(L.dev_off)
    need = [L.in_bytes, 56 * 50, 24 * 7, 8 * 33, 4 * 33, 32, L.out_bytes, 4 * lib.gcnn_workspace_floats(C.byref(_lib.Dims(130, 50, 7, 520, 33))),
            16, 40 * 7, 0]
    assert dev[0] == 0 and all(o % 256 == 0 for o in dev)
    for i in range(_lib.LPR_BLOCKS):
        assert dev[i] + need[i] <= (dev[i + 1] if i + 1 < _lib.LPR_BLOCKS else L.arena_bytes), i
    S = _lib.LpRoundLayout()
    assert lib.gcnn_lp_round_layout_for(C.byref(d), 15, 2, 9, C.byref(S)) == 0
    assert list(S.in_off) == off and list(S.out_off) == out
    f = list(S.forced_off)
    assert f[0] + 12 <= f[1] and f[1] + 36 <= f[2] and f[2] + 36 <= S.in_bytes
    assert S.arena_bytes - S.dev_off[10] >= lib.gcnn_select_workspace_bytes(7, 2, 7)
    N = _lib.LpRoundLayout()
    assert lib.gcnn_lp_round_layout_for(C.byref(d), 5, -1, 0, C.byref(N)) == 0           # col_ub and col_primal_avg stay away
    assert N.in_off[7] == N.in_off[8] and N.in_off[9] == N.in_off[10] and N.in_bytes == L.in_bytes - 800
    # the upload against the full snapshot's: the resident arrays are gone
    full = _lib.LpLayout()
    assert lib.gcnn_lp_layout_for(C.byref(d), 2, 9, C.byref(full)) == 0
    resident = 404 + 1600 + 3200 + 800 + 800 + 50 + 400
    assert S.in_bytes <= full.in_bytes - resident + 256


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    L, R = _lib.LpRoundLayout(), _lib.LpRowsLayout()
    res = _lib.LpResident(*([256] * 9), _lib.Graph(256, 256, 256, 256, 256, 256, 0, 0))
    big = _dims(n_cols=33000, n_model_vars=33000)                                        # no variable limit
    assert lib.gcnn_lp_round_layout_for(C.byref(big), 3, -1, 0, C.byref(L)) == 0 and L.arena_bytes > 0
    many = _dims(n_cuts=4097, cut_nnz=5000)
    assert lib.gcnn_lp_round_layout_for(C.byref(many), 3, -1, 0, C.byref(L)) == 0
    assert lib.gcnn_lp_round_layout_for(C.byref(many), 3, 0, 0, C.byref(L)) == -4
    assert lib.gcnn_lp_round(C.byref(many), 3, C.byref(res), 256, 256, 256, 256, 1 << 40, 1, None) == -4
    assert lib.gcnn_lp_round_select(C.byref(many), 3, 0, 0, C.byref(res), 256, 256, 256, 256, 1 << 40, 0.1, 0.5, None) == -4
    assert lib.gcnn_lp_round_layout_for(C.byref(_dims(n_cols=(1 << 24) + 1)), 3, -1, 0, C.byref(L)) == -4
    for over in (dict(n_rows=-1), dict(n_model_vars=0), dict(obj_norm=0.0), dict(obj_norm=float("nan")), dict(infinity=0.0),
                 dict(sum_epsilon=-1.0), dict(n_state_rows=201), dict(n_state_edges=801)):
        assert lib.gcnn_lp_round_layout_for(C.byref(_dims(**over)), 3, -1, 0, C.byref(L)) == -1, over
        assert lib.gcnn_lp_rows_layout_for(C.byref(_dims(**over)), C.byref(R)) == -1, over
    d = _dims()
    for present in (-1, 16):
        assert lib.gcnn_lp_round_layout_for(C.byref(d), present, -1, 0, C.byref(L)) == -1
    assert lib.gcnn_lp_round_layout_for(C.byref(_dims(has_incumbent=0)), 4, -1, 0, C.byref(L)) == -1      # primal without an incumbent
    assert lib.gcnn_lp_round_layout_for(C.byref(d), 3, 1, -1, C.byref(L)) == -1
    assert lib.gcnn_lp_round_layout_for(C.byref(d), 3, -1, 0, C.byref(L)) == 0
    A = L.arena_bytes
    assert lib.gcnn_lp_round(C.byref(d), 3, C.byref(res), 256, 256, 256, 256, A - 1, 0, None) == -1      # arena too small
    assert lib.gcnn_lp_round(C.byref(d), 3, C.byref(res), 256, 256, 256, 128, A, 0, None) == -1          # arena misaligned
    assert lib.gcnn_lp_round(C.byref(d), 3, C.byref(res), 0, 256, 256, 256, A, 0, None) == -1            # no parameters
    assert lib.gcnn_lp_round(C.byref(d), 3, None, 256, 256, 256, 256, A, 0, None) == -1                   # no resident block
    assert lib.gcnn_lp_round(C.byref(d), 3, C.byref(res), 256, 256, 256, 256, A, 2, None) == -1          # want_order outside -1..1
    hole = _lib.LpResident(*([256] * 9), _lib.Graph(256, 256, 256, 256, 256, 256, 0, 0))
    hole.row_place = None
    assert lib.gcnn_lp_round(C.byref(d), 3, C.byref(hole), 256, 256, 256, 256, A, 0, None) == -1
    assert lib.gcnn_lp_round_select(C.byref(d), 3, 0, 0, C.byref(res), 256, 256, 256, 256, 1 << 40, float("nan"), 0.5, None) == -1
    assert lib.gcnn_lp_round_select(C.byref(d), 3, -1, 0, C.byref(res), 256, 256, 256, 256, 1 << 40, 0.1, 0.5, None) == -1
    assert lib.gcnn_lp_round(C.byref(_dims(n_state_rows=0, n_state_edges=5)), 3, C.byref(res), 256, 256, 256, 256, 1 << 40, 0, None) == -1
    assert lib.gcnn_lp_rows_layout_for(C.byref(d), C.byref(R)) == 0
    assert lib.gcnn_lp_rows_build(C.byref(d), 256, 256, 256, 256, 256, 256, 256, R.bytes - 1, None) == -2
    assert lib.gcnn_lp_rows_build(C.byref(d), 256, 256, 256, 256, 256, 256, 128, R.bytes, None) == -1    # derived misaligned
    assert lib.gcnn_lp_rows_build(C.byref(d), 256, 0, 256, 256, 256, 256, 256, R.bytes, None) == -1      # entries without columns
