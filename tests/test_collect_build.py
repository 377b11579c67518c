"""CPU checks of the native side of the data collector's expert round (gcnn_lp_collect): declared, exported and bound at ABI 13; four
launch names of its own file only and no kernel of its own -- every kernel family keeps its count; a layout that is gcnn_lp_layout_for's
upload with the quality and the table added and gcnn_hybrid_layout_for's scratch, rows and workspace, piece by piece; table positions
that land inside the LP snapshot's arrays; limits and bad arguments returned without a device."""
import ctypes as C
import os
import re

import pytest

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
COLLECT = os.path.join(CSRC, "gcnn_collect.hpp")
NAMES = {"k_collect_stats", "k_collect_emit", "k_collect_pairs", "k_collect_filter"}     # the records of k_hyb_stats, k_hyb_emit, k_sel_pairs, k_hyb_filter
SYMBOLS = ("gcnn_lp_collect_layout_for", "gcnn_lp_collect")
# GCNN_HYBRID_* order -> GCNN_LP_*: cut_ptr, cut_col, cut_val, cut_lhs, cut_rhs, col_type, col_obj, col_lp
LP_ARRAY = (17, 18, 19, 20, 21, 8, 9, 13)


def al16(x):
    return (x + 15) & ~15


def test_symbols_in_header_binding_and_library_abi_13():
    header = buildsupport.declared_everywhere(SYMBOLS)
    assert "gcnn_lp_collect_layout" in header
    from gcnn_cut_selector_amd import _lib
    assert int(re.search(r"#define GCNN_LP_COLLECT_OUTPUTS (\d+)", header).group(1)) == _lib.LP_COLLECT_OUTPUTS == 14
    enum = re.search(r"enum \{ GCNN_LP_HEADER = 0,([^}]*)\}", header).group(1).replace("\n", " ").split(",")
    names = ["GCNN_LP_HEADER"] + [e.strip() for e in enum]
    assert [names[i] for i in LP_ARRAY] == ["GCNN_LP_CUT_PTR", "GCNN_LP_CUT_COL", "GCNN_LP_CUT_VAL", "GCNN_LP_CUT_LHS", "GCNN_LP_CUT_RHS",
                                            "GCNN_LP_COL_TYPE", "GCNN_LP_COL_OBJ", "GCNN_LP_COL_LP"]


def test_launch_names_are_its_own_and_it_adds_no_kernel():
    names = launchnames.launch_names(COLLECT)
    assert names == NAMES
    assert len(launchnames.launch_names()) == 28 and not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_collect.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_collect.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp", "gcnn_hybrid.hpp")
    src = re.sub(r"//[^\n]*", "", open(COLLECT).read())
    assert "__global__" not in src and "#include" not in src
    assert set(re.findall(r"hipLaunchKernelGGL\((\w+)", src)) == {"k_hyb_stats", "k_hyb_emit", "k_sel_pairs", "k_hyb_filter"}
    assert len(re.findall(r"hipMemcpyAsync", src)) == 2 and not re.search(r"hipMalloc|hipStreamSynchronize|hipDeviceSynchronize|hipEventSynchronize", src)
    build = buildsupport.device_build()
    rows = list(build.rows)
    assert not any("k_collect" in r for r in rows)
    assert sum("k_hyb_" in r for r in rows) == 3 and sum("k_lp_" in r for r in rows) == 2 and sum("k_sel_" in r for r in rows) == 2


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=40, n_cols=50, n_cuts=7, row_nnz=120, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=55,
             n_state_edges=170, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.5)
    f.update(over)
    return _lib.LpDims(**f)


def _layout(d, nf=0, nfe=0):
    from gcnn_cut_selector_amd import _lib
    L = _lib.LpCollectLayout()
    return _lib.lib().gcnn_lp_collect_layout_for(C.byref(d) if d is not None else None, nf, nfe, C.byref(L)), L


@pytest.mark.parametrize("over,forced", [(dict(), (0, 0)), (dict(), (3, 18)), (dict(n_cuts=1, cut_nnz=1), (1, 1)),
                                         (dict(n_cuts=0, cut_nnz=0), (0, 0)), (dict(n_cuts=4096, cut_nnz=50001, has_incumbent=0), (2, 5)),
                                         (dict(n_cols=70000, n_model_vars=70000), (1, 6)),
                                         (dict(n_rows=0, row_nnz=0, n_state_rows=0, n_state_edges=0), (0, 0))])
def test_layout_against_the_lp_and_the_hybrid_layout_piece_by_piece(over, forced):
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    d = _dims(**over)
    nf, nfe = forced
    rc, L = _layout(d, nf, nfe)
    assert rc == 0
    lp = _lib.LpLayout()
    assert lib.gcnn_lp_layout_for(C.byref(d), nf, nfe, C.byref(lp)) == 0
    hd = (_lib.HybridDims * 1)(_lib.HybridDims(n_cols=d.n_cols, n_cuts=d.n_cuts, cut_nnz=d.cut_nnz, reserved=0, infinity=d.infinity))
    hy = _lib.HybridLayout()
    assert lib.gcnn_hybrid_layout_for(1, hd, (C.c_int32 * 1)(nf), (C.c_int32 * 1)(nfe), _lib.HYBRID_SELECT, C.byref(hy)) == 0
    C_, V, K, E1, E2 = d.n_state_rows, d.n_cols, d.n_cuts, d.n_state_edges, d.cut_nnz
    q_bytes = al16(8 * K)
    # the upload: the LP call's, with the quality between the snapshot and the forced rows, and the table behind
    assert list(L.snap_off) == list(lp.snap_off) and L.quality_off == al16(lp.snap_bytes)
    assert L.quality_off + q_bytes <= L.forced_off[0] and [o - q_bytes for o in L.forced_off] == list(lp.forced_off)
    assert L.forced_off[2] + 4 * nfe <= L.table_off and L.table_bytes == hy.table_bytes
    assert L.in_bytes == lp.in_bytes + q_bytes + hy.table_bytes == L.table_off + L.table_bytes
    assert all(o % 16 == 0 for o in (L.quality_off, L.table_off, *L.forced_off, *L.out_off))
    # the table's eight positions land inside the LP snapshot's arrays, which do not overlap
    sizes = {17: 4 * (K + 1), 18: 4 * E2, 19: 8 * E2, 20: 8 * K, 21: 8 * K, 8: V, 9: 8 * V, 13: 8 * V}
    ends = sorted(list(lp.snap_off) + [L.quality_off])
    for pos, i in zip(L.entry_snap, LP_ARRAY):
        assert pos == lp.snap_off[i]
        nxt = min(e for e in ends if e > pos) if sizes[i] else pos
        assert pos + sizes[i] <= nxt <= L.quality_off, i
    # the download
    out = list(L.out_off)
    want = [16 * C_, 8 * E1, 4 * E1, 56 * V, 24 * K, 8 * E2, 4 * E2, 4 * K, 16, 8 * K, 24 * K, 4 * K, 16, 16]
    assert out[0] == 0 and all(out[i] + want[i] <= out[i + 1] for i in range(13)) and out[13] + 16 == L.out_bytes
    # the arena: upload | outputs | the hybrid call's rows, workspace and scratch | the LP call's scratch
    rows = list(L.rows_off)
    assert L.in_bytes <= L.out_dev_off and L.out_dev_off + L.out_bytes <= rows[0] and rows[0] + 4 * (K + 1) <= rows[1]
    assert rows[1] + 4 * E2 <= rows[2] and rows[2] + 4 * E2 <= L.ws_off
    assert [rows[1] - rows[0], rows[2] - rows[1], L.ws_off - rows[2]] == \
        [hy.rows_off[1] - hy.rows_off[0], hy.rows_off[2] - hy.rows_off[1], hy.ws_off - hy.rows_off[2]]
    assert L.ws_off + lib.gcnn_select_workspace_bytes(K, nf, K) <= L.lp_scratch_off and L.lp_scratch_off - L.ws_off == hy.scratch_off - hy.ws_off
    assert L.lp_scratch_off + lp.scratch_bytes <= L.hyb_scratch_off
    assert L.arena_bytes - L.hyb_scratch_off == hy.arena_bytes - hy.scratch_off and L.arena_bytes > L.hyb_scratch_off
    assert all(o % 256 == 0 for o in (L.out_dev_off, *rows, L.ws_off, L.lp_scratch_off, L.hyb_scratch_off, L.arena_bytes))


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    assert _layout(None)[0] == -1
    assert lib.gcnn_lp_collect_layout_for(C.byref(_dims()), 0, 0, None) == -1
    for over in (dict(n_cols=-1), dict(n_cuts=-1), dict(cut_nnz=-1), dict(n_rows=-1), dict(infinity=0.0), dict(infinity=float("nan")),
                 dict(sum_epsilon=0.0), dict(obj_norm=0.0), dict(obj_norm=float("inf")), dict(n_model_vars=0), dict(n_state_rows=81)):
        assert _layout(_dims(**over))[0] == -1, over
    assert _layout(_dims(), -1, 0)[0] == -1 and _layout(_dims(), 1, -1)[0] == -1 and _layout(_dims(), 0, 3)[0] == -1
    assert _layout(_dims(n_cuts=4096, cut_nnz=5000))[0] == 0
    assert _layout(_dims(n_cuts=4097, cut_nnz=5000))[0] == -4
    big = (1 << 24) + 1
    assert _layout(_dims(n_cols=big, n_model_vars=big))[0] == -4
    assert _layout(_dims(n_rows=big, n_state_rows=big))[0] == -4
    assert _layout(_dims(), big, big)[0] == -4
    assert _layout(_dims(n_cols=1 << 24, n_model_vars=1 << 24))[0] == 0
    fake = 1 << 20
    d = _dims()
    rc, L = _layout(d, 2, 9)
    call = lambda hin, hout, arena, size, p=0.1, ub=0.5, dims=d, nf=2, nfe=9: lib.gcnn_lp_collect(  # noqa: E731
        C.byref(dims), nf, nfe, hin, hout, arena, size, p, ub, None)
    assert call(fake, fake, fake * 256, L.arena_bytes - 1) == -1                     # arena too small
    assert call(fake, fake, fake * 256 + 16, L.arena_bytes) == -1                    # arena misaligned
    assert call(fake + 8, fake, fake * 256, L.arena_bytes) == -1                     # upload misaligned
    assert call(None, fake, fake * 256, L.arena_bytes) == -1 and call(fake, None, fake * 256, L.arena_bytes) == -1
    assert call(fake, fake, None, L.arena_bytes) == -1
    for p, ub in ((float("nan"), 0.5), (float("inf"), 0.5), (0.1, float("nan")), (0.1, float("-inf"))):
        assert call(fake, fake, fake * 256, L.arena_bytes, p, ub) == -1              # thresholds that are not finite
    assert call(fake, fake, fake * 256, 1 << 40, nf=-1) == -1
    assert call(fake, fake, fake * 256, 1 << 40, dims=_dims(n_cuts=4097, cut_nnz=5000)) == -4
    assert call(fake, fake, fake * 256, 1 << 40, dims=_dims(infinity=-1.0)) == -1
