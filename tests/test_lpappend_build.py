"""CPU checks of the incremental append's native side (csrc/gcnn_lpappend.hpp, csrc/k_lpappend.hpp): its three symbols are in the
header, the binding and the built library at ABI 13, its launch names are its own, its kernels cross-compile for gfx950 without
scratch and under 16 KiB of LDS, the layout query is self-consistent, and every bad argument and limit is returned before
anything could be enqueued."""
import ctypes as C
import os
import re

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
LPAPPEND = os.path.join(CSRC, "gcnn_lpappend.hpp")
NAMES = {"k_lpa_stats", "k_lpa_scan", "k_lpa_move", "k_lpa_order"}
SYMBOLS = ("gcnn_lp_append_layout_for", "gcnn_lp_rows_append", "gcnn_lp_round_append")


def test_symbols_in_header_binding_and_library_abi_13():
    from gcnn_cut_selector_amd import _lib
    header = buildsupport.declared_everywhere(SYMBOLS)
    for struct in ("gcnn_lp_append_dims", "gcnn_lp_rows_set", "gcnn_lp_append_layout"):
        assert struct in header
    assert C.sizeof(_lib.LpAppendDims) == 32 and C.sizeof(_lib.LpRowsSet) == 10 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.LpAppendLayout) == 13 * C.sizeof(C.c_size_t) + C.sizeof(_lib.LpRoundLayout)
    fields = re.search(r"typedef struct gcnn_lp_rows_set \{(.*?)\} gcnn_lp_rows_set;", header, re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields))) == _lib.LP_SET_FIELDS


def test_launch_names_are_its_own():
    names = launchnames.launch_names(LPAPPEND)
    assert names == NAMES
    assert not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_lpappend.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_lpappend.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp", "gcnn_lpres.hpp")
    kernels = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "k_lpappend.hpp")).read())
    assert set(re.findall(r"__global__[^\n;{]*?\bvoid (\w+)\(", kernels)) == NAMES
    assert not [n for n in NAMES if "k_lpr_" in n or "k_lp_" in n]


def test_kernels_compile_without_scratch():
    rows = {k: v for k, v in buildsupport.device_build().rows.items() if "k_lpa_" in k}
    got = {re.search(r"k_lpa_[a-z]+", k).group(0) for k in rows}
    assert got == NAMES and len(rows) == 4, sorted(rows)
    for name, v in rows.items():
        assert v["scratch"] == 0 and v["lds"] <= 16 * 1024, (name, v)


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=100, n_cols=50, n_cuts=7, row_nnz=400, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=130,
             n_state_edges=520, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.0)
    f.update(over)
    return _lib.LpDims(**f)


def _block(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=10, row_nnz=45, n_state_rows=14, n_state_edges=60, n_lhs_rows=6, n_lhs_edges=25, res_lhs_rows=60, res_lhs_edges=250)
    f.update(over)
    return _lib.LpAppendDims(**f)


def test_layout_is_self_consistent():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    d, b, L = _dims(), _block(), _lib.LpAppendLayout()
    assert lib.gcnn_lp_append_layout_for(C.byref(d), C.byref(b), 15, 2, 9, C.byref(L)) == 0
    after = _dims(n_rows=110, row_nnz=445, n_state_rows=144, n_state_edges=580)
    R = _lib.LpRoundLayout()
    assert lib.gcnn_lp_round_layout_for(C.byref(after), 15, 2, 9, C.byref(R)) == 0
    # the block: five arrays side by side inside block_bytes, which is a multiple of 256 and at most 256 more than they need
    sizes = [44, 180, 360, 80, 80]
    spans = sorted((L.block_off[i], L.block_off[i] + sizes[i]) for i in range(5))
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= L.block_bytes
    assert L.block_bytes % 256 == 0 and L.block_bytes < sum(sizes) + 256
    assert all(L.block_off[i] % 8 == 0 for i in (2, 3, 4)) and all(L.block_off[i] % 4 == 0 for i in (0, 1))
    # the round behind it is gcnn_lp_round_layout_for's for the dims after the append, with the append's flags closing the download
    assert L.in_bytes == L.block_bytes + R.in_bytes
    assert list(L.round.in_off) == list(R.in_off) and list(L.round.forced_off) == list(R.forced_off)
    assert list(L.round.out_off) == list(R.out_off) and L.flags_off == R.out_bytes and L.out_bytes == R.out_bytes + 16
    assert L.round_off == L.block_bytes and L.round_off % 256 == 0 and L.scratch_off % 256 == 0
    assert L.round_off + L.round.arena_bytes <= L.scratch_off and L.scratch_off + L.scratch_bytes == L.arena_bytes
    assert L.round.arena_bytes >= R.arena_bytes
    need = 16 * 10 + 16 + 4 + 8 * 50 + 4 + 4 * 50 + 8 * 45 + 2 * 4 * 60
    assert L.scratch_bytes >= need
    # the scratch does not depend on the round
    N = _lib.LpAppendLayout()
    assert lib.gcnn_lp_append_layout_for(C.byref(_dims(n_cuts=0, cut_nnz=0, has_incumbent=0)), C.byref(b), 0, -1, 0, C.byref(N)) == 0
    assert N.scratch_bytes == L.scratch_bytes and N.block_bytes == L.block_bytes


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    L = _lib.LpAppendLayout()
    d, b = _dims(), _block()
    P = 256
    sets = _lib.LpRowsSet(*([P] * 10))
    res = _lib.LpResident(*([P] * 9), _lib.Graph(P, P, P, P, P, P, 0, 0))

    def layout(dd=d, bb=b, present=3, nf=-1, nfe=0):
        return lib.gcnn_lp_append_layout_for(C.byref(dd), C.byref(bb), present, nf, nfe, C.byref(L))

    def fused(dd=d, bb=b, present=3, nf=-1, nfe=0, raw=(P,) * 5, src=sets, dst=sets, r=res, params=P, hin=P, hout=P, arena=P,
              bytes_=1 << 40, order=0, p=(0.1, 0.5)):
        return lib.gcnn_lp_round_append(C.byref(dd), C.byref(bb), present, nf, nfe, *raw, C.byref(src) if src else None,
                                        C.byref(dst) if dst else None, C.byref(r) if r else None, params, hin, hout, arena, bytes_, order,
                                        *p, None)

    def alone(dd=d, bb=b, raw=(P,) * 5, obj=P, src=sets, dst=sets, scratch=P, bytes_=1 << 40, flags=P):
        return lib.gcnn_lp_rows_append(C.byref(dd), C.byref(bb), *raw, obj, C.byref(src) if src else None, C.byref(dst) if dst else None,
                                       scratch, bytes_, flags, None)

    assert layout() == 0
    # the block's counts
    for over in (dict(n_rows=0), dict(n_rows=-1), dict(row_nnz=-1), dict(n_state_rows=21), dict(n_lhs_rows=11), dict(n_lhs_rows=15),
                 dict(n_lhs_edges=46), dict(n_state_edges=91), dict(n_lhs_edges=61), dict(res_lhs_rows=131), dict(res_lhs_rows=-1),
                 dict(res_lhs_edges=521), dict(n_state_rows=-1)):
        bad = _block(**over)
        assert layout(bb=bad) == -1, over
        assert fused(bb=bad) == -1 and alone(bb=bad) == -1, over
    for over in (dict(n_rows=-1), dict(n_model_vars=0), dict(obj_norm=0.0), dict(infinity=0.0), dict(n_state_rows=201)):
        assert layout(dd=_dims(**over)) == -1 and fused(dd=_dims(**over)) == -1 and alone(dd=_dims(**over)) == -1, over
    assert layout(dd=_dims(row_nnz=2 ** 31 - 40, n_state_edges=600)) == -1                       # the entries after the append leave int32
    for present in (-1, 16):
        assert layout(present=present) == -1 and fused(present=present) == -1
    assert layout(dd=_dims(has_incumbent=0), present=4) == -1
    assert layout(nf=1, nfe=-1) == -1
    # the round's limits, on the dims after the append, before anything is enqueued
    many = _dims(n_cuts=4097, cut_nnz=5000)
    assert layout(dd=many) == 0 and layout(dd=many, nf=0) == -4
    assert fused(dd=many, order=1) == -4 and fused(dd=many, nf=0) == -4 and fused(dd=many, order=0) != -4
    assert layout(dd=_dims(n_cols=(1 << 24) + 1)) == -4
    edge = _dims(n_rows=(1 << 24), n_state_rows=(1 << 24) - 5, row_nnz=1 << 25, n_state_edges=1 << 25)
    assert layout(dd=edge) == -4 and fused(dd=edge) == -4 and alone(dd=edge) == -4            # 2^24 state rows are passed by the block
    # pointers, the arena, the thresholds
    assert layout() == 0
    A = L.arena_bytes
    assert fused(bytes_=A - 1) == -1 and fused(arena=128, bytes_=A) == -1 and fused(arena=0) == -1
    assert fused(params=0) == -1 and fused(hin=0) == -1 and fused(hout=0) == -1 and fused(r=None) == -1
    assert fused(src=None) == -1 and fused(dst=None) == -1 and fused(order=2) == -1 and fused(order=-2) == -1
    assert fused(raw=(0, P, P, P, P)) == -1 and fused(raw=(P, 0, P, P, P)) == -1 and fused(raw=(P, P, P, 0, P)) == -1
    assert fused(nf=0, p=(float("nan"), 0.5)) == -1
    hole = _lib.LpRowsSet(*([P] * 10))
    hole.v_ptr = None
    assert fused(dst=hole) == -1 and alone(src=hole) == -1
    odd = _lib.LpRowsSet(*([P] * 10))
    odd.cons_feats = 8
    assert fused(dst=odd) == -1 and alone(dst=odd) == -1                                        # cons_feats is read as float4
    no_place = _lib.LpResident(*([P] * 9), _lib.Graph(P, P, P, P, P, P, 0, 0))
    no_place.row_place = None
    assert fused(r=no_place) == -1
    assert alone(scratch=0) == -1 and alone(scratch=8) == -1 and alone(flags=0) == -1 and alone(obj=0) == -1
    assert alone(bytes_=L.scratch_bytes - 1) == -2 and alone(raw=(P, P, 0, P, P)) == -1
