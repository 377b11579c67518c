"""CPU checks of the removal's native side (csrc/gcnn_lpremove.hpp, csrc/k_lpremove.hpp): its three symbols are in the header, the
binding and the built library at ABI 13, its launch names are its own, its kernels cross-compile for gfx950 as wave64 code without
scratch and under 16 KiB of LDS, the layout query is self-consistent against the plain round's and the fused append's for the
dims after the edit, and every bad argument and limit is returned before anything could be enqueued."""
import ctypes as C
import os
import re

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
LPREMOVE = os.path.join(CSRC, "gcnn_lpremove.hpp")
NAMES = {"k_lpd_mark", "k_lpd_rows", "k_lpd_vars"}
SYMBOLS = ("gcnn_lp_remove_layout_for", "gcnn_lp_rows_remove", "gcnn_lp_round_remove")


def test_symbols_in_header_binding_and_library_abi_13():
    from gcnn_cut_selector_amd import _lib
    header = buildsupport.declared_everywhere(SYMBOLS)
    for struct in ("gcnn_lp_remove_dims", "gcnn_lp_remove_layout"):
        assert struct in header
    assert C.sizeof(_lib.LpRemoveDims) == 32
    assert C.sizeof(_lib.LpRemoveLayout) == 16 * C.sizeof(C.c_size_t) + C.sizeof(_lib.LpRoundLayout)
    fields = re.search(r"typedef struct gcnn_lp_remove_dims \{(.*?)\} gcnn_lp_remove_dims;", header, re.S).group(1)
    assert tuple(re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields))) == tuple(n for n, _ in _lib.LpRemoveDims._fields_)


def test_launch_names_are_its_own():
    names = launchnames.launch_names(LPREMOVE)
    assert names == NAMES
    assert not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_lpremove.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_lpremove.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp", "gcnn_lpres.hpp", "gcnn_lpappend.hpp")
    kernels = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "k_lpremove.hpp")).read())
    assert set(re.findall(r"__global__[^\n;{]*?\bvoid (\w+)\(", kernels)) == NAMES
    assert "atomicAdd(" in kernels and not re.search(r"atomic\w*\([^;]*\(\s*(float|double)\s*\*", kernels)      # integer atomics only


def test_kernels_compile_as_wave64_without_scratch():
    build = buildsupport.device_build()
    rows = {k: v for k, v in build.rows.items() if "k_lpd_" in k}
    got = {re.search(r"k_lpd_[a-z]+", k).group(0) for k in rows}
    assert got == NAMES and len(rows) == 3, sorted(rows)
    for name, v in rows.items():
        assert v["scratch"] == 0 and v["lds"] <= 16 * 1024, (name, v)
        assert build.wavefront_size(name) == 64, name


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=100, n_cols=50, n_cuts=7, row_nnz=400, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=130,
             n_state_edges=520, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.0)
    f.update(over)
    return _lib.LpDims(**f)


def _gone(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=10, row_nnz=45, n_state_rows=14, n_state_edges=60, n_lhs_rows=6, n_lhs_edges=25, res_lhs_rows=60, res_lhs_edges=250)
    f.update(over)
    return _lib.LpRemoveDims(**f)


def _block(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=4, row_nnz=20, n_state_rows=6, n_state_edges=30, n_lhs_rows=2, n_lhs_edges=10, res_lhs_rows=54, res_lhs_edges=225)
    f.update(over)
    return _lib.LpAppendDims(**f)


def test_layout_is_self_consistent():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    d, m, L = _dims(), _gone(), _lib.LpRemoveLayout()
    assert lib.gcnn_lp_remove_layout_for(C.byref(d), C.byref(m), None, 15, 2, 9, C.byref(L)) == 0
    mid = _dims(n_rows=90, row_nnz=355, n_state_rows=116, n_state_edges=460)
    R = _lib.LpRoundLayout()
    assert lib.gcnn_lp_round_layout_for(C.byref(mid), 15, 2, 9, C.byref(R)) == 0
    # the list in front, padded to 256; then exactly the plain round's upload for the dims after the edit
    assert L.list_bytes == 256 and L.block_bytes == 0 and list(L.block_off) == [0] * 5
    assert L.in_bytes == L.list_bytes + R.in_bytes
    assert list(L.round.in_off) == list(R.in_off) and list(L.round.forced_off) == list(R.forced_off)
    # the download: that call's, then the removal's four flag words
    assert list(L.round.out_off) == list(R.out_off) and L.flags_off == R.out_bytes and L.out_bytes == R.out_bytes + 16
    # the arena: the upload | the round's arena | the removal's scratch
    assert L.round_off == L.list_bytes and L.scratch_off % 256 == 0 and L.round_off + L.round.arena_bytes <= L.scratch_off
    assert L.scratch_off + L.scratch_bytes == L.arena_bytes and L.round.arena_bytes >= R.arena_bytes
    assert L.scratch_bytes >= 2 * 16 * 1 + 4 * 50 + 4 * 1 + 4 * 130        # chunk counts, removed counters, the map
    for n, pad in ((64, 256), (65, 512)):
        big = _lib.LpRemoveLayout()
        many = _gone(n_rows=n, row_nnz=300, n_state_rows=80, n_state_edges=400, n_lhs_rows=40, n_lhs_edges=200)
        assert lib.gcnn_lp_remove_layout_for(C.byref(d), C.byref(many), None, 15, -1, 0, C.byref(big)) == 0
        assert big.list_bytes == pad and big.in_bytes % 16 == 0
    # with a block: the fused append's layout for the dims after the removal, both edits' flags behind the round's download
    b, A = _block(), _lib.LpAppendLayout()
    assert lib.gcnn_lp_remove_layout_for(C.byref(d), C.byref(m), C.byref(b), 15, 2, 9, C.byref(L)) == 0
    assert lib.gcnn_lp_append_layout_for(C.byref(mid), C.byref(b), 15, 2, 9, C.byref(A)) == 0
    assert L.in_bytes == L.list_bytes + A.in_bytes and L.block_bytes == A.block_bytes
    assert [o - L.list_bytes for o in L.block_off] == list(A.block_off)
    assert list(L.round.in_off) == list(A.round.in_off) and list(L.round.out_off) == list(A.round.out_off)
    assert L.append_flags_off == A.flags_off and L.flags_off == A.out_bytes and L.out_bytes == A.out_bytes + 16
    assert L.round_off == L.list_bytes + A.round_off and L.append_scratch_off == L.list_bytes + A.scratch_off
    assert L.append_scratch_off + A.scratch_bytes <= L.scratch_off and L.scratch_off + L.scratch_bytes == L.arena_bytes
    # the scratch does not depend on the round or the block
    N = _lib.LpRemoveLayout()
    assert lib.gcnn_lp_remove_layout_for(C.byref(_dims(n_cuts=0, cut_nnz=0, has_incumbent=0)), C.byref(m), None, 0, -1, 0, C.byref(N)) == 0
    assert N.scratch_bytes == L.scratch_bytes


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    L = _lib.LpRemoveLayout()
    d, m, b = _dims(), _gone(), _block()
    P = 1 << 20
    STEP = 1 << 30                                               # far apart: no span of one fake buffer meets another's

    def ptrs(k, n):
        return [P + (k * 16 + i) * STEP for i in range(n)]

    def a_set(k):
        return _lib.LpRowsSet(*ptrs(k, 10))

    src, transit, dst = a_set(0), a_set(1), a_set(2)
    raw, out = tuple(ptrs(3, 5)), tuple(ptrs(4, 5))
    res = _lib.LpResident(*([P] * 9), _lib.Graph(P, P, P, P, P, P, 0, 0))

    def layout(dd=d, mm=m, bb=None, present=3, nf=-1, nfe=0):
        return lib.gcnn_lp_remove_layout_for(C.byref(dd), C.byref(mm), C.byref(bb) if bb else None, present, nf, nfe, C.byref(L))

    def fused(dd=d, mm=m, bb=None, present=3, nf=-1, nfe=0, raw=raw, out=out, src=src, transit=None, dst=dst, r=res, params=P, hin=P,
              hout=P, arena=P, bytes_=1 << 40, order=0, p=(0.1, 0.5)):
        ref = lambda s: C.byref(s) if s else None  # noqa: E731
        return lib.gcnn_lp_round_remove(C.byref(dd), C.byref(mm), ref(bb), present, nf, nfe, *raw, *out, ref(src), ref(transit), ref(dst), ref(r),
                                        params, hin, hout, arena, bytes_, order, *p, None)

    def alone(dd=d, mm=m, lst=P, raw=raw, out=out, src=src, dst=dst, scratch=P, bytes_=1 << 40, flags=P):
        ref = lambda s: C.byref(s) if s else None  # noqa: E731
        return lib.gcnn_lp_rows_remove(C.byref(dd), C.byref(mm), lst, *raw, *out, ref(src), ref(dst), scratch, bytes_, flags, None)

    assert layout() == 0 and layout(bb=b) == 0
    # counts that cannot be: negative, more removed than resident, lhs counts above the totals, nothing left
    for over in (dict(n_rows=0), dict(n_rows=-1), dict(row_nnz=-1), dict(n_state_rows=-1), dict(n_state_edges=-1), dict(n_lhs_rows=-1),
                 dict(n_lhs_edges=-1), dict(n_rows=101), dict(row_nnz=401), dict(n_state_rows=21), dict(n_state_rows=131),
                 dict(n_state_edges=521), dict(n_lhs_rows=11), dict(n_lhs_rows=15), dict(n_lhs_edges=46), dict(n_lhs_edges=61),
                 dict(n_state_edges=91), dict(res_lhs_rows=131), dict(res_lhs_rows=-1), dict(res_lhs_edges=521), dict(res_lhs_rows=5),
                 dict(res_lhs_edges=24), dict(res_lhs_rows=125), dict(res_lhs_edges=500),
                 dict(n_rows=100, row_nnz=400, n_state_rows=130, n_state_edges=520, n_lhs_rows=60, n_lhs_edges=250)):
        bad = _gone(**over)
        assert layout(mm=bad) == -1, over
        assert fused(mm=bad) == -1 and alone(mm=bad) == -1, over
    everything = _gone(n_rows=100, row_nnz=400, n_state_rows=130, n_state_edges=520, n_lhs_rows=60, n_lhs_edges=250)
    assert layout(mm=everything, bb=_block(res_lhs_rows=0, res_lhs_edges=0)) == 0          # every resident row, with a block behind: rows are left
    for over in (dict(n_rows=-1), dict(n_model_vars=0), dict(obj_norm=0.0), dict(infinity=0.0), dict(n_state_rows=201)):
        assert layout(dd=_dims(**over)) == -1 and fused(dd=_dims(**over)) == -1 and alone(dd=_dims(**over)) == -1, over
    # the block: its own counts, and its resident lhs counts are those after the removal
    for over in (dict(n_rows=0), dict(n_lhs_rows=5), dict(res_lhs_rows=60), dict(res_lhs_edges=250)):
        assert layout(bb=_block(**over)) == -1 and fused(bb=_block(**over), transit=transit) == -1, over
    for present in (-1, 16):
        assert layout(present=present) == -1 and fused(present=present) == -1
    assert layout(dd=_dims(has_incumbent=0), present=4) == -1 and layout(nf=1, nfe=-1) == -1
    # the round's limits, on the dims after the edit, before anything is enqueued
    many = _dims(n_cuts=4097, cut_nnz=5000)
    assert layout(dd=many) == 0 and layout(dd=many, nf=0) == -4 and layout(dd=many, bb=b, nf=0) == -4
    assert fused(dd=many, order=1) == -4 and fused(dd=many, nf=0) == -4
    assert layout(dd=_dims(n_cols=(1 << 24) + 1)) == -4
    # pointers, overlaps, the arena, the thresholds
    assert layout() == 0
    arena_bytes = L.arena_bytes
    assert fused(bytes_=arena_bytes - 1) == -1 and fused(arena=P + 128, bytes_=arena_bytes) == -1 and fused(arena=0) == -1
    assert fused(params=0) == -1 and fused(hin=0) == -1 and fused(hout=0) == -1 and fused(r=None) == -1
    assert fused(src=None) == -1 and fused(dst=None) == -1 and fused(order=2) == -1 and fused(order=-2) == -1
    assert fused(bb=b, transit=None) == -1                                                      # a block needs the transit set
    for i in (0, 1, 3):
        hole = list(raw)
        hole[i] = 0
        assert fused(raw=tuple(hole)) == -1 and fused(out=tuple(hole)) == -1 and alone(raw=tuple(hole)) == -1 and alone(out=tuple(hole)) == -1
    assert fused(nf=0, p=(float("nan"), 0.5)) == -1 and fused(nf=0, p=(0.1, float("nan"))) == -1
    hole = a_set(5)
    hole.v_ptr = None
    assert fused(dst=hole) == -1 and alone(src=hole) == -1 and fused(bb=b, transit=hole) == -1
    odd = a_set(5)
    odd.cons_feats = P + 8
    assert fused(dst=odd) == -1 and alone(dst=odd) == -1                                        # cons_feats is read as float4
    # a source set, raw buffer or transit set that overlaps a destination
    assert fused(dst=src) == -1 and alone(dst=src) == -1 and fused(out=raw) == -1 and alone(out=raw) == -1
    assert fused(bb=b, transit=src) == -1 and fused(bb=b, transit=dst) == -1 and fused(bb=b, transit=transit, dst=src) == -1
    near = a_set(6)
    near.v_oth = src.v_coef + 4 * 519                                                           # one element into the source's v_coef
    assert alone(dst=near) == -1
    assert alone(lst=0) == -1 and alone(scratch=0) == -1 and alone(scratch=P + 8) == -1 and alone(flags=0) == -1
    assert alone(bytes_=L.scratch_bytes - 1) == -2
    # (every call above is refused before the device work: none of the addresses is memory)
