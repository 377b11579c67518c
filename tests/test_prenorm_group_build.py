"""CPU checks of PreNorm fitting with the merge on the device (gcnn_prenorm_merge, gcnn_group_prenorm_merge): declared, exported
and bound, refused on the host without a device, launch names of their own, and kernels that cross-compile for gfx950 without
scratch -- the merge with every fp32 operation rounded on its own."""
import ctypes as C
import os
import re

import pytest

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
SYMBOLS = ("gcnn_prenorm_merge", "gcnn_group_prenorm_merge")


def test_symbols_in_header_library_and_binding():
    from gcnn_cut_selector_amd import _lib
    header = buildsupport.declared_everywhere(SYMBOLS)
    for name, value in (("BYTES", _lib.PRENORM_STATE_BYTES), ("MEAN", _lib.PRENORM_STATE_MEAN), ("VAR", _lib.PRENORM_STATE_VAR)):
        assert f"#define GCNN_PRENORM_STATE_{name} {value}\n" in header
    # room for the 14 units of the widest input layer, each array 16-B aligned
    assert _lib.PRENORM_STATE_VAR - _lib.PRENORM_STATE_MEAN >= 4 * 14 and _lib.PRENORM_STATE_BYTES - _lib.PRENORM_STATE_VAR >= 4 * 14
    assert "#define GCNN_GROUP_MAX 8" in header


def _new_names():
    names = set()
    for f in ("gcnn_prenorm.hpp", "k_prenorm.hpp"):
        src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        names |= set(re.findall(r'"(k_[^"]*)"', src))
    group = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "gcnn_group.hpp")).read())
    keep = set(re.findall(r'"(k_group_[^"]*(?:keep A|stats|expand_ptr)[^"]*)"', group))
    return names, keep


def test_launch_names_are_their_own():
    solo, group = _new_names()
    assert solo == {"k_prenorm_expand_ptr", "k_prenorm_stats", "k_prenorm_stats_fold", "k_prenorm_stats_fold<merge>"}
    assert group == {"k_group_conv_fwd<proj, keep A>", "k_group_conv_fwd<readout, keep A>", "k_group_conv_fwd_split<proj, keep A>",
                     "k_group_conv_fwd_split<readout, keep A>", "k_group_expand_ptr", "k_group_stats", "k_group_stats_fold"}
    old = launchnames.launch_names()
    assert len(old) == 28 and not (solo | group) & old


@pytest.fixture(scope="module")
def device_asm():
    return buildsupport.device_build()


def test_kernels_compile_without_scratch(device_asm):
    rows = device_asm.rows
    new = {k: v for k, v in rows.items() if "k_pgroup_" in k or "k_stats_fold" in k or "k_expand_ptr" in k}
    # twins: 4 + 2 keep-A row programs, expand, stats, fold; solo: fold, expand
    assert len([k for k in new if "k_pgroup_" in k]) == 9 and len(new) == 11, sorted(new)
    for name, v in new.items():
        assert v["scratch"] == 0, (name, v)
    assert len([k for k in rows if "k_group_" in k]) == 35   # the training step's and forward pass's family is unchanged
    assert rows["_Z14k_pgroup_statsPK9GroupHead"]["occ"] == rows["_Z7k_stats8StatArgs"]["occ"]


def test_merge_rounds_every_operation(device_asm):
    """The Chan merge must round as NumPy does: no fused multiply-add outside the correctly rounded fp32 divisions (each
    v_div_scale / v_rcp / 3 v_fma + 2 v_fmac / v_div_fmas / v_div_fixup), and the three divisions of the merge are there."""
    for sym in ("_Z12k_stats_fold12StatFoldArgs", "_Z19k_pgroup_stats_foldPK9GroupHead"):
        body = device_asm.body(sym)
        fixup = len(re.findall(r"\bv_div_fixup_f32\b", body))
        fma = len(re.findall(r"\bv_fma_f32\b", body))
        fmac = len(re.findall(r"\bv_fmac_f32", body))
        assert fixup == 3 and fma == 3 * fixup and fmac == 2 * fixup, (sym, fixup, fma, fmac)
        assert not re.search(r"\bv_(mad|fma_mix|pk_fma)_f32\b", body), sym


def test_argument_checks_need_no_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    size = C.c_size_t()
    assert lib.gcnn_group_table_bytes(8, C.byref(size)) == 0
    dims = _lib.Dims(10, 20, 30, 40, 50)
    need = lib.gcnn_workspace_floats(C.byref(dims))
    fake = 1 << 20   # never dereferenced: every refusal below happens before anything is enqueued

    def member(i):
        g = _lib.GroupMember()
        g.dims = dims
        g.params = g.cons_feats = g.var_feats = g.cut_feats = fake
        g.workspace, g.workspace_floats = fake * (4 + i), need
        return g

    def call(n, layers=None, states=None, table=None):
        ms = [member(i) for i in range(n)]
        arr = (_lib.GroupMember * n)(*ms)
        lay = (C.c_int32 * n)(*(layers or [0] * n))
        st = (C.c_void_p * n)(*(states or [fake * (64 + i) for i in range(n)]))
        return lib.gcnn_group_prenorm_merge(n, arr, lay, st, fake, fake, size.value if table is None else table, None)

    assert call(0) == -1 and call(9) == -1
    assert call(2, table=1) == -2
    assert call(2, layers=[0, 11]) == -1 and call(2, layers=[-1, 0]) == -1
    assert call(2, states=[fake * 64, None]) == -1                         # a state missing
    assert call(2, states=[fake * 64, fake * 64 + 4]) == -1                 # misaligned (and overlapping)
    assert call(2, states=[fake * 64, fake * 64 + 8]) == -1                 # two states overlap
    assert call(2, states=[fake * 5 + 256, fake * 65]) == -1                # a state inside the other member's workspace
    arr = (_lib.GroupMember * 1)(member(0))
    assert lib.gcnn_group_prenorm_merge(1, arr, None, (C.c_void_p * 1)(fake * 64), fake, fake, size.value, None) == -1
    assert lib.gcnn_group_prenorm_merge(1, arr, (C.c_int32 * 1)(0), None, fake, fake, size.value, None) == -1
    g = member(0)
    for layer, state in ((11, fake * 64), (0, None), (0, fake * 64 + 4)):
        assert lib.gcnn_prenorm_merge(C.byref(dims), fake, fake, fake, fake, C.byref(g.cons_graph), C.byref(g.cut_graph),
                                      fake * 4, need, layer, state, None) == -1
    assert lib.gcnn_prenorm_merge(C.byref(dims), fake, fake, fake, fake, C.byref(g.cons_graph), C.byref(g.cut_graph),
                                  fake * 4, need - 1, 0, fake * 64, None) == -2
