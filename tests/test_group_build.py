"""CPU checks of the group entry points (gcnn_group_*): declared in the header, exported and bound, sized and checked on the host
without a device, launch names of their own, and group kernels that cross-compile for gfx950 without scratch."""
import ctypes as C
import os
import re

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
SYMBOLS = ("gcnn_group_table_bytes", "gcnn_group_train_step", "gcnn_group_forward")


def test_symbols_in_header_library_and_binding():
    from gcnn_cut_selector_amd import _lib
    header = buildsupport.declared_everywhere(SYMBOLS)
    assert "#define GCNN_GROUP_MAX 8" in header and _lib.GROUP_MAX == 8


def test_table_bytes():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    sizes = []
    for n in range(1, 9):
        b = C.c_size_t()
        assert lib.gcnn_group_table_bytes(n, C.byref(b)) == 0
        sizes.append(b.value)
    assert sizes[0] >= 15 * (64 + 4096 - 1024) and sizes == [sizes[0] * n for n in range(1, 9)]
    assert sizes[-1] < 8 << 20
    b = C.c_size_t()
    assert lib.gcnn_group_table_bytes(0, C.byref(b)) == -1 and lib.gcnn_group_table_bytes(9, C.byref(b)) == -1
    assert lib.gcnn_group_table_bytes(1, None) == -1


def _group_names():
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "gcnn_group.hpp")).read())
    return set(re.findall(r'"(k_[^"]*)"', src))


def test_group_launch_names_are_their_own():
    names = _group_names()
    assert len(names) >= 12 and all(n.startswith("k_group_") for n in names)
    assert not names & launchnames.launch_names()
    assert len(launchnames.launch_names()) == 28


def test_group_kernels_compile_without_scratch():
    rows = buildsupport.device_build().rows
    group = {k: v for k, v in rows.items() if "k_group_" in k}
    assert len(group) == 35, sorted(group)   # one per solo kernel variant the training step and the forward pass launch
    for name, v in group.items():
        assert v["scratch"] == 0, (name, v)
    # the solo kernels' pinned residency holds for their group counterparts
    assert rows["_Z17k_group_embed_fwdILi8EEvPK9GroupHead"]["occ"] >= 4
    assert rows["_Z13k_group_wgradPK9GroupHead"]["occ"] == 2
    assert rows["_Z14k_group_reducePK9GroupHead"]["occ"] >= 6


def test_argument_checks_need_no_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    size = C.c_size_t()
    assert lib.gcnn_group_table_bytes(2, C.byref(size)) == 0
    dims = _lib.Dims(10, 20, 30, 40, 50)
    need = lib.gcnn_workspace_floats(C.byref(dims))
    fake = 1 << 20   # never dereferenced: every refusal below happens before anything is enqueued

    def member(i, ws_floats=None, ws=None):
        g = _lib.GroupMember()
        g.dims = dims
        g.params = fake
        g.cons_feats = g.var_feats = g.cut_feats = g.targets = fake
        g.workspace = ws if ws is not None else fake * (4 + i)
        g.workspace_floats = need if ws_floats is None else ws_floats
        g.scores, g.grads, g.loss_out = fake * (16 + i), fake * (32 + i), fake * (48 + i)
        return g

    def call(ms, n=None, table=None, fn=lib.gcnn_group_train_step):
        arr = (_lib.GroupMember * len(ms))(*ms)
        return fn(len(ms) if n is None else n, arr, fake, fake, size.value if table is None else table, None)

    for fn in (lib.gcnn_group_train_step, lib.gcnn_group_forward):
        assert call([member(0)], n=0, fn=fn) == -1
        assert call([member(i) for i in range(9)], n=9, fn=fn) == -1
        assert call([member(0), member(1, ws_floats=need - 1)], fn=fn) == -2
        assert call([member(0), member(1, ws=fake * 4 + 64)], fn=fn) == -1   # workspaces overlap
        assert call([member(0), member(1)], table=size.value - 1, fn=fn) == -2
    shared_grads = [member(0), member(1)]
    shared_grads[1].grads = shared_grads[0].grads
    assert call(shared_grads) == -1
    far = [member(i) for i in range(2)]   # one member's gradients over the other's (read-only) parameters
    for i, g in enumerate(far):
        g.params, g.workspace, g.scores, g.grads, g.loss_out = [((i + 1) << 40) + (k << 36) for k in range(5)]
    assert call(far, table=size.value - 1) == -2   # (spaced apart: only the table size is wrong)
    far[1].grads = far[0].params
    assert call(far) == -1
    adam = _lib.AdamArgs(fake * 64, fake * 65, fake * 66, 1e-3, 0.9, 0.999, 1e-7)
    both = [member(0), member(1)]
    both[0].adam = both[1].adam = C.pointer(adam)            # one parameter buffer updated by two members
    assert call(both) == -1
