"""CPU checks of the test-set ranking's native side (gcnn_rank_deviations): declared in the header, exported and bound at ABI 13, a
launch name of its own file (gcnn_rank.hpp) apart from the 28 of gcnn_capi.hip, a kernel that cross-compiles for gfx950 without
scratch and within 80 KiB of LDS, and bad arguments refused on the host."""
import os
import re

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")


def test_symbol_in_header_library_and_binding_at_abi_13():
    from gcnn_cut_selector_amd import _lib
    header = open(os.path.join(ROOT, "include", "gcnn_hip.h")).read()
    lib = _lib.lib()
    assert re.search(r"\bgcnn_rank_deviations\s*\(", header)
    assert "gcnn_rank_deviations" in _lib.SIGNATURES and hasattr(lib, "gcnn_rank_deviations")
    assert _lib.ABI_VERSION == 13 and lib.gcnn_abi_version() == 13
    assert "gcnn_abi_version(void) { return 13; }" in open(os.path.join(CSRC, "gcnn_capi.hip")).read()


def test_launch_name_is_its_own():
    names = launchnames.launch_names(os.path.join(CSRC, "gcnn_rank.hpp"))
    assert names == {"k_rank_multi"}
    assert not names & launchnames.launch_names()
    assert len(launchnames.launch_names()) == 28


def test_kernel_compiles_without_scratch_within_80k_lds():
    rows = buildsupport.device_build().rows
    hits = {k: v for k, v in rows.items() if "k_rank_multi" in k}
    assert len(hits) == 1, sorted(rows)
    (v,) = hits.values()
    assert v["scratch"] == 0, v
    assert v["lds"] <= 80 * 1024, v   # two blocks per CU (160 KiB of LDS)


def test_bad_arguments_are_refused_without_a_device():
    from gcnn_cut_selector_amd import _lib
    f = _lib.lib().gcnn_rank_deviations
    d = 256   # never dereferenced: every call below is refused before anything is enqueued
    assert f(d, 1, d, d, d, 9, d, d, 1, d, None) == -1         # n_scores > GCNN_GROUP_MAX
    assert f(d, 1, d, d, d, 1, d, d, 9, d, None) == -1         # n_perms > GCNN_GROUP_MAX
    assert f(d, 1, d, d, d, -1, d, d, 1, d, None) == -1
    assert f(d, 1, None, d, d, 1, None, None, 0, d, None) == -1   # no fp32 truth for the scores
    assert f(d, 1, d, None, d, 1, d, None, 0, d, None) == -1      # no fp64 truth for the hybrid quality
    assert f(d, 1, d, None, None, 0, None, d, 1, d, None) == -1   # ... nor for a permutation
    assert f(d, 1, d, d, None, 1, None, None, 0, d, None) == -1   # scores missing
    assert f(d, 1, d, d, None, 0, None, None, 2, d, None) == -1   # perms missing
    assert f(d, 1, d, d, None, 0, None, None, 0, d, None) == -1   # no candidate
    assert f(None, 1, d, d, d, 1, d, d, 1, d, None) == -1
    assert f(d, 1, d, d, d, 1, d, d, 1, None, None) == -1
    assert f(d, 0, d, d, d, 1, d, d, 1, d, None) == -1
