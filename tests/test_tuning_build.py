"""CPU checks of the two builds `build()` makes: the product library reads no tuning knob, the experiment build
(-DGCNN_TUNING, libgcnn_hip_tuning.so) reads every one and says so, and both carry the same C ABI.  The variant tests
(test_gpu_variants.py, test_gpu_train.py's split test) force dispatch variants through the experiment build; without it
they would compare a variant with itself.  Also checks the launch-name parser the dispatch tests rely on."""
import os
import re
import subprocess
import sys

import pytest

import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
PRODUCT = os.path.join(CSRC, "libgcnn_hip.so")
TUNING = os.path.join(CSRC, "libgcnn_hip_tuning.so")
# every knob tools/README.md documents as read by the library (GCNN_LIB and GCNN_FORCE_DP are read by Python)
DOCUMENTED = {"GCNN_ROWS_WAVES", "GCNN_SPLIT_MAX_TILES", "GCNN_WG_ROWS", "GCNN_WG_SHARE", "GCNN_WG_COST2", "GCNN_WG_COST3",
              "GCNN_WG_COST3K", "GCNN_EMB_CAP", "GCNN_SLOTS4_DEG", "GCNN_SLOTS2_DEG"}


def _knobs():
    src = open(os.path.join(CSRC, "gcnn_capi.hip")).read()
    return set(re.findall(r'GCNN_KNOB\(\s*"(GCNN_\w+)"', src))


def test_knob_list_matches_the_documented_knobs():
    assert _knobs() == DOCUMENTED


def test_product_library_contains_no_knob_name():
    data = open(PRODUCT, "rb").read()
    found = sorted(k for k in _knobs() if k.encode() in data)
    assert not found, f"the product library reads tuning knobs: {found}"
    assert b"gcnn knob " not in data


def test_tuning_library_contains_every_knob_name():
    assert os.path.exists(TUNING), f"{TUNING} missing: build() makes it"
    data = open(TUNING, "rb").read()
    missing = sorted(k for k in _knobs() if k.encode() not in data)
    assert not missing, f"the tuning library does not read {missing}"
    assert b"gcnn knob %s=%d" in data


_ABI_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
from gcnn_cut_selector_amd import _lib
h = _lib.lib()   # binds every symbol of include/gcnn_hip.h and checks the ABI version
print("LIB", _lib.LIB_PATH, "ABI", h.gcnn_abi_version())
"""


@pytest.mark.parametrize("path", [PRODUCT, TUNING], ids=["product", "tuning"])
def test_library_exports_the_header_and_abi(path):
    """Loaded through GCNN_LIB in a child process: every symbol of include/gcnn_hip.h, the binding's ABI version."""
    from gcnn_cut_selector_amd import _lib
    header = open(os.path.join(ROOT, "include", "gcnn_hip.h")).read()
    assert set(re.findall(r"\b(gcnn_[a-z0-9_]+)\s*\(", header)) == set(_lib.SIGNATURES)
    env = dict(os.environ, GCNN_LIB=path)
    r = subprocess.run([sys.executable, "-c", _ABI_SCRIPT.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"LIB {path} ABI {_lib.ABI_VERSION}" in r.stdout


def test_launch_name_parser():
    names = launchnames.launch_names()
    assert len(names) == 28 and all(n.strip() for n in names), sorted(names)
    # both sides of nested conditionals, literals with commas inside, and both launch macros
    for n in ("k_edge_fwd<count> + long segments", "k_edge_fwd<count>", "k_edge_fwd", "k_edge_bwd_send + long segments",
              "k_conv_fwd<readout, keep A>", "k_embed_fwd_split", "k_conv_bwd", "k_reduce<adam>", "k_reduce"):
        assert n in names, n
