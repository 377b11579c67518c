"""CPU checks of tests/buildsupport.py itself, without a compiler: the remark parser, the two readers of the assembly text, and
that one compile -- a failed one as well -- serves every caller."""
import subprocess
import sys

import pytest

import buildsupport

REMARKS = """\
k_rows.hpp:10:1: remark: Function Name: _Z5k_onePf [-Rpass-analysis=kernel-resource-usage]
k_rows.hpp:10:1: remark:     SGPRs: 24 [-Rpass-analysis=kernel-resource-usage]
k_rows.hpp:10:1: remark:     VGPRs: 37 [-Rpass-analysis=kernel-resource-usage]
k_rows.hpp:10:1: remark:     AGPRs: 8 [-Rpass-analysis=kernel-resource-usage]
k_rows.hpp:10:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
k_rows.hpp:10:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
k_rows.hpp:10:1: remark:     LDS Size [bytes/block]: 4096 [-Rpass-analysis=kernel-resource-usage]
k_edge.hpp:20:1: remark: Function Name: _Z5k_twoPf [-Rpass-analysis=kernel-resource-usage]
k_edge.hpp:20:1: remark:     SGPRs: 96 [-Rpass-analysis=kernel-resource-usage]
k_edge.hpp:20:1: remark:     VGPRs: 256 [-Rpass-analysis=kernel-resource-usage]
k_edge.hpp:20:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
k_edge.hpp:20:1: remark:     ScratchSize [bytes/lane]: 1208 [-Rpass-analysis=kernel-resource-usage]
k_edge.hpp:20:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]
k_edge.hpp:20:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""

ASM = """\
_Z5k_onePf:
\tv_fma_f32 v0, v1, v2, v3
\ts_endpgm
_Z5k_twoPf:
\tv_add_f32 v0, v1, v2
\ts_endpgm
amdhsa.kernels:
  - .name:           _Z5k_onePf
    .wavefront_size: 64
  - .name:           _Z5k_twoPf
    .wavefront_size: 32
"""


def test_parse_resource_usage():
    rows = buildsupport.parse_resource_usage(REMARKS)
    assert rows == {"_Z5k_onePf": {"vgpr": 37, "occ": 8, "lds": 4096, "scratch": 0},
                    "_Z5k_twoPf": {"vgpr": 256, "occ": 2, "lds": 0, "scratch": 1208}}


def test_body_and_wavefront_size():
    build = buildsupport.DeviceBuild({}, ASM)
    assert build.body("_Z5k_onePf") == "_Z5k_onePf:\n\tv_fma_f32 v0, v1, v2, v3\n\t"
    assert "v_add_f32" in build.body("_Z5k_twoPf") and "v_fma_f32" not in build.body("_Z5k_twoPf")
    assert (build.wavefront_size("_Z5k_onePf"), build.wavefront_size("_Z5k_twoPf")) == (64, 32)
    with pytest.raises(ValueError):
        build.body("_Z7k_threePf")


def _fake_compiler(monkeypatch, returncode, stderr):
    calls = []

    def run(out):
        calls.append(out)
        open(out, "w").write(ASM)
        return subprocess.CompletedProcess([], returncode, "", stderr)

    monkeypatch.setattr(buildsupport, "HIPCC", sys.executable)   # any file that exists: no skip where hipcc is missing
    monkeypatch.setattr(buildsupport, "_run_hipcc", run)
    monkeypatch.setattr(buildsupport, "_result", None)           # the session's real build comes back afterwards
    return calls


def test_one_compile_serves_every_caller(monkeypatch):
    calls = _fake_compiler(monkeypatch, 0, REMARKS)
    first = buildsupport.device_build()
    assert buildsupport.device_build() is first and len(calls) == 1
    assert first.rows["_Z5k_twoPf"]["scratch"] == 1208 and first.asm == ASM


def test_a_failed_compile_is_remembered(monkeypatch):
    calls = _fake_compiler(monkeypatch, 1, "gcnn_capi.hip:1:1: error: expected unqualified-id")
    for _ in range(2):
        with pytest.raises(AssertionError, match="expected unqualified-id"):
            buildsupport.device_build()
    assert len(calls) == 1


def _fake_host_compiler(monkeypatch, returncode, stderr):
    calls = []

    def run(out):
        calls.append(out)
        if returncode == 0:
            open(out, "w").write("#!/bin/sh\n")
        return subprocess.CompletedProcess([], returncode, "", stderr)

    monkeypatch.setattr(buildsupport, "HIPCC", sys.executable)
    monkeypatch.setattr(buildsupport, "_run_hostsan_hipcc", run)
    monkeypatch.setattr(buildsupport, "_hostsan", None)          # the session's real program comes back afterwards
    return calls


def test_one_sanitizer_compile_serves_every_caller(monkeypatch):
    calls = _fake_host_compiler(monkeypatch, 0, "")
    first = buildsupport.host_sanitizer_build()
    assert buildsupport.host_sanitizer_build() == first == calls[0] and len(calls) == 1


def test_a_failed_sanitizer_compile_is_remembered(monkeypatch):
    calls = _fake_host_compiler(monkeypatch, 1, "hostsan_main.hip:1:1: error: expected unqualified-id")
    for _ in range(2):
        with pytest.raises(AssertionError, match="expected unqualified-id"):
            buildsupport.host_sanitizer_build()
    assert len(calls) == 1


def test_the_sanitizer_build_instruments_host_code_only():
    flags = buildsupport.HOSTSAN_FLAGS
    at = [i for i, f in enumerate(flags) if f.startswith("-fsanitize") or f == "-fno-omit-frame-pointer"]
    assert len(at) == 3 and all(flags[i - 1] == "-Xarch_host" for i in at)
    assert [f for f in flags if f.startswith("--offload-arch")] == ["--offload-arch=gfx950"]     # the plain target, no feature suffix
