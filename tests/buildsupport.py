"""The library's device code, cross-compiled once (helper for the *_build tests and test_kernel_resources.py): hipcc compiles
gcnn_capi.hip to gfx950 assembly and reports registers, occupancy, LDS and scratch per function with
-Rpass-analysis=kernel-resource-usage.  `device_build()` runs that compile once per Python process -- pytest imports this module
once per session, so every module that asks shares it -- and remembers a failure as well as a success.  Also the check that a
set of entry points is declared in the header, bound, exported and at ABI 13, and the check of where a host file is included."""
from __future__ import annotations

import atexit
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "gcnn_hip.h")
HIPCC = "/opt/rocm/bin/hipcc"

_PATTERNS = (("vgpr", r" VGPRs: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
             ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"))   # " VGPRs" with its space: "AGPRs: " must not match


def parse_resource_usage(stderr_text: str) -> dict[str, dict[str, int]]:
    """Mangled function name -> {vgpr, occ, lds, scratch} from the compiler's kernel-resource-usage remarks."""
    rows, cur = {}, None
    for line in stderr_text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
        for key, pat in _PATTERNS:
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


class DeviceBuild:
    def __init__(self, rows: dict[str, dict[str, int]], asm: str):
        self.rows, self.asm = rows, asm

    def demangled(self) -> dict[str, dict[str, int]]:
        """`rows` of the kernels (k_*), keyed by their demangled names where c++filt is there to give them."""
        rows = self.rows
        filt = shutil.which("c++filt")
        names = list(rows)
        if filt:
            dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
            rows = {d: rows[n] for n, d in zip(names, dem)}
        return {k: v for k, v in rows.items() if re.search(r"\bk_[a-z_0-9]+", k)}

    def body(self, symbol: str) -> str:
        """The function's instructions: from its label to the first end of program after it."""
        body = self.asm[self.asm.index(f"{symbol}:"):]
        return body[:body.index("s_endpgm")]

    def wavefront_size(self, symbol: str) -> int:
        meta = self.asm[self.asm.index(f".name:           {symbol}\n"):]
        return int(re.search(r"\.wavefront_size:\s+(\d+)", meta).group(1))


def _run_hipcc(out: str) -> subprocess.CompletedProcess:
    return subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "gcnn_capi.hip"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True,
                          text=True, timeout=600)


_result = None   # a DeviceBuild, or the text every caller of a failed compile fails with


def device_build() -> DeviceBuild:
    global _result
    if not os.path.exists(HIPCC):
        pytest.skip(f"the cross-compiler {HIPCC} is not installed: the gfx950 resource check cannot run here")
    if _result is None:
        tmp = tempfile.mkdtemp(prefix="gcnn_device_build_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "k.s")
        try:
            p = _run_hipcc(out)
            _result = DeviceBuild(parse_resource_usage(p.stderr), open(out).read()) if p.returncode == 0 else p.stderr[-2000:]
        except subprocess.TimeoutExpired as e:
            _result = f"{e}"
    assert isinstance(_result, DeviceBuild), _result
    return _result


HOSTSAN = os.path.join(ROOT, "tests", "hostsan")
HOSTSAN_FLAGS = ("-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined,implicit-conversion", "-Xarch_host",
                 "-fno-omit-frame-pointer", "-Xarch_host", f"-fsanitize-ignorelist={os.path.join(HOSTSAN, 'ubsan_ignorelist.txt')}")


def _run_hostsan_hipcc(out: str) -> subprocess.CompletedProcess:
    # host code alone is instrumented (-Xarch_host); the device code is compiled as always and never runs
    return subprocess.run([HIPCC, *HOSTSAN_FLAGS, f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-o", out,
                           os.path.join(HOSTSAN, "hostsan_main.hip")], capture_output=True, text=True, timeout=600)


_hostsan = None   # the program's path, or the text every caller of a failed compile fails with


def host_sanitizer_build() -> str:
    """The path of tests/hostsan's stand-alone program: gcnn_capi.hip's host code under ASan and UBSan, compiled once per Python
    process as device_build() compiles the device code -- skipped only without hipcc, a failed compile fails every caller."""
    global _hostsan
    if not os.path.exists(HIPCC):
        pytest.skip(f"the cross-compiler {HIPCC} is not installed: the sanitized host program cannot be built here")
    if _hostsan is None:
        tmp = tempfile.mkdtemp(prefix="gcnn_hostsan_build_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "hostsan")
        try:
            p = _run_hostsan_hipcc(out)
            _hostsan = out if p.returncode == 0 and os.path.exists(out) else "hostsan compile failed:\n" + p.stderr[-2000:]
        except subprocess.TimeoutExpired as e:
            _hostsan = f"hostsan compile failed: {e}"
    assert not _hostsan.startswith("hostsan compile failed"), _hostsan
    return _hostsan


def declared_everywhere(symbols) -> str:
    """Every symbol is declared in the header, has a signature in the binding and is exported by the built library, and both
    sides are at ABI 13.  Returns the header's text for the caller's own checks of it."""
    from gcnn_cut_selector_amd import _lib
    header = open(HEADER).read()
    lib = _lib.lib()
    for sym in symbols:
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert _lib.ABI_VERSION == 13 and lib.gcnn_abi_version() == 13
    return header


def included_once_after(name, *needs):
    """The host file `name` (gcnn_*.hpp) is included exactly once, from gcnn_capi.hip's list, behind every file of `needs` -- those
    whose statics it uses -- and no host file includes another host file."""
    include = re.compile(r'^[ \t]*#include "(gcnn_\w+\.hpp)"', re.M)
    order = include.findall(open(os.path.join(CSRC, "gcnn_capi.hip")).read())
    assert order.count(name) == 1 and all(order.count(n) == 1 and order.index(n) < order.index(name) for n in needs), order
    for host in sorted(os.listdir(CSRC)):
        if re.fullmatch(r"gcnn_\w+\.hpp", host):
            assert not include.findall(open(os.path.join(CSRC, host)).read()), host
