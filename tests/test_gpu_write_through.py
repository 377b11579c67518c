"""Write-through result stores (store16<ST_WT>, gcnn_common.hpp) write exactly what plain stores write.

The 4- and 8-wave row programs of a training step store their result tensors with 16-byte sc1 (write-through) vector stores while
the launch's largest row set has at most GCNN_WT_MAX_ROWS (32,768) rows (k_*_wt, k_rows.hpp; rows_write_through, gcnn_capi.hip).  Parity over
repeated steps cannot see a store that is silently dropped or lands in the wrong place: the workspace still holds the previous
step's rows.  So here every step starts from a workspace filled with a NaN bit pattern, with 16 guard rows behind its end, and
runs twice in child processes (a process loads one library): through the product library and through libgcnn_hip_plain.so, the
same sources with -DGCNN_STORE_PLAIN (every write-through store as a plain one; `build()` makes it beside the product).

The row programs have no per-op wrapper in ops.py (its linear_* wrappers run k_linear.hpp), so each case is one `train_step`
on a synthetic state whose three row sets (constraints, variables, cuts) have the row counts under test:
  1 (one partial tile), 16 (one exact tile), 17 (one row past a tile), 4097 (257 tiles: the first size past the 256-tile split
  threshold, so the write-through 4- and 8-wave programs run; the smaller sets take the four-waves-per-tile programs, which store
  plain in both builds, beside them).
What is compared, per case:
  * the whole workspace, word for word: a row the write-through build did not write still carries the pattern where the plain
    build has a value, a stray store shows where the plain build has the pattern -- either is a difference;
  * no pattern word in loss, scores or gradients, and all three equal to the plain build's bits;
  * the plain build wrote at least the [n, 64] result tensors the row programs are known to store (so the comparison is not
    between two workspaces nobody wrote), and the guard rows behind the workspace still carry the pattern in both.
And one workspace, two different batches back to back: the second batch's results equal those of a fresh model and workspace.

Without a GPU: the compiled write-through kernels carry the sc1 vector stores (and only the 16-byte form) and keep the pinned
residency of their plain twins; no other kernel carries one."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import buildsupport
from gpucommon import GUARD, PATTERN, make_state, run_step  # noqa: F401  (the child scripts reach them as T.*)

ROOT = buildsupport.ROOT
PRODUCT_LIB = os.path.join(buildsupport.CSRC, "libgcnn_hip.so")
PLAIN_LIB = os.path.join(buildsupport.CSRC, "libgcnn_hip_plain.so")
ROW_COUNTS = (1, 16, 17, 4097)
# (constraints, variables, cuts)
CASES = [(n, n, n) for n in ROW_COUNTS] + [(4097, 17, 1), (16, 4097, 17), (1, 16, 4097)]
PAIR = ((4097, 17, 16), (17, 4097, 1))   # two batches through one workspace
# [n, 64] fp32 tensors a training step certainly stores per row of a row set, read off k_rows.hpp: the embedding X with its
# projections (constraints 2, variables 3, cuts 2) and the convolution's output X' on its receiver set -- a lower bound (Z1, the
# tails, the gradients and the edge passes write more)
MIN_TENSORS = {"cons": 2 + 1, "vars": 3 + 1, "cuts": 2 + 1}


def case_id(c):
    return "x".join(map(str, c))


CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import hashlib
import numpy as np, torch
from gcnn_cut_selector_amd import _lib
import test_gpu_write_through as T
from gpucommon import make_model
assert _lib.LIB_PATH == {lib!r}, _lib.LIB_PATH
dev = torch.device("cuda", 0)
out = {{}}
m, _ = make_model(21, dev)
for i, c in enumerate(T.CASES):
    state, y = T.make_state(*c, seed=100 + i)
    res, w, need, _ = T.run_step(m, state, y)
    k = T.case_id(c)
    for name, v in res.items():
        out[k + "/" + name] = v
    out[k + "/need"] = np.int64(need)
    out[k + "/pattern"] = np.packbits(w == T.PATTERN)
    out[k + "/sha"] = np.frombuffer(hashlib.sha256(w.tobytes()).digest(), np.uint8)
# two different batches back to back through ONE workspace, then the second through a fresh model and workspace
(s1, y1), (s2, y2) = (T.make_state(*c, seed=200 + i) for i, c in enumerate(T.PAIR))
_, _, need2, _ = T.run_step(m, s2, y2)
_, _, _, ws = T.run_step(m, s1, y1, floats=need2)
res, _, _, _ = T.run_step(m, s2, y2, ws=ws)
fresh, _ = make_model(21, dev)
ref, _, _, _ = T.run_step(fresh, s2, y2)
for name in res:
    out["pair/" + name] = res[name]; out["fresh/" + name] = ref[name]
np.savez({out!r}, **out)
print("CHILD OK")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{"wt": ..., "plain": ...}: the child's arrays for the product library and for the plain-store build, one child at a time."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert os.path.exists(PLAIN_LIB), "build() makes libgcnn_hip_plain.so"
    tmp = tmp_path_factory.mktemp("write_through")
    tests = os.path.dirname(os.path.abspath(__file__))
    out = {}
    for tag, lib in (("plain", PLAIN_LIB), ("wt", PRODUCT_LIB)):
        path = str(tmp / f"{tag}.npz")
        script = CHILD.format(root=ROOT, tests=tests, lib=lib, out=path)
        r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, GCNN_LIB=lib), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, f"{tag}: exit {r.returncode}\n{r.stderr[-3000:]}"
        with np.load(path) as z:
            out[tag] = {k: z[k] for k in z.files}
    return out


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_step_writes_what_the_plain_build_writes(runs, case):
    k, wt, plain = case_id(case), runs["wt"], runs["plain"]
    need = int(plain[k + "/need"])
    assert int(wt[k + "/need"]) == need
    pat_wt = np.unpackbits(wt[k + "/pattern"])[:need + GUARD].astype(bool)
    pat_plain = np.unpackbits(plain[k + "/pattern"])[:need + GUARD].astype(bool)
    written = int((~pat_plain[:need]).sum())
    floor = 64 * sum(n * MIN_TENSORS[s] for n, s in zip(case, ("cons", "vars", "cuts")))
    print(f"\n{k}: workspace {need} words, plain build wrote {written} (floor {floor}), write-through build {int((~pat_wt[:need]).sum())}")
    assert written >= floor, "the plain build left rows of its own result tensors unwritten: the reference proves nothing"
    for tag, pat in (("plain", pat_plain), ("write-through", pat_wt)):
        assert pat[need:].all(), f"{tag}: the guard rows behind the workspace were written"
    dropped, stray = np.flatnonzero(pat_wt & ~pat_plain), np.flatnonzero(~pat_wt & pat_plain)
    assert dropped.size == 0, f"{dropped.size} words the plain build writes still carry the pattern, first at word {dropped[0]} (row {dropped[0] // 64})"
    assert stray.size == 0, f"{stray.size} words written that the plain build leaves alone, first at word {stray[0]}"
    assert np.array_equal(wt[k + "/sha"], plain[k + "/sha"]), "the workspaces hold different bits"
    for name in ("loss", "scores", "grads"):
        a, b = _words(wt[f"{k}/{name}"]), _words(plain[f"{k}/{name}"])
        assert not (a == PATTERN).any() and not np.isnan(wt[f"{k}/{name}"]).any(), name
        assert np.array_equal(a, b), f"{name} differs from the plain build's bits"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["wt", "plain"])
def test_second_batch_through_a_used_workspace_equals_a_fresh_model(runs, tag):
    r = runs[tag]
    for name in ("loss", "scores", "grads"):
        a, b = _words(r["pair/" + name]), _words(r["fresh/" + name])
        assert not (a == PATTERN).any() and not np.isnan(r["pair/" + name]).any(), name
        assert np.array_equal(a, b), f"{tag}: {name} of the second batch depends on what the first left in the workspace"
    assert np.array_equal(_words(runs["wt"]["pair/grads"]), _words(runs["plain"]["pair/grads"]))


WT_STORE = re.compile(r"global_store_dwordx4 .*\bsc1\b")


def _kernels(asm):
    """{mangled kernel symbol: body}"""
    db = buildsupport.device_build()
    return {s: db.body(s) for s in re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)}


def test_write_through_kernels_store_sc1_and_every_other_kernel_plain():
    db = buildsupport.device_build()
    ks = _kernels(db.asm)
    assert len(ks) > 40, sorted(ks)
    for stem in ("k_embed_fwd_wtILi", "k_conv_fwd_wtILi", "k_conv_bwd_wtILi", "k_tail_bwd_wtILi"):
        hit = [s for s in ks if stem in s]
        assert len(hit) >= 2, (stem, hit)   # the 4- and the 8-wave form
        for s in hit:
            assert WT_STORE.search(ks[s]), f"{s} stores its results with plain stores"
            # only the 16-byte form: a narrower sc1 store is 6-12x the time per byte
            assert not re.search(r"(global|buffer|flat)_store_(byte|short|dword|dwordx2|dwordx3) .*\bsc1\b", ks[s]), s
    plain = [s for s in ks if "_wtILi" not in s]
    assert len(plain) > 40
    for s in plain:
        assert not WT_STORE.search(ks[s]), f"{s}: write-through stores outside the adopted kernels"


def test_write_through_embedding_keeps_four_waves_per_simd():
    """The residency tests/test_kernel_resources.py pins for k_embed_fwd<8> (two 8-wave blocks per CU), for its write-through twin."""
    usage = buildsupport.device_build().demangled()
    hits = {k: v for k, v in usage.items() if k.replace("void ", "").startswith("k_embed_fwd_wt<8>")}
    assert len(hits) == 1, hits
    assert all(v["occ"] >= 4 and not v.get("scratch", 0) for v in hits.values()), hits
