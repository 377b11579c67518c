"""The library's host code (csrc/gcnn_*.hpp and the host half of gcnn_capi.hip) under AddressSanitizer and
UndefinedBehaviorSanitizer, on the CPU: tests/hostsan's stand-alone program executes the records of hostsancases.py with every
output buffer malloc'ed at exactly the size the library asked for, and writes back what the library returned and wrote.

What is asserted: the run is clean (exit 0 under UBSAN_OPTIONS=halt_on_error=1, no report on stderr); the sanitizers are live
(the program's three self-test modes, errors in its own code, must each be reported); every record gives the bytes the -O3 product
library gives through the ctypes binding; layouts are aligned, ordered and inside their totals, tables point inside the arena, a
refused call leaves its output as it found it; packed edges equal NumPy's stable argsort; and every size function, layout
function, table writer and host packer the header declares has records.

No GPU takes part and none is needed: the program enqueues nothing -- pure host functions, and argument sets an entry point
refuses before its first HIP call.  One size query does reach the HIP runtime: every layout that sizes a sort asks rocprim for the
radix sort's temporary storage, which rocprim picks for the current device.  So both the program and the product-library side
run with every device hidden, and that size is the same on both sides everywhere.

Leak detection is off for the run (ASAN_OPTIONS=detect_leaks=0).  On a machine without a driver a run with it on reports nothing;
what the HIP runtime's start-up (the static registration of the code objects) leaves allocated at exit differs with the driver
it finds, is not the library's -- whose host code owns no heap memory beyond function-local std::vectors -- and must not decide
this test.  -fsanitize=implicit-conversion (silent 64-to-32-bit narrowing of sizes) is part of the build: it reports nothing
in the library, and a third self-test mode shows that it would."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import buildsupport
import hostsancases as H
import hostsanlayouts as layouts

ROOT = buildsupport.ROOT
HIDDEN = {"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}
SAN_ENV = {**HIDDEN, "ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
REPORT = re.compile(r"runtime error|AddressSanitizer|LeakSanitizer")


def _env(extra):
    return {**os.environ, **extra}


class Run:
    pass


_run = None


@pytest.fixture(scope="module")
def run():
    """One execution of the whole list by both sides, shared by the tests below and left unchanged."""
    global _run
    if _run is None:
        program = buildsupport.host_sanitizer_build()
        r = Run()
        r.program = program
        r.tmp = tempfile.mkdtemp(prefix="gcnn_hostsan_run_")
        atexit.register(shutil.rmtree, r.tmp, ignore_errors=True)
        cases, san, lib = (os.path.join(r.tmp, n) for n in ("cases.bin", "san.bin", "lib.bin"))
        r.records = H.write_cases(cases)
        r.san_proc = subprocess.run([program, cases, san], capture_output=True, text=True, timeout=300, env=_env(SAN_ENV))
        r.lib_proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hostsancases.py"), "--ctypes", cases, lib],
                                    capture_output=True, text=True, timeout=300, env=_env(HIDDEN), cwd=ROOT)
        r.san = H.read_results(san) if os.path.exists(san) else []
        r.lib = H.read_results(lib) if os.path.exists(lib) else []
        _run = r
    return _run


def test_the_sanitizers_are_live():
    program = buildsupport.host_sanitizer_build()
    p = subprocess.run([program, "--selftest-asan"], capture_output=True, text=True, timeout=60, env=_env(SAN_ENV))
    assert p.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in p.stderr and "selftest_asan" in p.stderr, p.stderr[-2000:]
    p = subprocess.run([program, "--selftest-ubsan"], capture_output=True, text=True, timeout=60, env=_env(SAN_ENV))
    assert p.returncode != 0 and "runtime error: signed integer overflow: 2147483647 + 1" in p.stderr, p.stderr[-2000:]
    p = subprocess.run([program, "--selftest-conversion"], capture_output=True, text=True, timeout=60, env=_env(SAN_ENV))
    assert p.returncode != 0 and "runtime error: implicit conversion from type 'long long'" in p.stderr, p.stderr[-2000:]


def test_the_whole_list_runs_clean(run):
    p = run.san_proc
    assert p.returncode == 0 and not REPORT.search(p.stderr), (p.returncode, p.stderr[-4000:])
    assert f"hostsan: {len(run.records)} records" in p.stderr and len(run.san) == len(run.records)


def test_every_record_gives_the_product_librarys_bytes(run):
    assert run.lib_proc.returncode == 0, run.lib_proc.stderr[-4000:]
    assert len(run.lib) == len(run.san) == len(run.records)
    for i, ((fid, words), a, b) in enumerate(zip(run.records, run.san, run.lib)):
        assert a == b, (i, fid, words[:40], a[0], b[0], len(a[1]), len(b[1]),
                        next((k for k, (x, y) in enumerate(zip(a[1], b[1])) if x != y), None))
    # the list is not a list of refusals: most layouts are accepted, and every function has accepted records
    by = {}
    for (fid, _), (rc, _) in zip(run.records, run.san):
        by.setdefault(fid, []).append(rc)
    for fid, rcs in by.items():
        assert any(rc >= 0 for rc in rcs) or fid == H.REFUSALS, fid
    assert all(rc < 0 for rc in by[H.REFUSALS]) and len(by[H.REFUSALS]) > 200


def test_every_host_entry_point_of_the_header_has_records(run):
    header = open(buildsupport.HEADER).read()
    decl = re.findall(r"^(?:int|size_t)\s+(gcnn_\w+)\s*\(", header, re.M)
    sized = re.findall(r"^size_t\s+(gcnn_\w+)\s*\(", header, re.M)
    want = {n for n in decl if n.endswith("_layout_for") or n.endswith("_fill_table") or n.startswith("gcnn_host_") or
            n.startswith("gcnn_param_") or n == "gcnn_group_table_bytes"} | set(sized)
    assert len(want) == 20 + 5 + 2 + 3 + 1 + 3, sorted(want)
    # a function's key is its id, or (id, first word) where two functions share an id: each has to have records of its own
    have = {fid for fid, _ in run.records} | {(fid, w[0]) for fid, w in run.records if w}
    missing = sorted(n for n in want if H.FUNCTIONS.get(n) not in have)
    assert not missing, missing
    # every other declared function launches: it has refusal records, made by the sanitized program and matched there
    launching = sorted(set(decl) - want - set(H.NOT_LAUNCHING))
    assert launching == sorted(H.REFUSAL_ENTRIES), sorted(set(launching) ^ set(H.REFUSAL_ENTRIES))
    entries = {w[0] for fid, w in run.records if fid == H.REFUSALS}
    assert entries == set(range(len(H.REFUSAL_ENTRIES)))
    for e in range(len(H.REFUSAL_ENTRIES)):
        assert sum(1 for fid, w in run.records if fid == H.REFUSALS and w[0] == e) >= 3, H.REFUSAL_ENTRIES[e]


# ---- layouts ---------------------------------------------------------------------------------------------------------------------

def _layout_types():
    from gcnn_cut_selector_amd import _lib
    return {10: _lib.InferLayout, 11: _lib.SelectLayout, 12: _lib.IbatchLayout, 13: _lib.MbatchLayout, 14: _lib.EnsembleLayout,
            15: _lib.EnsembleLayout, 16: _lib.LpLayout, 17: _lib.LpBatchLayout, 18: _lib.LpModelsLayout, 19: _lib.LpCollectLayout,
            20: _lib.LpRowsLayout, 21: _lib.LpRoundLayout, 22: _lib.LpAppendLayout, 23: _lib.LpRemoveLayout, 24: _lib.LpRoundsLayout,
            25: _lib.LpRoundsEditLayout, 26: _lib.LpEnsembleLayout, 27: _lib.LpEnsembleLayout, 28: _lib.LpRoundEnsembleLayout,
            29: _lib.HybridLayout}


def test_a_refused_call_leaves_its_output_as_it_was(run):
    types = _layout_types()
    untouched = lambda blob: blob == bytes([H.FILL]) * len(blob)  # noqa: E731
    seen = 0
    for (fid, words), (rc, blob) in zip(run.records, run.san):
        if rc < 0 and rc != H.SKIPPED and (fid in types or fid in (3, 4) or 30 <= fid <= 34 or (fid == 40 and rc == -1)):
            assert untouched(blob), (fid, words[:40], rc)
            seen += 1
    assert seen > 1000


def _flat(x):
    if isinstance(x, C.Array):
        return [v for item in x for v in _flat(item)]
    return [x]


# the header's alignments: 16 inside an upload, a download or a scratch block, 256 for a block of the device arena
IN_FIELDS = ("in_off", "forced_off")
ARENA_FIELDS = ("ws_off", "lp_off", "scratch_off", "out_dev_off", "rows_off", "up_off", "round_off", "arena_off", "lp_scratch_off",
                "hyb_scratch_off", "append_scratch_off", "remove_scratch_off", "counts_base", "out_base", "member_off", "member_round_off")


def _used(offs):
    """offs without the entries a layout does not use, which stay zero at its end (members or blocks it has none of)."""
    offs = list(offs)
    while offs and offs[-1] == 0:
        offs.pop()
    return offs


def _walk(L, path=""):
    """(path, struct) of L and of every struct nested in it."""
    yield path, L
    for name, _ in L._fields_:
        v = getattr(L, name)
        if isinstance(v, C.Structure):
            yield from _walk(v, f"{path}{name}.")


def test_offsets_are_aligned_and_inside_their_totals(run):
    from gcnn_cut_selector_amd import _lib
    types = _layout_types()
    checked = 0
    for (fid, words), (rc, blob) in zip(run.records, run.san):
        if fid not in types or rc != 0:
            continue
        top = types[fid].from_buffer_copy(blob)
        arena_top = next((getattr(s, "arena_bytes") for _, s in _walk(top) if hasattr(s, "arena_bytes")), None)
        for path, L in _walk(top):
            names = {n for n, _ in L._fields_}
            ctx = (fid, words[:40], path)
            if isinstance(L, _lib.LpLayout) and not L.call_supported:
                assert L.arena_bytes == 0 and L.out_bytes == 0 and L.snap_bytes % 16 == 0 and max(L.snap_off) <= L.snap_bytes, ctx
                continue
            if "in_bytes" in names:
                for f in names & set(IN_FIELDS):
                    offs = _used(_flat(getattr(L, f)))
                    assert all(o % 16 == 0 and o <= L.in_bytes for o in offs) and offs == sorted(offs), (ctx, f, offs, L.in_bytes)
            if "snap_bytes" in names:
                offs = list(L.snap_off)
                assert offs == sorted(offs) and all(o % 16 == 0 for o in offs) and offs[-1] <= L.snap_bytes <= L.in_bytes, ctx
            if "out_bytes" in names and "out_off" in names and "out_base" not in names:
                offs = _used(_flat(L.out_off))
                assert all(o % 16 == 0 and o <= L.out_bytes for o in offs) and offs == sorted(offs), (ctx, offs, L.out_bytes)
            arena = getattr(L, "arena_bytes", arena_top)
            if arena is None:
                continue
            # the single-state arena starts its blocks right behind the upload (16-byte aligned) in steps of 256 bytes; every other
            # arena starts them at multiples of 256
            solo = isinstance(L, (_lib.InferLayout, _lib.SelectLayout))
            unit = 16 if solo else 256
            assert arena % 16 == 0, ctx      # (a layout that ends in a scratch block ends 16-byte aligned)
            for f in names & set(ARENA_FIELDS):
                offs = _flat(getattr(L, f))
                assert all(o % unit == 0 and o <= arena for o in offs), (ctx, f, offs, arena)
            if "dev_off" in names:
                offs = list(L.dev_off)
                if isinstance(L, _lib.InferLayout):      # [0], [1]: the two by-left offset arrays, inside the uploaded zero block
                    assert L.in_off[0] <= offs[0] <= offs[1] <= L.in_off[1] and offs[0] % 4 == 0 and offs[1] % 4 == 0, ctx
                    offs = offs[2:]
                    assert all((o - L.in_bytes) % 256 == 0 for o in offs), ctx
                offs = _used(offs)
                assert all(o % unit == 0 and o <= arena for o in offs) and offs == sorted(offs), (ctx, offs, arena)
                if "in_bytes" in names and offs and not isinstance(L, _lib.LpRoundLayout):
                    assert offs[0] >= L.in_bytes, ctx
            if "table_bytes" in names:
                assert L.table_bytes % 16 == 0, ctx
        checked += 1
    assert checked > 2000


def test_every_block_of_every_layout_fits(run):
    """All 20 layouts, block by block, in Python integers from the dims (hostsanlayouts.py restates what lies behind each offset):
    no block starts before the one in front of it ends, and the last ends inside the stated total."""
    types = _layout_types()
    seen = {}
    for (fid, words), (rc, blob) in zip(run.records, run.san):
        if fid in types and rc == 0:
            L = types[fid].from_buffer_copy(blob)
            bad = layouts.fits(layouts.blocks_of(fid, words, L))
            assert bad is None, (fid, words[:48], bad)
            seen[fid] = seen.get(fid, 0) + 1
    assert set(seen) == set(types) and all(v >= 20 for v in seen.values()), seen


def H_select_ws(cuts, forced, max_cuts):
    """gcnn_select_workspace_bytes: two bits of parallelism per pair the filter can consult, 16 bytes per row and 64 cuts."""
    return max((cuts + forced) * ((max_cuts + 63) // 64) * 16, 16)


def test_size_functions_in_python_integers(run):
    for (fid, words), (rc, blob) in zip(run.records, run.san):
        if fid == 2:
            a, b, c = (max(x, 0) for x in words)
            assert int.from_bytes(blob, "little") == H_select_ws(a, b, c), words
        if fid == 0:
            got = int.from_bytes(blob, "little")
            bad = words[0] & H.NULL_FIRST or min(words[1:]) < 0
            assert (got == 0) == bool(bad), words
            if not bad:
                assert got == layouts.workspace_floats(*words[1:6]), words
        if fid == 1:
            assert int.from_bytes(blob, "little") >= 3 * 4 * max(words[0], 1), words


def test_tables_point_inside_the_arena(run):
    """The byte positions of the descriptors of gcnn_hybrid_fill_table (18 per snapshot), gcnn_lp_batch_fill_table and
    gcnn_lp_models_fill_table (38) against the arena of the same record's layout, as the sanitized program got it; the offset
    columns of the union tables; and the model words behind them (gcnn_infer_models_fill_table, gcnn_lp_models_fill_table)."""
    from gcnn_cut_selector_amd import _lib
    stride = _lib.IBATCH_TABLE_STRIDE
    by_record = {(fid, tuple(words)): blob for (fid, words), (rc, blob) in zip(run.records, run.san) if fid in (17, 18, 29) and rc == 0}
    seen = {30: 0, 31: 0, 32: 0, 33: 0, 34: 0}

    def columns(table, n):
        cols = table[:7 * stride].reshape(7, stride)[:, :n + 1]
        assert (cols[:, 0] == 0).all() and (np.diff(cols, axis=1) >= 0).all()
        assert (cols[:3, -1] <= 1 << 24).all() and (cols[3:5, -1] <= 1 << 30).all() and cols[5, -1] <= 1 << 24 and cols[6, -1] <= 1 << 30

    def model_words(table, n, n_models, model_of):
        mod = table[7 * stride:7 * stride + 16 + 64]
        first = mod[1:2 + n_models].tolist()
        assert mod[0] == n_models and first[0] == 0 and first[-1] == n and first == sorted(first) and (mod[2 + n_models:16] == 0).all()
        assert mod[16:16 + n].tolist() == list(model_of) and (mod[16 + n:] == 0).all()
        assert all(model_of[s] == m for m in range(n_models) for s in range(first[m], first[m + 1]))

    for (fid, words), (rc, blob) in zip(run.records, run.san):
        if rc != 0 or not blob or fid not in seen:
            continue
        n, real = words[0], words[1]
        table = np.frombuffer(blob, np.int32)
        if fid == 34:
            L = _lib.HybridLayout.from_buffer_copy(by_record[29, tuple(words[:-1])])
            assert len(blob) == L.table_bytes and table[0] == n
            head = 4 + 4 * stride
            entry = (L.table_bytes - 4 * head) // n
            for s in range(n):
                pos = table[head + s * entry // 4:][:2 * 18].view(np.int64)
                assert (pos >= 0).all() and (pos < L.arena_bytes).all(), (words[:20], s, pos.tolist(), L.arena_bytes)
        if fid in (32, 33):    # the union's table, two block prefixes, then the descriptors (word 0 of each is a count, not a position)
            if fid == 32:
                L, union = _lib.LpBatchLayout.from_buffer_copy(by_record[17, tuple(words[:-1])]), 7 * stride
            else:
                L, union = _lib.LpModelsLayout.from_buffer_copy(by_record[18, tuple(words[:-1])]).lp, _lib.MBATCH_TABLE_WORDS
            head = 4 + 2 * stride
            assert len(blob) == L.table_bytes and table[union] == n
            entry = (L.table_bytes - 4 * union - 4 * head) // n
            for s in range(n):
                pos = table[union + head + s * entry // 4:][:2 * 38].view(np.int64)
                assert (pos[1:] >= 0).all() and (pos[1:] < L.arena_bytes).all(), (words[:20], s, pos.tolist(), L.arena_bytes)
        if fid in (30, 31, 32, 33):
            columns(table, n)
        if fid in (31, 33):
            width = 5 if fid == 31 else 10
            model_of = words[3 + (width + 2) * real:3 + (width + 3) * real]
            model_words(table, n, words[-2], model_of)
        seen[fid] += 1
    assert all(v > 50 for v in seen.values()), seen


# ---- packed edges ------------------------------------------------------------------------------------------------------------------

def test_packed_edges_equal_numpys_stable_argsort(run):
    seen = {0: 0, 1: 0, 2: 0, -1: 0}
    for (fid, words), (rc, blob) in zip(run.records, run.san):
        if fid != 40:
            continue
        which, n_edges, n_left, k, mask, _ = words[:6]
        rows, cols = np.asarray(words[6:6 + k], np.int32), np.asarray(words[6 + k:6 + 2 * k], np.int32)
        vals = (1.0 + 0.25 * np.arange(k)).astype(np.float32)
        inds, out_vals = np.frombuffer(blob[:8 * k], np.int32), np.frombuffer(blob[8 * k:], np.float32)
        in_range = k == 0 or (rows.min() >= 0 and rows.max() < n_left)
        is_sorted = bool((np.diff(rows) >= 0).all())
        bad = n_edges < 0 or n_left < 0 or (n_edges > 0 and mask)
        if which == 0:
            want_rc = -1 if bad else 0 if (is_sorted or n_edges == 0) else 1 if in_range else 2
        else:
            want_rc = -1 if bad or not (in_range or n_edges == 0) else 0
        assert rc == want_rc, (words[:12], rc, want_rc)
        seen[rc] += 1
        if rc == -1 or n_edges == 0:
            assert blob == bytes([H.FILL]) * len(blob), words[:12]        # nothing written
        elif rc == 2 or (rc == 0 and which == 0):                         # passed through as it is
            assert inds.tolist() == rows.tolist() + cols.tolist() and out_vals.tobytes() == vals.tobytes(), words[:12]
        else:
            order = np.argsort(rows, kind="stable")
            assert inds.tolist() == rows[order].tolist() + cols[order].tolist() and out_vals.tobytes() == vals[order].tobytes(), words[:12]
    assert all(v >= 3 for v in seen.values()), seen
