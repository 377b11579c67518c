"""tests/batchcases.py proved on the host: the constants are the source's, every case is what its id says, every item of every launch
is served by exactly one thread on one trip, the restatement equals the plain operation (`np.argsort(kind="stable")` with
`np.bincount(...).cumsum()`; `utils.collate` followed by that CSR), a restatement with one of the named defects changes an exact
expected output on a named case, and the three entry points refuse bad arguments without a device.  CPU only."""
import os
import re
import time

import numpy as np
import pytest

import batchcases as B

S_CHECK, S_BUILD = B.check_seam(), B.build_seam()


# ---- the thresholds and the rules are the source's -----------------------------------------------------------------------------------
def test_constants_are_those_of_the_launchers_and_the_kernels():
    c = B.constants()
    assert (c["check_threads"], c["check_max"], c["build_threads"], c["build_max"]) == (256, 1024, 256, 4096)
    assert (c["chunks"], c["collate_max"], c["collate_stride"], c["max_jobs"]) == (8, 2048, 256, 24)
    # where the issue's seams are: the second trips start at 262,145 edges (check), 1,048,576 edges (build: its items are E + 1),
    # 257 samples and 2,049 words
    assert (S_CHECK + 1, S_BUILD, B.collate_seam() + 1, B.inner_seam() + 1) == (262145, 1048576, 257, 2049)
    assert B.check_grid(S_CHECK) == B.check_grid(S_CHECK + 1) == 1024 and B.check_grid(S_CHECK - 256) == 1023
    assert B.build_grid(S_BUILD - 1) == B.build_grid(S_BUILD) == 4096 and B.build_grid(S_BUILD - 257) == 4095
    assert B.collate_grid(256) == B.collate_grid(257) == 2048 and B.collate_grid(255) == 2040
    assert B.check_sizes() == (1, 2, 255, 256, 257, 262143, 262144, 262145, 524289)
    assert [B.large_specs()[i][0] for i in B.LARGE_IDS] == [1048575, 1048575, 1048576, 1048576, 1048577, 1048577, 2097153, 2097153]
    assert B.large_words() == (2040, 2047, 2048, 2049, 2056, 2057, 4097)
    assert tuple(B.batches()) == B.BATCH_IDS


def test_rules_restated_are_the_kernels_lines():
    misc = open(os.path.join(B.CSRC, "k_misc.hpp")).read()
    for line in ("bad |= (l < 0) | (l >= n_left) | (v < 0) | (v >= n_var);",
                 "if (i + 1 < n) unsorted |= ei[i + 1] < l;",
                 "const int l = ei[i], v = ei[n + i];",
                 "for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {",
                 "const int lo = i == 0 ? -1 : max(keys[i - 1], -1);",
                 "const int hi = i == n ? n_seg : min(keys[i], n_seg);",
                 "for (int k = lo + 1; k <= hi; ++k) ptr[k] = i;",
                 "for (int item = blockIdx.x; item < a.batch * COLLATE_CHUNKS; item += gridDim.x) {",
                 "const long long per = (words + COLLATE_CHUNKS - 1) / COLLATE_CHUNKS;",
                 "const long long w0 = min(words, c * per), w1 = min(words, w0 + per);",
                 "j.dst[dof[a.batch] * j.width] = (int)aof[a.batch];",
                 "const int add = aof ? (int)aof[s] : 0, n = (int)(w1 - w0);"):
        assert line in misc, line
    capi = open(os.path.join(B.CSRC, "gcnn_capi.hip")).read()
    assert "while ((1ll << bits) < (long long)nseg + 1 && bits < 31) ++bits;" in capi and "unsigned bits = 1;" in capi
    assert re.search(r"radix_sort_pairs\(sort_tmp, sort_bytes, key_in, keys, iota, perm, \(unsigned\)n_edges, 0u, bits, st\)", capi)
    assert [B.sort_bits(n) for n in (0, 1, 2, 3, 255, 256, 257, 65535, 65536, 65537)] == [1, 1, 2, 2, 8, 9, 9, 16, 17, 17]


# ---- every item is served once -------------------------------------------------------------------------------------------------------
def _served(n_items, n_workers):
    """How often each item is taken when worker w takes w, w + n_workers, ... -- and on which trip."""
    count, trip_of = np.zeros(n_items, np.int64), np.full(n_items, -1, np.int64)
    trip = 0
    while trip * n_workers < n_items or trip == 0:
        items = trip * n_workers + np.arange(n_workers)
        items = items[items < n_items]
        count[items] += 1
        trip_of[items] = trip
        trip += 1
    return count, trip_of, trip


@pytest.mark.parametrize("n", B.check_sizes() + (S_BUILD - 1, S_BUILD, S_BUILD + 1, 2 * S_BUILD + 1))
def test_every_item_of_the_check_and_the_build_has_one_thread_on_one_trip(n):
    count, trip_of, trips = _served(n, B.check_grid(n) * 256)                  # k_check_edges: items [0, n)
    assert (count == 1).all() and trips == B.cdiv(n, S_CHECK) and trip_of[-1] == (n - 1) // S_CHECK
    count, trip_of, trips = _served(n + 1, B.build_grid(n) * 256)              # k_seg_offsets: items [0, n]
    assert (count == 1).all() and trips == B.cdiv(n + 1, S_BUILD) and trip_of[n] == n // S_BUILD
    count, _, _ = _served(n, B.build_grid(n) * 256)                           # k_iota, k_gather_edges: items [0, n) on the same grid
    assert (count == 1).all()
    assert B.build_grid(n) * 256 >= min(n + 1, S_BUILD)                        # an uncapped grid has a thread per item


@pytest.mark.parametrize("bid", B.BATCH_IDS)
def test_every_chunk_of_every_sample_has_one_block_and_every_word_one_chunk(bid):
    ids = B.batches()[bid]
    count, trip_of, trips = _served(len(ids) * 8, B.collate_grid(len(ids)))
    assert (count == 1).all() and trips == B.cdiv(len(ids), B.collate_seam())
    for words in set(w for i in set(ids.tolist()) for w in B.words_of(B.pool()[i]).values()):
        ch = B.chunks(words)
        covered = np.zeros(words, np.int64)
        for w0, w1 in ch:
            assert 0 <= w0 <= w1 <= words
            covered[w0:w1] += 1
        assert (covered == 1).all(), words
        assert max(w1 - w0 for w0, w1 in ch) == B.cdiv(words, 8)


# ---- check cases ------------------------------------------------------------------------------------------------------------------------
def _plain_flags(c):
    left, var = c["left"].astype(np.int64), c["var"].astype(np.int64)
    bad = (left.min() < 0) or (left.max() >= c["n_left"]) or (var.min() < 0) or (var.max() >= c["n_var"])
    return int(bad), int(np.any(np.diff(left) < 0))


def test_check_bases_are_sorted_valid_and_end_above_the_first_variable_id():
    for n in B.check_sizes():
        left, var = B.check_base(n)
        assert left.size == var.size == n and np.all(np.diff(left) >= 0)
        assert left.min() >= 1 and left[-1] == B.CHECK_N_LEFT - 1 and var.min() >= 0 and var.max() < B.CHECK_N_VAR
        assert var[0] < left[-1]                                # an unguarded item n - 1 would call this a descent
        assert n == 1 or var.max() == B.CHECK_N_VAR - 1


@pytest.mark.parametrize("n", B.check_sizes())
def test_check_cases_plant_one_entry_and_flag_what_their_id_says(n):
    base = B.check_base(n)
    kinds = B.check_plants(n)
    want_pos = {p for p in (0, 255, 256, S_CHECK - 1, S_CHECK, n - 1) if p < n}
    assert {int(k.split("@")[1]) for k in kinds if "=" in k} == want_pos
    assert {int(k.split("@")[1]) for k in kinds if k.startswith("descent")} == {p for p in (0, 255, S_CHECK - 1, S_CHECK, n - 2)
                                                                                if 0 <= p < n - 1}
    for kind in kinds:
        c = B.check_case(f"E{n}/{kind}")
        got = B.check_flags(c["left"], c["var"], c["n_left"], c["n_var"])
        assert got == _plain_flags(c), (n, kind)
        changed = [int((c[r] != b).sum()) for r, b in zip(("left", "var"), base)]
        if kind in ("ok", "ties", "max-only"):
            assert got == (0, 0)
            if kind == "ties":
                assert np.unique(c["left"]).size == 1
            if kind == "max-only":
                assert (c["left"] == c["n_left"] - 1).all() and (c["var"] == c["n_var"] - 1).all()
        elif kind.startswith("descent"):
            p = int(kind.split("@")[1])
            assert changed == [1, 0] and got == (0, 1) and np.flatnonzero(np.diff(c["left"]) < 0).tolist() == [p]
        else:
            row, rest = kind.split("=")
            value, p = rest.split("@")
            p = int(p)
            assert changed == ([1, 0] if row == "left" else [0, 1])
            assert c[row][p] == (-1 if value == "-1" else c["n_" + row])
            # a wrong left id is also out of order against a neighbour: below the one in front of it, or above the one behind
            unsorted = int(row == "left" and ((value == "-1" and p > 0) or (value == "n" and p < n - 1)))
            assert got == (1, unsorted), (n, kind)


# ---- build cases ------------------------------------------------------------------------------------------------------------------------
def _plain_csr(left, var, coef, n_left, n_var):
    out = []
    for key, oth, n in ((left, var, n_left), (var, left, n_var)):
        order = np.argsort(key, kind="stable")
        ptr = np.concatenate([[0], np.bincount(key, minlength=n).cumsum()]).astype(np.int32)
        out.append((ptr, oth[order], coef[order], order.astype(np.int32)))
    (lp, lo, lc, perm), (vp, vo, vc, _) = out
    return lp, lo, lc, perm, vp, vo, vc


def _same(a, b):
    return [f for f, x, y in zip(B.CSR_FIELDS, a, b) if not (x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32)))]


@pytest.mark.parametrize("cid", B.BUILD_IDS)
def test_restated_csr_is_the_plain_stable_order(cid):
    c = B.build_case(cid)
    assert c["left"].size == 0 or (0 <= c["left"].min() and c["left"].max() < c["n_left"] and 0 <= c["var"].min() and c["var"].max() < c["n_var"])
    assert c["left_sorted"] == bool(np.all(np.diff(c["left"]) >= 0)) == (not B.check_flags(c["left"], c["var"], c["n_left"], c["n_var"])[1])
    assert np.unique(c["coef"]).size == c["coef"].size and np.array_equal(c["coef"].astype(np.int64).astype(np.float32), c["coef"])
    want = _plain_csr(c["left"], c["var"], c["coef"], c["n_left"], c["n_var"])
    t0 = time.perf_counter()
    got = B.expected_csr(cid, left_sorted=False)
    took = time.perf_counter() - t0
    assert _same(got, want) == [], cid
    if c["left_sorted"]:
        assert _same(B.expected_csr(cid, left_sorted=True), want) == [], cid       # the copy path gives the sort path's arrays
    if cid in B.LARGE_IDS:
        print(f"\n{cid}: restated in {took:.2f} s")
        assert took < 5.0                                       # about a second each where measured; eight of them


def test_small_build_cases_are_what_their_ids_say():
    for e in (1, 255, 256, 257):
        assert B.build_case(f"E/{e}/sorted")["left"].size == e
    for n in (1, 2, 255, 256, 257, 65535, 65536, 65537):
        for form in ("sorted", "unsorted")[:1 if n == 1 else 2]:
            c = B.build_case(f"nseg/{n}/{form}")
            assert c["n_left"] == c["n_var"] == n
            for row in ("left", "var"):
                assert c[row].min() == 0 and c[row].max() == n - 1
    lens = lambda cid, i: np.diff(B.expected_csr(cid)[i].astype(np.int64))
    first, last, both = (lens(f"{k}/sorted", 0) for k in ("first-only", "last-only", "first-last"))
    assert first.size == last.size == both.size == 300001
    assert first[0] == 6 and first[1:].sum() == 0 and last[-1] == 6 and last[:-1].sum() == 0
    assert both[0] == both[-1] == 3 and both[1:-1].sum() == 0
    for cid in ("first-last/sorted", "first-last/unsorted"):    # both orders: one item of k_seg_offsets writes 300,000 entries
        c = B.build_case(cid)
        for row, n in (("left", c["n_left"]), ("var", c["n_var"])):
            _, trip, thread = B.seg_offsets(np.sort(c[row]), n)
            assert np.bincount(thread).max() == 300000 and (trip == 0).all()
    for form in ("sorted", "unsorted"):
        l, v = lens(f"lead-trail/{form}", 0), lens(f"lead-trail/{form}", 4)
        assert l[:400].sum() == 0 and l[600:].sum() == 0 and l[400] > 0 and l[599] > 0 and l.size == 1000
        assert v[:300].sum() == 0 and v[320:].sum() == 0 and v.size == 900
        t = B.build_case(f"ties/{form}")
        assert t["left"].size == 2000 and t["n_left"] == 3 and t["n_var"] == 2
    one = lens("one-seg/sorted", 0)
    assert one[4] == 300 and one.sum() == 300 and lens("one-seg/sorted", 4)[2] == 300
    assert B.build_case("E0/sorted")["left"].size == 0 and B.build_case("E0/sorted")["n_left"] == 5
    z = B.build_case("E0-void/sorted")
    assert (z["left"].size, z["n_left"], z["n_var"]) == (0, 0, 0) and [a.size for a in B.expected_csr("E0-void/sorted")] == [1, 0, 0, 0, 1, 0, 0]
    assert not B.build_case("E/257/unsorted")["left_sorted"] and B.build_case("E/257/sorted")["left_sorted"]
    # the temp of a direct build is carved in 256-byte steps: most cases have 4 E off that grid, a few on it
    sizes = [B.build_case(cid)["left"].size for cid in B.SMALL_IDS]
    assert sum(1 for n in sizes if n and (4 * n) % 256) >= 20 and any(n and (4 * n) % 256 == 0 for n in sizes)


@pytest.mark.parametrize("cid", B.LARGE_IDS)
def test_large_build_cases_change_key_on_the_trip_seams(cid):
    n, many, srt = B.large_specs()[cid]
    c = B.build_case(cid)
    assert c["left"].size == n and c["left_sorted"] == srt
    assert (4 * n) % 256 != 0 or n == S_BUILD                      # (the temp carve of the C ABI rounds 4 E up to 256 bytes)
    want = [p for p in (S_BUILD - 1, S_BUILD, S_BUILD + 1, 2 * S_BUILD) if 0 < p < n]
    assert B.forced_changes(n) == (want or [n - 2, n - 1])
    for row, n_seg, is_many in (("left", c["n_left"], many), ("var", c["n_var"], not many)):
        keys = np.sort(c[row])
        assert n_seg == (300001 if is_many else 5)
        used = np.unique(keys).size
        assert 190000 < used < 210000 if is_many else used == 5
        for p in B.forced_changes(n):
            assert keys[p - 1] != keys[p], (cid, row, p)
        ptr, trip, thread = B.seg_offsets(keys, n_seg)
        assert (trip >= 0).all() and trip.max() == n // S_BUILD
        closing = np.arange(int(keys[-1]) + 1, n_seg + 1)
        assert (ptr[closing] == n).all() and (trip[closing] == n // S_BUILD).all() and (thread[closing] == n % S_BUILD).all()
        if n == S_BUILD:                                           # the second trip is the closing item alone
            assert np.flatnonzero(trip == 1).tolist() == closing.tolist() and (thread[closing] == 0).all()
        if n > S_BUILD:                                            # entries written by the first items of a second (third) trip
            for p in B.forced_changes(n):
                if p >= S_BUILD:
                    assert ptr[keys[p]] == p and trip[keys[p]] == p // S_BUILD and thread[keys[p]] == p % S_BUILD


# ---- collate cases ------------------------------------------------------------------------------------------------------------------------
def test_pool_has_every_word_count_and_every_degenerate_sample():
    pool = B.pool()
    t = B.n_tiny()
    assert t == 40 and len(pool) == 48
    width = {name: w for name, _, w, _, _ in B.JOBS}
    assert sorted(set(width.values())) == [1, 4, 6, 14] and len(B.JOBS) == 16
    seen = {}
    for i, s in enumerate(pool):
        for name, words in B.words_of(s).items():
            seen.setdefault(words, set()).add(width[name])
        assert i >= t or max(B.sample_sizes(s)) <= 17
    for w in B.SEAM_WORDS + B.large_words():
        assert w in seen, w
    for wd in (1, 4, 6, 14):                                       # every width: an empty segment, a short one, one past a copy trip
        mine = [w for w, ws in seen.items() if wd in ws]
        assert 0 in mine and any(0 < w < 8 * wd + 8 for w in mine) and any(w > B.inner_seam() for w in mine), wd
    assert {w for w in B.SEAM_WORDS + B.large_words() if 4 in seen[w]} >= {0, 8, 16, 2040, 2048, 2056} and 2040 in {w for w, ws in seen.items() if 6 in ws}
    assert B.sample_sizes(pool[0]) == (0, 0, 0, 0, 0)
    nc, nv, nk, e1, e2 = B.sample_sizes(pool[1])
    assert nk == 0 and e2 == 0 and e1 > 0 and nc > 0
    assert B.sample_sizes(pool[2])[3:] == (0, 0) and B.sample_sizes(pool[2])[2] > 0
    assert B.sample_sizes(pool[3])[2:] == (0, 0, 0) and B.sample_sizes(pool[3])[0] > 0
    assert np.any(np.diff(pool[12][0][1]["indices"][0]) < 0)      # one sample's edges are not sorted
    for s in pool:
        for edge, nl in ((s[0][1], B.sample_sizes(s)[0]), (s[0][4], B.sample_sizes(s)[2])):
            ei = edge["indices"]
            flat = ei[0].astype(np.int64) * max(B.sample_sizes(s)[1], 1) + ei[1]
            assert np.unique(flat).size == flat.size and (ei.size == 0 or (ei.min() >= 0 and ei[0].max() < nl and ei[1].max() < B.sample_sizes(s)[1]))


def test_batches_are_what_their_ids_say():
    b, t = B.batches(), B.n_tiny()
    assert [len(b[k]) for k in ("b1", "b255", "b256", "b257", "b600")] == [1, 255, 256, 257, 600]
    for k in ("b255", "b256", "b257", "b600"):
        assert b[k].max() < t and np.unique(b[k]).size < len(b[k]) and np.unique(b[k]).size >= 38      # drawn with repeats
    assert b["void-ends"][0] == 0 and b["void-ends"][-1] == 0
    assert set(range(t, len(B.pool()))) <= set(b["large"].tolist()) and np.array_equal(b["every-tiny"], np.arange(t))


@pytest.mark.parametrize("bid", B.BATCH_IDS)
def test_restated_batch_is_the_host_collate_and_its_plain_csr(bid):
    from gcnn_cut_selector_amd import utils
    ids = B.batches()[bid]
    c, cei, cef, v, k, kei, kef, n_cons, n_vars, n_cuts, imp = utils.collate([B.pool()[i] for i in ids])
    got = B.collate(ids)
    bits = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32)
    want = {"cons_feats": bits(c), "var_feats": bits(v), "cut_feats": bits(k), "improvements": bits(imp)}
    for slot, (ei, ef, nl) in enumerate(((cei, cef, int(n_cons.sum())), (kei, kef, int(n_cuts.sum())))):
        plan = dict(zip(B.CSR_FIELDS, _plain_csr(ei[0], ei[1], ef.reshape(-1), nl, int(n_vars.sum()))))
        for f in ("l_ptr", "l_oth", "v_ptr", "v_oth"):
            want[f"{slot}.{f}"] = plan[f]
        for f in ("l_coef", "v_coef"):
            want[f"{slot}.{f}"] = bits(plan[f])
    assert set(got) == set(want) == set(B.NAMES)
    for name in B.NAMES:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (bid, name)
    guarded = B.collate(ids, guard=8)
    for name in B.NAMES:
        assert np.array_equal(guarded[name][:-8], got[name]) and (guarded[name][-8:] == B.PATTERN).all()


# ---- named defects -----------------------------------------------------------------------------------------------------------------------
# defect: [(case, must the flags change?)] -- the case ids are those tests/test_gpu_batch_seams.py runs on the device
CHECK_NAMED = {
    "check_one_trip": [(f"E{S_CHECK + 1}/left=-1@{S_CHECK}", True), (f"E{S_CHECK + 1}/var=n@{S_CHECK}", True),
                       (f"E{2 * S_CHECK + 1}/descent@{S_CHECK}", True), (f"E{S_CHECK}/left=n@{S_CHECK - 1}", False)],
    "check_reads_past_end": [("E1/ok", True), ("E256/ok", True), (f"E{S_CHECK + 1}/ok", True), ("E257/max-only", True)],
    "upper_le": [("E256/left=n@255", True), (f"E{S_CHECK + 1}/var=n@{S_CHECK}", True), ("E256/left=-1@255", False)],
    "neg_ok": [("E257/var=-1@256", True), ("E2/left=-1@0", True), ("E257/var=n@256", False)],
    "var_unchecked": [("E255/var=n@0", True), (f"E{S_CHECK}/var=-1@{S_CHECK - 1}", True), ("E255/left=n@0", False)],
    "ties_unsorted": [("E2/ties", True), ("E257/ties", True), ("E257/max-only", True)],
}
# defect: [(case, fields that must change, fields that must not)]
BUILD_NAMED = {
    "build_one_trip": [(f"L{S_BUILD}/seg5/sorted", ("l_ptr", "v_ptr"), ("l_oth", "v_oth", "l_perm")),
                       (f"L{S_BUILD + 1}/many/sorted", ("l_ptr", "v_ptr"), ()), (f"L{S_BUILD - 1}/seg5/sorted", (), B.CSR_FIELDS)],
    "no_closing": [("E/1/sorted", ("l_ptr", "v_ptr"), ()), ("first-only/sorted", ("l_ptr", "v_ptr"), ()), ("last-only/sorted", ("l_ptr",), ()),
                   (f"L{S_BUILD}/many/unsorted", ("l_ptr", "v_ptr"), ())],
    "no_leading": [("last-only/sorted", ("l_ptr", "v_ptr"), ()), ("lead-trail/unsorted", ("l_ptr", "v_ptr"), ()), ("E/1/sorted", ("l_ptr", "v_ptr"), ())],
    "gap_single": [("first-last/unsorted", ("l_ptr", "v_ptr"), ()), ("lead-trail/sorted", ("l_ptr", "v_ptr"), ()),
                   ("nseg/65537/unsorted", ("l_ptr", "v_ptr"), ())],
    "bits_short": [("nseg/257/unsorted", ("l_ptr", "l_oth", "v_ptr", "v_oth"), ()), ("nseg/65537/unsorted", ("l_ptr", "l_oth", "v_ptr", "v_oth"), ()),
                   ("nseg/257/sorted", ("v_ptr", "v_oth"), ("l_ptr", "l_oth", "l_perm")),
                   ("nseg/256/unsorted", (), B.CSR_FIELDS), ("nseg/65536/unsorted", (), B.CSR_FIELDS)],    # ids below n_seg need a bit less
    "unstable": [("ties/unsorted", ("l_oth", "l_coef", "l_perm", "v_oth", "v_coef"), ("l_ptr", "v_ptr")),
                 ("ties/sorted", ("v_oth", "v_coef"), ("l_oth", "l_coef", "l_perm"))],
    "perm_from_var": [("ties/sorted", ("l_perm",), ("l_ptr", "l_oth", "l_coef", "v_ptr", "v_oth", "v_coef")),
                      ("E/257/unsorted", ("l_perm",), ("l_ptr", "l_oth", "l_coef", "v_ptr", "v_oth", "v_coef"))],
}
# defect: [(batch, arrays that must change (None: none may))]
COLLATE_NAMED = {
    "collate_one_trip": [("b257", ("cons_feats", "0.l_oth", "1.v_ptr")), ("b600", ("var_feats",)), ("b256", None)],
    "inner_one_trip": [("large", ("cons_feats", "var_feats", "cut_feats", "improvements", "0.l_ptr", "0.l_coef", "1.v_oth")), ("every-tiny", None)],
    "per_floor": [("every-tiny", ("improvements", "0.l_oth", "1.l_coef", "0.v_ptr")), ("large", ("0.l_oth",))],
    "no_clamp": [("b1", ("cons_feats", "0.l_oth")), ("large", ("0.v_ptr", "1.v_ptr"))],   # behind the last sample's 9 words
    "add_prev": [("void-ends", ("0.l_ptr", "0.l_oth", "0.v_oth", "1.v_ptr")), ("b257", ("1.l_ptr",)), ("b1", None)],
    "ptr_tail_missing": [("b1", ("0.l_ptr", "0.v_ptr", "1.l_ptr", "1.v_ptr")), ("large", ("0.l_ptr",))],
}


@pytest.mark.parametrize("defect", B.DEFECTS["check"])
def test_named_check_defect_changes_the_flags(defect):
    assert set(CHECK_NAMED) == set(B.DEFECTS["check"])
    for cid, changes in CHECK_NAMED[defect]:
        assert cid in B.check_ids(), cid
        c = B.check_case(cid)
        args = (c["left"], c["var"], c["n_left"], c["n_var"])
        assert (B.check_flags(*args) != B.check_flags(*args, defect)) == changes, (defect, cid)


@pytest.mark.parametrize("defect", B.DEFECTS["build"])
def test_named_build_defect_changes_an_exact_expected_array(defect):
    assert set(BUILD_NAMED) == set(B.DEFECTS["build"])
    for cid, changed, same in BUILD_NAMED[defect]:
        assert cid in B.BUILD_IDS, cid
        differ = _same(B.expected_csr(cid), B.expected_csr(cid, defect=defect))
        assert set(changed) <= set(differ) and not set(same) & set(differ), (defect, cid, differ)


@pytest.mark.parametrize("defect", B.DEFECTS["collate"])
def test_named_collate_defect_changes_an_exact_expected_array(defect):
    assert set(COLLATE_NAMED) == set(B.DEFECTS["collate"])
    for bid, changed in COLLATE_NAMED[defect]:
        ids = B.batches()[bid]
        good, bad = B.collate(ids, guard=8), B.collate(ids, defect, guard=8)
        differ = {n for n in B.NAMES if not np.array_equal(good[n], bad[n])}
        assert (not differ) if changed is None else set(changed) <= differ, (defect, bid, sorted(differ))


def test_defects_lose_the_entries_they_are_named_for():
    cid = f"L{S_BUILD}/seg5/sorted"                                 # the second trip is item n alone: every closing entry, nothing else
    c = B.build_case(cid)
    good, bad = B.expected_csr(cid)[0], B.expected_csr(cid, defect="build_one_trip")[0]
    assert np.flatnonzero(good != bad).tolist() == list(range(int(c["left"].max()) + 1, c["n_left"] + 1)) and (bad[good != bad] == B.PATTERN).all()
    good, bad = B.expected_csr("first-last/sorted")[0], B.expected_csr("first-last/sorted", defect="gap_single")[0]
    assert np.flatnonzero(good != bad).tolist() == list(range(1, 300000))       # the run between the two keys; both keys' own entries stay
    ids = B.batches()["b257"]
    good, bad = B.collate(ids), B.collate(ids, "collate_one_trip")
    src_off, dst_off = B.tables(ids)
    for name, kind, width, _, is_ptr in B.JOBS:                     # the 257th sample's segment, and only that
        lost = np.flatnonzero(good[name] != bad[name])
        lo, hi = int(dst_off[kind][256]) * width, int(dst_off[kind][257]) * width
        assert ((lost >= lo) & (lost < hi)).all() and lost.size > 0.9 * (hi - lo) and (bad[name][lost] == B.PATTERN).all(), name
    words = B.words_of(B.pool()[B.n_tiny() + 6])["0.l_oth"]          # 4,097 words: chunks of 513, of which one trip copies 256
    assert words == 4097
    good, bad = B.collate([B.n_tiny() + 6]), B.collate([B.n_tiny() + 6], "inner_one_trip")
    assert int((bad["0.l_coef"] == B.PATTERN).sum()) == 4097 - 7 * 256 - 256 == int((good["0.l_coef"] != bad["0.l_coef"]).sum())


# ---- bad arguments -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_device():
    """What the three entry points return GCNN_E_BADARG for before any HIP call (gcnn_graph_build sizes its temp through
    gcnn_graph_temp_bytes only after these: tests/test_gpu_batch_seams.py has GCNN_E_WORKSPACE)."""
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    d = 256   # never dereferenced: every call below is refused before anything is enqueued
    check = lib.gcnn_graph_check
    assert check(d, -1, 4, 4, d, None) == -1                       # negative count
    assert check(d, 1, 4, 4, None, None) == -1                     # no flags
    assert check(None, 1, 4, 4, d, None) == -1                     # edges promised, none given
    build = lambda e=1, nl=1, nv=1, l_ptr=d, v_ptr=d: lib.gcnn_graph_build(d, d, e, nl, nv, 0, l_ptr, d, d, v_ptr, d, d, d, d, 1 << 30, None)
    assert build(e=-1) == -1 and build(nl=-1) == -1 and build(nv=-1) == -1
    assert build(l_ptr=None) == -1 and build(v_ptr=None) == -1
    assert build(e=0, l_ptr=None) == -1 and build(e=0, v_ptr=None) == -1

    def collate(n_jobs=1, batch=1, max_words=1, jobs=True, src_off=d, dst_off=d, kind=0, width=1, add=-1, is_ptr=0):
        arr = (_lib.CollateJob * 1)(_lib.CollateJob(d, d, kind, width, add, is_ptr))
        return lib.gcnn_collate(arr if jobs else None, n_jobs, src_off, dst_off, batch, max_words, None)

    assert collate(n_jobs=-1) == -1 and collate(batch=-1) == -1 and collate(max_words=-1) == -1
    assert collate(n_jobs=B.constants()["max_jobs"] + 1) == -1     # more jobs than the kernel's argument block holds
    assert collate(jobs=False) == -1 and collate(src_off=None) == -1 and collate(dst_off=None) == -1
    assert collate(width=0) == -1 and collate(width=-1) == -1 and collate(kind=-1) == -1
    assert collate(is_ptr=1, width=2, add=0) == -1                 # segment offsets are single words ...
    assert collate(is_ptr=1, width=1, add=-1) == -1                # ... and are shifted by some kind's offset
    assert collate(n_jobs=0) == 0 and collate(batch=0) == 0        # nothing to do: no launch
