"""The plan restatements and their cases (tests/plancases.py), proved on the host:

1. every launch formula the restatement uses still stands in the source, letter for letter;
2. on well-formed input the restatement is what plain NumPy says (searchsorted offsets, bincount sums, a stable argsort);
3. every case puts what it names on the seam it names, by the restated block / thread / trip maps;
4. each defect a plan kernel could have changes a named output of a named case (or trips the bounds check), so a device that had
   it would not pass tests/test_gpu_plan_seams.py -- no defective build is ever run on a device;
5. the degenerate states (edges with no rows or no variables to point at) leave their arrays in the restatement, which is why the
   single-state call refuses them on the host."""
import os
import re

import numpy as np
import pytest

import plancases as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcnn-cut-selector_amd", "csrc")
PLAN_KEYS = ("l_ptr0", "l_ptr1", "inds0", "inds1", "vcount", "cursor", "v_ptr", "v_pos", "v_oth", "v_coef", "flags", "left", "var0",
             "var1", "iota", "f_col", "path", "zeroed")
WELL_FORMED = tuple(c for c in P.SINGLE_IDS if not c.startswith("bad/"))


def _squash(text):
    return re.sub(r"\s+", " ", text)


@pytest.mark.parametrize("name", sorted(P.SOURCE_PINS))
def test_formulas_stand_in_the_source(name):
    src = _squash(open(os.path.join(CSRC, name)).read())
    for literal in P.SOURCE_PINS[name]:
        assert _squash(literal) in src, f"{name} no longer says: {literal}"


def test_rows_waves_against_the_row_launch_rules():
    # split while tiles <= 256; four waves up to 1,024 tiles; eight beyond (rows_split, rows_blocks)
    assert [P.rows_waves((n,)) for n in (0, 1, 4096, 4097, 16384, 16385)] == [4, 4, 4, 4, 4, 8]
    assert P.rows_waves((64, P.BIG_C, 3)) == 8 and P.rows_waves((4096, 500, 4)) == 4 and P.rows_waves((32768, 500, 4)) == 8


# ---- 2. plain statements -----------------------------------------------------------------------------------------------------------
def _segments(ptr, values):
    return [frozenset(values[ptr[v]:ptr[v + 1]].tolist()) for v in range(len(ptr) - 1)]


@pytest.mark.parametrize("cid", WELL_FORMED)
def test_single_restatement_is_plain_numpy(cid):
    st = P.single(cid)
    C, V, K = st[7:]
    (rows1, cols1), (rows2, cols2), coef = st[1], st[5], st[2].reshape(-1)
    p = P.expected_case(cid)
    assert np.array_equal(p["l_ptr0"], np.searchsorted(rows1, np.arange(C + 1))) and np.array_equal(p["l_ptr1"], np.searchsorted(rows2, np.arange(K + 1)))
    assert np.array_equal(p["inds0"], st[1].reshape(-1)) and np.array_equal(p["inds1"], st[5].reshape(-1)) and not p["alt"]["l_ptr0"]
    deg = np.bincount(cols1, minlength=V)
    assert np.array_equal(p["vcount"], deg) and np.array_equal(p["cursor"], deg)
    assert np.array_equal(p["v_ptr"], np.concatenate([[0], np.cumsum(deg)]))
    perm = np.argsort(cols1, kind="stable")
    long = np.repeat(deg > P.MAX_DEG, deg)
    assert np.array_equal(p["v_oth"], np.where(long, 0, rows1[perm])) and np.array_equal(p["v_coef"], np.where(long, np.float32(0), coef[perm]))
    assert _segments(p["v_ptr"], p["v_pos"]) == _segments(p["v_ptr"], perm)
    assert p["flags"].tolist() == [0, 0, 0, int(long.any())] and p["zeroed"] == np.nonzero(deg > P.MAX_DEG)[0].tolist()
    assert np.unique(st[2]).size == st[2].size and (np.unique(st[6]).size == st[6].size or cid.startswith("twins/"))   # distinct coefficients
    P.forward_gathers(p, C, V, K)


@pytest.mark.parametrize("cid", [c for c in P.UNION_IDS if c != "ib/bad"])
def test_union_restatement_is_plain_numpy(cid):
    states, forced = P.union(cid)
    p = P.expected_case(cid)
    tab = P.union_table([(s[7], s[8], s[9], s[1].shape[1], s[5].shape[1]) for s in states])
    rows1 = np.concatenate([s[1][0] + tab[0][i] for i, s in enumerate(states)])
    cols1 = np.concatenate([s[1][1] + tab[1][i] for i, s in enumerate(states)])
    rows2 = np.concatenate([s[5][0] + tab[2][i] for i, s in enumerate(states)])
    cols2 = np.concatenate([s[5][1] + tab[1][i] for i, s in enumerate(states)])
    coef = np.concatenate([s[2].reshape(-1) for s in states])
    Ct, Vt, Kt = (int(x) for x in tab[:3, -1])
    assert np.array_equal(p["left"], rows1) and np.array_equal(p["var0"], cols1) and np.array_equal(p["var1"], cols2)
    assert np.array_equal(p["iota"], np.arange(rows1.size)) and not p["flags"].any() and not p["alt"]["l_ptr0"] and not p["alt"]["l_ptr1"]
    assert np.array_equal(p["l_ptr0"], np.searchsorted(rows1, np.arange(Ct + 1))) and np.array_equal(p["l_ptr1"], np.searchsorted(rows2, np.arange(Kt + 1)))
    perm = np.argsort(cols1, kind="stable")
    assert np.array_equal(p["v_ptr"], np.concatenate([[0], np.cumsum(np.bincount(cols1, minlength=Vt))]))
    assert np.array_equal(p["v_oth"], rows1[perm]) and np.array_equal(p["v_coef"], coef[perm])
    if forced:
        want = np.concatenate([fi[1][np.argsort(fi[0], kind="stable")] + tab[1][i] for i, (fi, _, _) in enumerate(forced)])
        assert np.array_equal(p["f_col"], want)
    P.union_gathers(p, [(s[7], s[8], s[9], s[1].shape[1], s[5].shape[1]) for s in states])


# ---- 3. every case on its seam -----------------------------------------------------------------------------------------------------
def _launch(cid):
    st = P.single(cid)
    return P.launch_single(st[7], st[8], st[9], st[1].shape[1], st[5].shape[1]), st


def test_count_cases_sit_on_block_and_trip_seams():
    # (threads, blocks, where the closing position i == E runs): one block with the closing position, the first position of block
    # 1, the last position of a one-trip launch, the first position of the second trip
    want = {"count/E1/0": (256, 1, (0, 0, 0)), "count/E1/1": (256, 1, (0, 1, 0)), "count/E1/254": (256, 1, (0, 254, 0)),
            "count/E1/255": (256, 1, (0, 255, 0)), "count/E1/256": (256, 2, (1, 0, 0)), "count/E1/257": (256, 2, (1, 1, 0)),
            "count/E1/8190": (256, 32, (31, 254, 0)), "count/E1/8191": (256, 32, (31, 255, 0)), "count/E1/8192": (256, 32, (0, 0, 1)),
            "count/E1/8193": (256, 32, (0, 1, 1)),
            "count/E1/512/510": (512, 1, (0, 510, 0)), "count/E1/512/511": (512, 1, (0, 511, 0)), "count/E1/512/512": (512, 2, (1, 0, 0)),
            "count/E1/512/513": (512, 2, (1, 1, 0)), "count/E1/512/16382": (512, 32, (31, 510, 0)), "count/E1/512/16383": (512, 32, (31, 511, 0)),
            "count/E1/512/16384": (512, 32, (0, 0, 1)), "count/E1/512/16385": (512, 32, (0, 1, 1))}
    assert set(want) == {c for c in P.SINGLE_IDS if c.startswith("count/E1/")}
    for cid, (nt, nb, where) in want.items():
        L, st = _launch(cid)
        E1 = st[1].shape[1]
        assert (L["count_nt"], L["blocks0"], P.count_where(E1, nt, nb)) == (nt, nb, where), cid
    want2 = {0: (1, (0, 0, 0)), 1: (1, (0, 1, 0)), 2046: (8, (7, 254, 0)), 2047: (8, (7, 255, 0)), 2048: (8, (0, 0, 1)), 2049: (8, (0, 1, 1))}
    for E2, (nb, where) in want2.items():
        L, st = _launch(f"count/E2/{E2}")
        assert (L["count_nt"], L["blocks1"], P.count_where(E2, 256, nb)) == (256, nb, where), E2


def test_row_cases_leave_the_rows_they_name_empty():
    p, st = P.expected_case("rows/first_empty"), P.single("rows/first_empty")
    assert (p["l_ptr0"][:8] == 0).all() and p["l_ptr0"][8] > 0 and (p["l_ptr1"][:3] == 0).all()
    p, st = P.expected_case("rows/last_empty"), P.single("rows/last_empty")
    assert (p["l_ptr0"][-9:] == 500).all() and st[1][0].max() < st[7] - 9 and (p["l_ptr1"][-3:] == 9).all() and st[5][0].max() < st[9] - 3
    # the position that fills a run of empty rows is the first of a block / of the second trip
    for cid, rows, i in (("rows/run_at_block", range(100, 105), 256), ("rows/run_at_trip", range(300, 304), 8192)):
        L, st = _launch(cid)
        p = P.expected_case(cid)
        assert len(rows) >= 3 and all(p["l_ptr0"][r] == i and p["l_ptr0"][r + 1] == i for r in rows), cid
        assert P.count_where(i, L["count_nt"], L["blocks0"])[:2] == (i // 256 % 32, 0) and L["count_nt"] == 256
        assert P.count_where(i, 256, L["blocks0"])[2] == (1 if i == 8192 else 0) and st[1][0][i - 1] < rows[0] <= rows[-1] < st[1][0][i]
    p = P.expected_case("rows/one_row")
    assert set(p["l_ptr0"].tolist()) == {0, 500} and p["l_ptr0"][123] == 0 and p["l_ptr0"][124] == 500
    assert P.single("rows/C1")[7] == 1 and P.expected_case("rows/C1")["l_ptr0"].tolist() == [0, 30]
    assert P.single("rows/K1")[9] == 1 and P.expected_case("rows/K1")["l_ptr1"].tolist() == [0, 9]


def test_scan_cases_sit_on_chunk_and_form_seams():
    per256 = {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3, 4095: 16, 4096: 16}
    for V, per in per256.items():
        L, st = _launch(f"scan/256/V{V}")
        assert L["place_fused"] and L["order_fused"] and L["place_nt"] == 256 and P.scan_where(V - 1, V, 256)[3] == per, V
        assert L["names"][1].startswith("k_infer_s2") and L["names"][2].startswith("k_infer_s3")
    per1024 = {1: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2048: 2, 2049: 3, 4096: 4}
    for V, per in per1024.items():
        L, st = _launch(f"scan/1024/V{V}")
        assert not L["place_fused"] and L["order_fused"] and L["place_nt"] == 1024 and P.scan_where(V - 1, V, 1024)[3] == per, V
        assert L["names"][1:] == ["k_iplan_place", "k_infer_s3 (conv row program + plan: order)"] and L["order_groups"] == 32
    for V, per in {4097: 5, 32767: 32, 32768: 32}.items():
        L, st = _launch(f"scan/1024/big/V{V}")
        assert L["names"][1:] == ["k_iplan_place", "k_iplan_order"] and P.scan_where(V - 1, V, 1024)[3] == per and V <= P.MAX_VARS
    assert 4 * (P.MAX_VARS + 1) > 128 * 1024 - 64 * 4                     # the scan's LDS at its limit
    # empty variables: the first nine, the last nine, and across the ends of thread chunks (per = 4), of a wave's chunks among them
    deg = {k: np.bincount(P.single(f"scan/256/{k}")[1][1], minlength=1000) for k in ("empty_start", "empty_end", "empty_chunks", "one_var")}
    assert not deg["empty_start"][:9].any() and deg["empty_start"][9:].all() and not deg["empty_end"][-9:].any() and deg["empty_end"][:-9].all()
    for t in (1, 63, 64, 200):
        a, b = P.scan_where(4 * t - 1, 1000, 256), P.scan_where(4 * t, 1000, 256)
        assert (a[0], a[2], b[0], b[2]) == (t - 1, 3, t, 0) and not deg["empty_chunks"][4 * t - 2:4 * t + 2].any()
    assert P.scan_where(255, 1000, 256)[1] == 0 and P.scan_where(256, 1000, 256)[1] == 1      # 4 * 64: the first chunk of wave 1
    assert deg["one_var"][517] == 1500 and deg["one_var"].sum() == 1500


def test_place_and_order_cases_sit_on_trip_seams():
    for form, fused in (("fused", True), ("alone", False)):
        for E1, trip in ((65536, 0), (65537, 1)):
            L, st = _launch(f"place/trip/{form}/{E1}")
            assert L["place_fused"] == fused and st[1].shape[1] == E1 and P.place_where(E1 - 1, L)[2] == trip
            assert P.place_where(E1 - 1, L)[:2] == ((0, 0) if trip else (L["place_blocks"] - 1, L["place_nt"] - 1))
    # the fused order blocks: 16 lane groups per block of a 4-wave launch, 32 of an 8-wave one; 48 blocks at the most
    for V, groups, blocks, last in ((16, 16, 1, (0, 15, 0)), (17, 16, 2, (1, 0, 0)), (768, 16, 48, (47, 15, 0)), (769, 16, 48, (0, 0, 1)),
                                    (32, 32, 1, (0, 31, 0)), (33, 32, 2, (1, 0, 0)), (1536, 32, 48, (47, 31, 0)), (1537, 32, 48, (0, 0, 1))):
        L, st = _launch(f"order/trip/V{V}")
        assert L["order_fused"] and (L["order_groups"], L["order_blocks"], P.order_where(V - 1, L)) == (groups, blocks, last), V
        assert np.bincount(st[1][1], minlength=V)[V - 1] > 0 or V % 3 == 2                    # (degrees 1, 0, 2 in turn)
    seam = {0, 3, 4, 5, 16, 17, 255, 256, 257}
    for cid, first in (("order/trip/degs/4w", 768), ("order/trip/degs/8w", 1536)):
        L, st = _launch(cid)
        deg = np.bincount(st[1][1], minlength=st[8])
        second = [v for v in range(st[8]) if P.order_where(v, L)[2] == 1]
        assert second and second[0] == first and seam <= set(deg[second].tolist()), cid
    L, st = _launch("order/2048")
    deg = np.bincount(st[1][1], minlength=st[8])
    last_block = [v for v in range(st[8]) if P.order_where(v, L)[0] == 2047]
    assert not L["order_fused"] and L["order_blocks"] == 2048 and st[8] == P.MAX_VARS and P.order_where(st[8] - 1, L) == (2047, 15, 0)
    assert seam <= set(deg[last_block].tolist())


def test_degree_cases_take_the_paths_they_name():
    for cid, degs in (("deg", P.SEAM_DEGS), ("deg/2049", P.SEAM_DEGS + (2049,))):
        st, p = P.single(cid), P.expected_case(cid)
        assert np.bincount(st[1][1], minlength=st[8]).tolist() == list(degs)
        path = dict(zip(degs, p["path"]))
        assert path[256] == "lds" and path[257] == "global" and path[2048] == "global" and path[255] == "lds" and path[1] == "lds"
        assert p["zeroed"] == ([19] if cid == "deg/2049" else []) and p["flags"].tolist() == [0, 0, 0, int(cid == "deg/2049")]
    p = P.expected_case("deg/2049")
    seg = slice(p["v_ptr"][19], p["v_ptr"][20])
    assert not p["v_oth"][seg].any() and not p["v_coef"][seg].any() and seg.stop - seg.start == 2049


@pytest.mark.parametrize("K", (1, 2, 257, 1025, 4096))
def test_twins_are_identical_cuts(K):
    st = P.single(f"twins/K{K}")
    pairs = P.twin_pairs(f"twins/K{K}")
    assert pairs == [(a, b) for a, b in ((0, K - 1), (255, 256), (1023, 1024), (4094, 4095)) if a < b < K] and (pairs or K == 1)
    for a, b in pairs:
        assert np.array_equal(st[4][a], st[4][b]) and np.array_equal(st[5][1, 2 * a:2 * a + 2], st[5][1, 2 * b:2 * b + 2])
        assert np.array_equal(st[6][2 * a:2 * a + 2], st[6][2 * b:2 * b + 2]) and (st[5][0, 2 * a:2 * a + 2] == a).all()


@pytest.mark.parametrize("cid", [c for c in P.SINGLE_IDS if c.startswith("bad/")])
def test_bad_cases_flag_and_stay_inside(cid):
    _, which, value, where = cid.split("/")
    st, p = P.single(cid), P.expected_case(cid)
    clean = P.random_state(60, P.BAD_C, P.BAD_V, P.BAD_K, P.BAD_E1, P.BAD_E2)
    lst, row = (1, 0 if which == "cons_row" else 1) if which.startswith("cons") else (5, 0 if which == "cut_row" else 1)
    at = {"first": 0, "last": st[lst].shape[1] - 1, "block_end": 255}[where]
    changed = np.argwhere(st[lst] != clean[lst])
    assert changed.tolist() == [[row, at]] and P.count_where(255, 256, 3)[:2] == (0, 255)
    bad = int(st[lst][row, at])
    size = {"cons_row": P.BAD_C, "cons_var": P.BAD_V, "cut_row": P.BAD_K, "cut_var": P.BAD_V}[which]
    assert bad == (-3 if value == "neg" else size)
    rows = st[lst][0]
    unsorted = int((np.diff(rows) < 0).any())
    assert p["flags"][0] == 1 and p["flags"][1 if lst == 1 else 2] == unsorted and p["flags"][3] == 0
    if row == 0:
        assert unsorted == (0 if (value, where) in (("neg", "first"), ("size", "last")) else 1)
        assert np.array_equal(p["inds0"], st[1].reshape(-1)) and np.array_equal(p["inds1"], st[5].reshape(-1))       # row ids stay as uploaded
    else:
        E = st[lst].shape[1]
        assert p["inds0" if lst == 1 else "inds1"][E + at] == 0                  # the variable id is replaced
    # every plan entry inside its array, every gather of the forward inside its table
    for name, n in (("l_ptr0", P.BAD_E1), ("l_ptr1", P.BAD_E2), ("v_ptr", P.BAD_E1)):
        assert p[name].min() >= 0 and p[name].max() <= n
        for vals in p["alt"].get(name, {}).values():
            assert min(vals) >= 0 and max(vals) <= n
    assert p["v_oth"].min() >= 0 and p["v_oth"].max() < P.BAD_C and sorted(p["v_pos"].tolist()) == list(range(P.BAD_E1))
    P.forward_gathers(p, P.BAD_C, P.BAD_V, P.BAD_K)


def test_union_cases_sit_on_their_seams():
    for S in (1, 2, 3, 17, 64):
        assert len(P.union(f"ib/S{S}")[0]) == S <= P.IB_MAX_STATES
    st, _ = P.union("ib/empty")
    e1, e2, c = [s[1].shape[1] for s in st], [s[5].shape[1] for s in st], [s[7] for s in st]
    assert (e1[1], e2[3], c[4], e1[4], e1[5]) == (0, 0, 0, 0, 0) and all(e1[i] and e2[i] and c[i] for i in (0, 2, 6))
    p = P.expected_case("ib/empty")
    tab = P.union_table([(s[7], s[8], s[9], s[1].shape[1], s[5].shape[1]) for s in st])
    assert tab[0][4] == tab[0][5] and p["l_ptr0"][tab[0][4]] == tab[3][4] == tab[3][6]     # a state without rows shares its neighbour's entry
    # item 255 is state 0's closing position (block 0's last thread), item 256 state 1's first edge (block 1's first)
    st, _ = P.union("ib/seam")
    assert st[0][1].shape[1] == 255 and st[1][1].shape[1] > 0
    items = P.expected_case("ib/seam")["items"]
    assert P.unpack_where(255, items)[:2] == (0, 255) and P.unpack_where(256, items)[:2] == (1, 0)
    for total, trip in ((262144, 0), (262145, 1)):
        p = P.expected_case(f"ib/trip/{total}")
        assert p["items"] == total and P.unpack_launch(total) == 1024 and P.unpack_where(total - 1, total)[2] == trip
    st, forced = P.union("ib/forced")
    tab = P.union_table([(s[7], s[8], s[9], s[1].shape[1], s[5].shape[1]) for s in st], [(f[2], f[0].shape[1]) for f in forced])
    assert tab[6].tolist() == [0, 6, 6, 6, 15, 15, 18]                   # ties in the search: states without forced entries
    p = P.expected_case("ib/bad")
    assert p["flags"].tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
    P.union_gathers(p, [(s[7], s[8], s[9], s[1].shape[1], s[5].shape[1]) for s in P.union("ib/bad")[0]])


# ---- 4. defects -------------------------------------------------------------------------------------------------------------------
# defect -> [(case, what it must change: names of plan outputs, or OutOfBounds where the bounds check must fire)]
OOB = "OutOfBounds"
DEFECT_TABLE = {
    "count_lt": [("count/E1/255", {"l_ptr0"}), ("count/E1/8191", {"l_ptr0"}), ("count/E1/512/16383", {"l_ptr0"}), ("count/E2/2047", {"l_ptr1"}),
                 ("rows/last_empty", {"l_ptr0", "l_ptr1"}), ("count/E1/0", {"l_ptr1"})],
    "per_floor": [("scan/256/V257", {"v_ptr"}), ("scan/256/V255", OOB), ("scan/1024/V1025", {"v_ptr"}), ("scan/1024/big/V4097", {"v_ptr"})],
    "no_pre_n": [("scan/256/V256", {"v_ptr"}), ("scan/1024/V1024", {"v_ptr"}), ("scan/1024/big/V32768", {"v_ptr"})],
    "no_wave_base": [("scan/256/V257", {"v_ptr", "v_oth", "v_coef"}), ("scan/1024/V2049", {"v_ptr", "v_oth", "v_coef"}),
                     ("scan/256/empty_chunks", {"v_ptr", "v_oth", "v_coef"})],
    "pad_zero": [("deg", OOB), ("order/trip/degs/4w", OOB)],
    "lds_lt": [("deg", {"path"})],
    "maxdeg_ge": [("deg", {"v_oth", "v_coef", "flags", "zeroed"})],
    "order_one_trip": [(f"order/trip/V{V}", {"v_oth", "v_coef"}) for V in (769, 1537)]
                      + [("order/trip/degs/4w", {"v_oth", "v_coef"}), ("order/trip/degs/8w", {"v_oth", "v_coef"})],
    "place_one_trip": [("place/trip/fused/65537", OOB), ("place/trip/alone/65537", OOB)],
    "no_clamp_lptr": [("bad/cons_row/neg/first", OOB), ("bad/cons_row/neg/block_end", OOB), ("bad/cut_row/neg/last", OOB)],
    "no_clamp_var": [("bad/cons_var/neg/first", OOB), ("bad/cons_var/size/last", OOB), ("bad/cut_var/size/block_end", OOB),
                     ("bad/cut_var/neg/first", OOB)],
    "no_clamp_voth": [("bad/cons_row/neg/block_end", OOB), ("bad/cons_row/size/first", OOB)],
    "ib_lptr0_from_data": [("ib/bad", {"l_ptr0"})],
    "ib_rows_from_0": [("ib/bad", {"l_ptr0"})],
    "ib_search_lt": [("ib/S2", OOB), ("ib/seam", OOB), ("ib/forced", OOB)],
    "ib_no_clamp_var": [("ib/bad", {"var0", "v_ptr"})],
    "ib_no_clamp_left": [("ib/bad", {"left", "v_oth"})],
}


def _differing(a, b):
    out = set()
    for k in PLAN_KEYS:
        if k in a:
            x, y = a[k], b[k]
            same = x == y if isinstance(x, list) else np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x,
                                                                     y.view(np.int32) if y.dtype == np.float32 else y)
            if not same:
                out.add(k)
    return out


def _defective(cid, defect):
    """The defective restatement's outputs with the gathers the forward would make through them."""
    if cid in P.SINGLE:
        st = P.single(cid)
        p = P.expected_single(st, {defect})
        P.forward_gathers(p, *st[7:])
    else:
        states, forced = P.union(cid)
        p = P.expected_union(states, P.packed_forced(states, forced), {defect})
        P.union_gathers(p, [(s[7], s[8], s[9], s[1].shape[1], s[5].shape[1]) for s in states])
    return p


def test_the_defect_table_covers_the_defect_list():
    assert set(DEFECT_TABLE) == set(P.DEFECTS) and not P.ACTIVE


@pytest.mark.parametrize("defect", P.DEFECTS)
def test_each_defect_changes_a_named_output_of_a_named_case(defect):
    for cid, want in DEFECT_TABLE[defect]:
        good = P.expected_case(cid)
        if want == OOB:
            with pytest.raises(P.OutOfBounds):
                _defective(cid, defect)
        else:
            try:
                got = _differing(good, _defective(cid, defect))
            except P.OutOfBounds:
                continue                        # (the outputs differ so far that a later step leaves its arrays)
            assert want <= got, (defect, cid, got)


# ---- 5. degenerate states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,leaves", [("V0_E1", True), ("C0_E1", True), ("V0_E2", True), ("K0_E2", False)])
def test_degenerate_states_leave_their_arrays(name, leaves):
    """Edges with no rows or no variables to point at: the count step rewrites every variable id to 0 and the order step clamps
    every row id to 0, and the forward then gathers row 0 of a table without rows.  Three of the four leave an array (the cut
    list of a state without cuts does not: no cut row, no edge pass); all four are refused on the host, as gcnn_infer_batch does."""
    from gcnn_cut_selector_amd.infer import edges_without_nodes
    st = P.degenerate(name)
    key = (st[7], st[8], st[9], st[1].shape[1], st[5].shape[1])
    assert key == P.DEGENERATE[name] and edges_without_nodes(key)

    def run():
        p = P.expected_single(st)
        assert p["flags"][0] == 1
        P.forward_gathers(p, *st[7:])
    if leaves:
        with pytest.raises(P.OutOfBounds):
            run()
    else:
        run()
    assert not edges_without_nodes((5, 4, 3, 6, 4)) and not edges_without_nodes((0, 0, 0, 0, 0)) and not edges_without_nodes((0, 3, 0, 0, 0))
