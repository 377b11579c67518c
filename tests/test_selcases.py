"""The cut-selection edge cases of tests/selcases.py, checked on the host against the restatement alone: every case is what it
claims to be, and a selection with the defect a case was built against gives a different (order, n_kept) -- so the device test
that runs the case (tests/test_gpu_select_edges.py) can tell the two apart.  CPU only."""
import numpy as np
import pytest

import cutsel_restate as R
import selcases as S

# name -> per partner, the products it makes with the pivot in each chunk of the pivot's columns (chunks start at the pivot's mn)
F32 = lambda x: float(np.float32(x))  # noqa: E731
PARTIALS = {
    "span1": [{0: F32(0.8)}],
    "span2": [{1: F32(0.8)}],
    "seam": [{0: F32(0.8)}, {1: F32(0.8)}, {1: F32(0.8)}, {2: F32(0.8)}],
    "sum": [{0: F32(0.2), 1: F32(0.2)}],
    "cancel": [{0: F32(0.4), 2: -F32(0.4)}],
    "alias": [{}],
    "top": [{1: 0.5}],
    "dup": [{1: 0.5}],
    "forced_sum": [{0: F32(0.2), 1: F32(0.2)}],
    "forced_cancel": [{0: F32(0.4), 2: -F32(0.4)}],
}
SPANS = {"span1": S.CH - 1, "span2": S.CH, "seam": 2 * S.CH, "sum": S.CH + 10, "cancel": 2 * S.CH + 20, "alias": S.CH + 50,
         "top": S.CH + 1000, "dup": S.CH, "forced_sum": S.CH + 10, "forced_cancel": 2 * S.CH + 20}


def with_pair_value(P, pair, partner, value):
    """The parallelisms with the one between `pair`'s pivot and `partner` replaced."""
    P_cc, P_fc = P[0].copy(), P[1].copy()
    kind, i = pair["pivot"]
    if kind == "cut":
        P_cc[i, partner["idx"]] = P_cc[partner["idx"], i] = value
    else:
        P_fc[i, partner["idx"]] = value
    return P_cc, P_fc


def test_the_variant_loop_with_default_comparisons_is_the_restatement():
    rng = np.random.default_rng(0)
    samples = [S.random_sample(rng, K, 16, F) for K, F in ((1, 0), (30, 2), (90, 1))]
    samples += [S.tie_case(v)["samples"][0] for v in S.TIE_VARIANTS]
    for thr in (S.B_THR, S.C_THR):
        for s in samples:
            P = S.parallelisms(s)
            assert S.same(S.select_variant(s["q"], P, *thr), S.restate_sample(s, *thr, P=P))


# ---- A ------------------------------------------------------------------------------------------------------------------------------
def test_chunk_pairs_have_the_span_chunks_and_partial_products_they_claim():
    case = S.chunk_case()
    sample, pairs = case["samples"][0], case["pairs"]
    assert (case["K"], case["V"], case["F"], case["max_cuts"]) == (S.A_K, S.A_V, 2, S.A_K) and (S.A_K + 63) // 64 == 3
    assert sorted(p["name"] for p in pairs) == sorted(PARTIALS)
    P = S.parallelisms(sample)
    order, n, _ = S.expected(case)[0]
    kept = set(order[:n].tolist())
    first_words = set()
    for p in pairs:
        kind, i = p["pivot"]
        cols = (sample["cut"] if kind == "cut" else sample["forced"])[i][0]
        assert cols.min() == p["mn"] and cols.max() - cols.min() == SPANS[p["name"]], p["name"]
        assert (cols.max() - cols.min()) // S.CH + 1 == p["n_chunks"], p["name"]
        if kind == "cut":
            first_words.add((i + 1) >> 6)
            assert i in kept, p["name"]
        assert len(p["partners"]) == len(PARTIALS[p["name"]])
        for partner, want in zip(p["partners"], PARTIALS[p["name"]]):
            j = partner["idx"]
            assert S.pair_partials(p, partner) == want, (p["name"], j)
            got = P[0][i, j] if kind == "cut" else P[1][i, j]
            assert got == abs(sum(want.values())), (p["name"], j)
            assert (j in kept) == (not partner["removed"]), (p["name"], j)
            assert kind == "forced" or j > i                      # the pivot is the row the kernel scatters: the lower index
    assert first_words == {0, 1, 2}                               # pivots whose first partner word is 0, 1 and 2
    by_name = {p["name"]: p for p in pairs}
    assert max(c for c, _ in by_name["top"]["entries"]) == S.A_V - 1
    assert by_name["top"]["mn"] + 2 * S.CH > S.A_V                # the last chunk is cut short by n_vars
    dup_cols = [c for c, _ in by_name["dup"]["entries"]]
    assert dup_cols.count(by_name["dup"]["mn"] + S.CH) == 2       # the duplicate sits on the first column of chunk 1
    alias = by_name["alias"]
    slot = lambda c: (c - alias["mn"]) % S.CH  # noqa: E731
    assert slot(alias["partners"][0]["entries"][0][0]) in {slot(c) for c, _ in alias["entries"]}


def test_chunk_random_fill_has_clear_margins_and_spans_chunks():
    seed, rejected = S.chunk_seed()
    assert 0 <= rejected <= seed < 20
    case = S.chunk_case()
    rec = S.expected(case)[0][2]
    assert R.margins_ok(rec, *S.A_THR)
    hand = {p["pivot"][1] for p in case["pairs"] if p["pivot"][0] == "cut"} | {q["idx"] for p in case["pairs"] for q in p["partners"]}
    wide = [k for k, (c, _) in enumerate(case["samples"][0]["cut"]) if k not in hand and c.size and c.max() - c.min() >= S.CH]
    assert len(wide) >= 30 and len(hand) == 21
    assert S.expected(case)[0][1] < S.A_K - 10                    # the random rows remove something as well
    union = S.chunk_union_case()
    assert union["c_off"][1] > 0 and union["f_off"][1] > 0 and union["v_off"][1] > 0 and len(union["samples"]) == 3
    assert all(R.margins_ok(rec, *S.A_THR) for _, _, rec in S.expected(union))
    assert S.same(S.expected(union)[1], S.expected(case)[0])


def test_every_chunk_pair_tells_a_defective_sum_from_the_correct_one():
    case = S.chunk_case()
    sample = case["samples"][0]
    P = S.parallelisms(sample)
    right = S.expected(case)[0]
    checked = 0
    for p in case["pairs"]:
        for partner in p["partners"]:
            parts = S.pair_partials(p, partner)
            wrong = [abs(sum(v for c, v in parts.items() if c != drop)) for drop in parts]       # one chunk's products dropped
            if len(parts) > 1:
                wrong.append(abs(parts[max(parts)]))                                             # the last chunk's alone (=, not +=)
            if p["name"] == "alias":
                wrong.append(F32(0.8))                                                           # the slot still holds chunk 0
            if p["name"] == "dup":
                wrong.append(0.25)                                                               # one of the two entries
            assert wrong, p["name"]
            for value in wrong:
                got = S.restate_sample(sample, *S.A_THR, P=with_pair_value(P, p, partner, value))
                assert not S.same(got, right), (p["name"], partner["idx"], value)
                checked += 1
    assert checked >= 20


# ---- B ------------------------------------------------------------------------------------------------------------------------------
def test_grid_case_has_a_second_trip_that_matters():
    case = S.grid_case()
    n_rows = case["K"] + case["F"]
    assert 66000 <= n_rows <= 70000 and n_rows > S.GRID and case["V"] == S.B_SAMPLES * S.B_V
    sizes = np.diff(case["c_off"])
    assert sizes.min() >= 40 and sizes.max() <= 90 and (case["max_cuts"] + 63) // 64 == 2
    assert set(np.diff(case["f_off"]).tolist()) == {0, 1, 2}
    exp = S.expected(case)
    assert all(R.margins_ok(rec, *S.B_THR) for _, _, rec in exp)
    removing = [s for s, (_, n, _) in enumerate(exp) if n < sizes[s]]
    assert len(removing) > 0.9 * S.B_SAMPLES
    assert len(case["straddle"]) == 1
    s = case["straddle"][0]
    assert case["start"][s] < S.GRID < case["start"][s + 1] and case["beyond"][0] == s + 1
    assert len([s for s in case["beyond"] if s in set(removing)]) >= 20
    # the planted pair: the block whose first pivot is row ga takes cut 0 of sample b next
    a, ga, b = case["alias"]
    assert ga + S.GRID == case["start"][b] and b in case["beyond"]
    la = ga - case["start"][a]
    assert 0 <= la < sizes[a] - 1                                   # a cut with partners: the pivot is not skipped
    ca, cb0, cb1 = case["samples"][a]["cut"][la][0], case["samples"][b]["cut"][0][0], case["samples"][b]["cut"][1][0]
    assert (cb1[0] - cb0.min()) in set((ca - ca.min()).tolist()) and cb1.size == 1 and cb1[0] not in cb0
    Pb = S.parallelisms(case["samples"][b])
    assert Pb[0][0, 1] == 0.0
    stale = Pb[0].copy()
    stale[0, 1] = stale[1, 0] = 1.0
    assert not S.same(S.restate_sample(case["samples"][b], *S.B_THR, P=(stale, Pb[1])), exp[b])


# ---- C ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", S.TIE_VARIANTS)
def test_tie_case_is_exact_and_pins_each_comparison(variant):
    case = S.tie_case(variant)
    sample = case["samples"][0]
    P = S.parallelisms(sample)
    with_pivot = P[1][0, 1:] if variant.startswith("forced-") else P[0][0, 1:]
    assert np.all(with_pivot == case["P"])                         # dyadic: exact in any order, so == is meant
    assert list(case["P"]) == [0.25, 0.25 + 2.0 ** -20, 0.25 + 2.0 ** -20, 0.5, 0.5 + 2.0 ** -20]
    thr = S.C_THR
    right = S.restate_sample(sample, *thr, P=P)
    assert (right[0].tolist(), right[1]) == case["want"]
    q, t = sample["q"], case["t"]
    assert q[2] == t and q[4] > t and q[5] > t and q[1] < t and q[0] == case["q0"]
    kind = variant.split("-")[-1]
    if kind == "tform":
        assert S.t_float32_form(case["q0"]) == np.nextafter(t, np.float32(0)) == q[3]      # the two forms of t differ by one ulp
    else:
        assert S.t_float32_form(case["q0"]) == t
        assert q[3] == (t if kind == "equal" else np.nextafter(t, np.float32(0)))
    ge, le = np.greater_equal, np.less_equal
    assert not S.same(S.select_variant(q, P, *thr, gt_max=ge), right)
    assert not S.same(S.select_variant(q, P, *thr, gt_ub=ge), right)
    assert not S.same(S.select_variant(q, P, *thr, lt=le), right)
    if kind == "tform":
        assert not S.same(S.select_variant(q, P, *thr, threshold=S.t_float32_form), right)
