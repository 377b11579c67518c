"""Cut selection on the device at the edges of k_sel_pairs / k_sel_filter (GPU): pivots across more than one LDS chunk of 8,192
columns, more pivot rows than the 65,535 blocks of the launch, and parallelisms and scores exactly on a threshold.  The cases are
tests/selcases.py (what each is and why it discriminates: tests/test_selcases.py, on the host); here `(order, n_kept)` of the device
is compared with the restatement tests/cutsel_restate.py by `np.array_equal` and `==`.  There is no tolerance anywhere: the random
parts keep the margins of test_gpu_select.py (1e-9 around both thresholds, one float32 ulp around t), the tie cases are dyadic and
exact in any summation order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
import selcases as S  # noqa: E402
from gcnn_cut_selector_amd import ops  # noqa: E402
from gcnn_cut_selector_amd.graph import BipartiteGraph  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401
from test_gpu_select import forced_rows, restate, state_with_cuts  # noqa: E402


def device_select(case, dev, as_union):
    """`ops.select_cuts` on a case: (order [total cuts], n_kept [samples]) as host arrays."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    g = BipartiteGraph(t(np.stack([case["rows"], case["cols"]])), t(case["vals"]), case["K"], case["V"])
    forced = None
    if case["F"]:
        forced = tuple(t(a) for a in ops.pack_rows(case["forced_inds"], case["forced_vals"], case["F"], case["V"]))
    if as_union:
        order, n_kept = ops.select_cuts(t(case["q"]), g, t(case["c_off"]), forced, t(case["f_off"]) if case["F"] else None,
                                        p_max=case["p_max"], p_max_ub=case["p_max_ub"], max_cuts=case["max_cuts"])
    else:
        assert len(case["samples"]) == 1
        order, n_kept = ops.select_cuts(t(case["q"]), g, None, forced, p_max=case["p_max"], p_max_ub=case["p_max_ub"])
    return order.cpu().numpy(), n_kept.cpu().numpy()


def first_wrong(case, order, n_kept):
    """None, or (sample, its first global pivot row, got n_kept, wanted n_kept) of the first sample the device got wrong."""
    c_off = case["c_off"]
    for s, (want_order, want_n, _) in enumerate(S.expected(case)):
        if not (np.array_equal(order[c_off[s]:c_off[s + 1]], want_order) and int(n_kept[s]) == want_n):
            return s, int(c_off[s] + case["f_off"][s]), int(n_kept[s]), want_n
    return None


def wrong_pairs(case, order, n_kept):
    """The hand-placed pairs of the chunk case whose partner the device judged differently (for the failure message)."""
    kept = set(order[:int(n_kept)].tolist())
    return [(p["name"], q["idx"]) for p in case["pairs"] for q in p["partners"] if (q["idx"] in kept) == q["removed"]]


# ---- A: more than one column chunk -------------------------------------------------------------------------------------------------
def test_pivots_across_column_chunks(dev):
    case = S.chunk_case()
    order, n_kept = device_select(case, dev, as_union=False)
    assert order.dtype == np.int32 and n_kept.shape == (1,)
    want_order, want_n, _ = S.expected(case)[0]
    assert np.array_equal(order, want_order) and int(n_kept[0]) == want_n, ("pairs judged wrongly:", wrong_pairs(case, order, n_kept[0]))


def test_pivots_across_column_chunks_inside_a_union(dev):
    case = S.chunk_union_case()
    order, n_kept = device_select(case, dev, as_union=True)
    assert first_wrong(case, order, n_kept) is None, first_wrong(case, order, n_kept)


def test_columns_outside_the_variables_take_no_part(dev):
    """include/gcnn_hip.h: "Entries whose column lies outside [0, n_vars) take no part" -- neither in the pivot's span nor in a
    product.  Pivot and partner share the column n_vars + 5 (and -1, what the batched unpack writes for a bad id); inside the
    variables they share one column with product 0.125 < p_max.  Counted, the outside column would give 0.875 > p_max_ub.  Its LDS
    slot (106) lies inside the chunk either way."""
    V = 9000
    cut = [S._row([(V - 101, 1.0), (V + 5, 1.0), (-1, 1.0)]), S._row([(V - 101, 0.125), (V + 5, 0.75), (-1, 0.5)])]
    ptr = np.array([0, 3, 6], np.int32)
    col = np.concatenate([c for c, _ in cut]).astype(np.int32)
    val = np.concatenate([v for _, v in cut])
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    g = BipartiteGraph.from_plan(2, V, t(ptr), t(col), t(val), torch.zeros(V + 1, dtype=torch.int32, device=dev), none,
                                 torch.zeros(0, device=dev))
    fcol, fval = S._row([(V - 101, 0.25), (V + 5, 1.0), (-1, 1.0)])     # a forced pivot: 0.25 and 0.03125 inside, 1.25 and 0.78 counted
    for forced in (None, (t(ptr[:2]), t(fcol.astype(np.int32)), t(fval))):
        order, n_kept = ops.select_cuts(t(np.float32([1.0, 0.95])), g, None, forced, p_max=0.3, p_max_ub=0.6)
        assert order.cpu().tolist() == [0, 1] and int(n_kept.cpu()[0]) == 2


# ---- B: more pivot rows than blocks ------------------------------------------------------------------------------------------------
def test_more_pivot_rows_than_blocks(dev):
    case = S.grid_case()
    assert case["K"] + case["F"] > S.GRID
    order, n_kept = device_select(case, dev, as_union=True)
    bad = first_wrong(case, order, n_kept)
    if bad is not None:
        s, row, got, want = bad
        where = "beyond" if s in case["beyond"] else "astride" if s in case["straddle"] else "below"
        pytest.fail(f"sample {s} (pivot rows from {row}: {where} row {S.GRID}): n_kept {got}, expected {want}; planted pair in "
                    f"sample {case['alias'][2]}")


# ---- C: exact ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", S.TIE_VARIANTS)
def test_values_exactly_on_a_threshold(dev, variant):
    case = S.tie_case(variant)
    order, n_kept = device_select(case, dev, as_union=False)
    want_order, want_n, _ = S.expected(case)[0]
    assert (want_order.tolist(), want_n) == case["want"]
    assert np.array_equal(order, want_order) and int(n_kept[0]) == want_n, (order.tolist(), int(n_kept[0]), case["want"])


# ---- one full-size capfac state through the model's paths ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    return make_model(90, dev)[0]


@pytest.fixture(scope="module")
def capfac(dev, model):
    """A BASELINE-size capfac state (10,100 variables) with 100 planted cuts over all of them and two forced rows.  Built once."""
    return clear_state(model, "capfac", 0, 100, 2, 1.0, 1000)


def clear_state(model, problem, index, K, F, scale, seed0):
    """(inputs, cut edges, forced rows, the single call's result) from the first of 20 seeds whose restatement -- fed the device's
    scores -- has clear margins."""
    for seed in range(seed0, seed0 + 20):
        rng = np.random.default_rng(seed)
        inp, edges = state_with_cuts(problem, index, rng, K, scale=scale)
        forced = forced_rows(rng, F, inp[8], edges)
        res = model.select_cuts(inp, (forced[0], forced[1], F))
        if R.margins_ok(restate(res.scores, edges, K, inp[8], forced, 0.1, 0.5)[2], 0.1, 0.5):
            return inp, edges, forced, res
    pytest.fail("no seed with clear margins")


def check_against_restatement(res, edges, K, V, forced):
    order, n, rec = restate(res.scores, edges, K, V, forced, 0.1, 0.5)
    assert R.margins_ok(rec, 0.1, 0.5)
    assert np.array_equal(res.order, order) and res.n_kept == n
    return order, n


def test_full_size_capfac_state_through_the_model_paths(dev, model, capfac):
    inp, edges, forced, single = capfac
    K, V = 100, inp[8]
    assert V > S.CH
    order, n = check_against_restatement(single, edges, K, V, forced)
    assert n < K
    rows, cols, _ = edges
    span = np.array([np.ptp(cols[rows == k]) if (rows == k).any() else 0 for k in range(K)])
    assert (span[order[:n - 1]] >= S.CH).sum() >= 1, "no consulted pivot spans more than one chunk"
    f = (forced[0], forced[1], 2)
    general = model.select_cuts(tuple(torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x for x in inp), f)
    check_against_restatement(general, edges, K, V, forced)
    assert np.array_equal(np.asarray(general.scores), np.asarray(single.scores))
    small, small_edges, small_forced, _ = clear_state(model, "setcov", 1, 40, 1, 0.3, 2000)
    many = model.select_cuts_many([inp, small], [f, (small_forced[0], small_forced[1], 1)])
    check_against_restatement(many[0], edges, K, V, forced)
    check_against_restatement(many[1], small_edges, 40, small[8], small_forced)
    assert np.array_equal(many[0].order, single.order) and many[0].n_kept == single.n_kept
