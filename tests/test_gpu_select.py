"""Cut selection on the device (GPU): `GCNN.select_cuts` (single call gcnn_infer_select, or prepare + forward + gcnn_select_cuts)
and `ops.select_cuts` (any quality vector, one workgroup per sample) against the NumPy restatement tests/cutsel_restate.py, fed
the device's own scores.  Every case asserts its margins: each parallelism the filter consulted lies more than 1e-9 from both
thresholds and each score more than one float32 ulp from the threshold t -- cases come from seeds that satisfy this."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
import launchnames  # noqa: E402
from gcnn_cut_selector_amd import _lib, ops, synthetic, utils  # noqa: E402
from gcnn_cut_selector_amd.graph import BipartiteGraph  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402
from test_select_build import SELECT, SELECT_NAMES  # noqa: E402

THRESHOLDS = [(0.1, 0.5), (0.0, 0.0), (0.9, 0.95)]


@pytest.fixture(scope="module")
def model(dev):
    return make_model(90, dev)[0]


def plant_rows(rng, K, V, extras=True):
    """K cut rows over V variables as (rows, cols, vals) lists: random unit rows, plus exact copies, scaled and sign-flipped copies,
    partial overlaps with P = 0.05 / 0.3 / 0.7 / 0.92, empty rows and split (duplicate) entries."""
    R_, C_, X_ = [], [], []
    bank = []
    for k in range(K):
        kind = rng.integers(0, 8) if (extras and k > 0) else 0
        if kind == 1 or kind == 2:                       # copy, scaled / sign-flipped copy of an earlier row
            cols, vals = bank[rng.integers(0, len(bank))]
            vals = vals * np.float32([1.0, -1.0, 2.0, -0.6][rng.integers(0, 4)])
        elif kind == 3 and V >= 4:                       # partial overlap: alpha * base + beta * (disjoint columns)
            cols0, vals0 = bank[rng.integers(0, len(bank))]
            alpha = [0.05, 0.3, 0.7, 0.92][rng.integers(0, 4)]
            free = np.setdiff1d(np.arange(V), cols0)
            if free.size == 0:
                cols, vals = cols0, vals0
            else:
                extra = rng.choice(free, size=min(free.size, int(rng.integers(1, 6))), replace=False)
                ev = rng.standard_normal(extra.size)
                ev = ev / np.linalg.norm(ev) * np.sqrt(1 - alpha * alpha)
                cols = np.concatenate([cols0, extra])
                vals = np.concatenate([alpha * vals0.astype(np.float64), ev]).astype(np.float32)
        elif kind == 4:                                  # empty row
            cols, vals = np.zeros(0, np.int64), np.zeros(0, np.float32)
        else:
            nnz = int(rng.integers(1, min(12, V) + 1))
            cols = np.sort(rng.choice(V, size=nnz, replace=False))
            v = rng.standard_normal(nnz)
            vals = (v / np.linalg.norm(v)).astype(np.float32)
        if cols.size:
            bank.append((cols, vals))
        if kind == 5 and cols.size:                      # one entry split in two: duplicate (row, col) entries add
            j = int(rng.integers(0, cols.size))
            half = np.float32(vals[j] * np.float32(0.5))
            cols = np.concatenate([cols, [cols[j]]])
            vals = np.concatenate([vals[:j], [half], vals[j + 1:], [np.float32(vals[j] - half)]]).astype(np.float32)
        R_.append(np.full(cols.size, k))
        C_.append(cols)
        X_.append(vals)
    rows = np.concatenate(R_).astype(np.int32) if R_ else np.zeros(0, np.int32)
    cols = np.concatenate(C_).astype(np.int32) if C_ else np.zeros(0, np.int32)
    vals = np.concatenate(X_).astype(np.float32) if X_ else np.zeros(0, np.float32)
    return rows, cols, vals


def forced_rows(rng, F, V, cut_edges):
    """F forced rows: copies / partial copies of cut rows and random rows, as an edge list."""
    rows, cols, vals = cut_edges
    out = [[], [], []]
    for r in range(F):
        if rows.size and rng.random() < 0.7:
            k = int(rng.choice(rows))
            sel = rows == k
            scale = np.float32([1.0, 0.3, -0.7][rng.integers(0, 3)])
            c, v = cols[sel], vals[sel] * scale
        else:
            n = int(rng.integers(1, min(8, V) + 1))
            c = rng.choice(V, size=n, replace=False).astype(np.int32)
            v = rng.standard_normal(n).astype(np.float32)
            v = v / np.float32(np.linalg.norm(v))
        out[0].append(np.full(c.size, r)); out[1].append(c); out[2].append(v)
    if not F:
        return np.zeros((2, 0), np.int32), np.zeros(0, np.float32)
    return (np.stack([np.concatenate(out[0]), np.concatenate(out[1])]).astype(np.int32),
            np.concatenate(out[2]).astype(np.float32))


def state_with_cuts(problem, index, rng, K, shuffle=False, extras=True, scale=0.3):
    state, _ = synthetic.make_sample(problem, index, scale=scale)
    inp = list(utils.state_to_inputs(state))
    V = inp[8]
    rows, cols, vals = plant_rows(rng, K, V, extras)
    if shuffle and rows.size > 1:
        p = rng.permutation(rows.size)
        rows, cols, vals = rows[p], cols[p], vals[p]
    inp[4] = rng.standard_normal((K, 6)).astype(np.float32)
    inp[5] = np.stack([rows, cols]).astype(np.int32)
    inp[6] = vals.reshape(-1, 1)
    inp[9] = K
    return tuple(inp), (rows, cols, vals)


def restate(q, edges, K, V, forced, p_max, p_max_ub):
    rows, cols, vals = edges
    A = R.dense_rows(rows, cols, vals, K, V)
    fi, fv = forced
    B = R.dense_rows(fi[0], fi[1], fv, int(fi[0].max()) + 1 if fi.size else 0, V)
    rec = {}
    order, n = R.select(q, A, B, p_max, p_max_ub, record=rec)
    return order, n, rec


def n_forced_of(forced):
    return int(forced[0][0].max()) + 1 if forced[0].size else 0


@pytest.mark.parametrize("problem", synthetic.PROBLEMS)
def test_planted_states_match_the_restatement(dev, model, problem):
    for i, (p_max, p_ub) in enumerate(THRESHOLDS):
        for seed in range(100 * i, 100 * i + 20):
            rng = np.random.default_rng(seed)
            K = int(rng.integers(10, 101))
            inp, edges = state_with_cuts(problem, seed % 7, rng, K)
            forced = forced_rows(rng, 2, inp[8], edges)
            res = model.select_cuts(inp, (forced[0], forced[1], 2), p_max=p_max, p_max_ub=p_ub, max_selected=K // 2)
            order, n, rec = restate(res.scores, edges, K, inp[8], forced, p_max, p_ub)
            if R.margins_ok(rec, p_max, p_ub):
                break
        else:
            pytest.fail("no seed with clear margins")
        assert np.array_equal(np.asarray(res.scores), model.score_state(inp).numpy())
        assert res.order.dtype == np.int32 and np.array_equal(res.order, order), (problem, seed)
        assert res.n_kept == n and res.n_selected == min(n, K // 2)
        assert n < K   # the planted copies remove something


def _quality(rng, K, kind):
    if kind == "equal":
        return np.full(K, 0.7, np.float32)
    if kind == "tied":
        return rng.choice(np.float32([0.2, 0.5, 1.0]), size=K).astype(np.float32)
    if kind == "negative":
        return (-rng.uniform(0.1, 1.0, K)).astype(np.float32)
    q = rng.uniform(0.0, 1.0, K).astype(np.float32)
    q[rng.random(K) < 0.2] = np.nan
    return q


SWEEP_K = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4096]
KINDS = ["equal", "tied", "negative", "nan"]


def _sweep_cases():
    cases = []
    for K in SWEEP_K:
        for F in (0, 1, 3):
            for ti, thr in enumerate(THRESHOLDS):
                for ki, kind in enumerate(KINDS):
                    if K >= 1000 and (F + ti + ki) % 4:     # the large states: a quarter of the grid, every value still covered
                        continue
                    cases.append((K, F, thr, kind))
    return cases


def test_sweep_matches_the_restatement(dev):
    seen_removed = 0
    for ci, (K, F, (p_max, p_ub), kind) in enumerate(_sweep_cases()):
        V = 40 if K < 1000 else 300
        for seed in range(ci * 50, ci * 50 + 20):
            rng = np.random.default_rng(seed)
            edges = plant_rows(rng, K, V)
            if rng.random() < 0.5 and edges[0].size > 1:          # edge list not sorted by row: the graph build sorts it
                p = rng.permutation(edges[0].size)
                edges = tuple(a[p] for a in edges)
            q = _quality(rng, K, kind)
            forced = forced_rows(rng, F, V, edges)
            order, n, rec = restate(q, edges, K, V, forced, p_max, p_ub)
            if R.margins_ok(rec, p_max, p_ub):
                break
        else:
            pytest.fail(f"no seed with clear margins for {(K, F, p_max, p_ub, kind)}")
        g = BipartiteGraph(torch.from_numpy(np.stack([edges[0], edges[1]])).to(dev), torch.from_numpy(edges[2]).to(dev), K, V)
        packed = ops.pack_rows(forced[0], forced[1], F, V) if F else None
        got_order, got_n = ops.select_cuts(torch.from_numpy(q).to(dev), g, None,
                                           tuple(torch.from_numpy(a).to(dev) for a in packed) if packed else None,
                                           p_max=p_max, p_max_ub=p_ub)
        got_order, got_n = got_order.cpu().numpy(), int(got_n.cpu()[0])
        assert np.array_equal(got_order, order) and got_n == n, (K, F, p_max, p_ub, kind, seed)
        seen_removed += n < K
    assert seen_removed > 20


def test_single_call_general_and_batched_paths_agree(dev, model):
    rng = np.random.default_rng(7)
    states, forceds, results = [], [], []
    for s in range(8):
        K = [12, 40, 64, 65, 100, 3, 0, 200][s]
        inp, edges = state_with_cuts(synthetic.PROBLEMS[s % 4], s, rng, K, shuffle=(s % 3 == 0))
        forced = forced_rows(rng, s % 3, inp[8], edges)
        f = (forced[0], forced[1], s % 3)
        single = model.select_cuts(inp, f)
        dev_inp = tuple(torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x for x in inp)
        general = model.select_cuts(dev_inp, f)
        assert np.array_equal(np.asarray(single.scores), np.asarray(general.scores))
        assert np.array_equal(single.order, general.order) and single.n_kept == general.n_kept, s
        order, n, rec = restate(single.scores, edges, K, inp[8], forced, 0.1, 0.5)
        assert R.margins_ok(rec, 0.1, 0.5), s
        assert np.array_equal(single.order, order) and single.n_kept == n, s
        states.append((inp, edges)); forceds.append(f); results.append(single)
    # the batched entry: the 8 states stacked (cut rows and forced rows with shifted variable ids), one workgroup per sample
    v_off = np.cumsum([0] + [inp[8] for inp, _ in states])
    k_off = np.cumsum([0] + [inp[9] for inp, _ in states])
    f_off = np.cumsum([0] + [f[2] for f in forceds])
    rows = np.concatenate([e[0] + k_off[i] for i, (_, e) in enumerate(states)]).astype(np.int32)
    cols = np.concatenate([e[1] + v_off[i] for i, (_, e) in enumerate(states)]).astype(np.int32)
    vals = np.concatenate([e[2] for _, e in states]).astype(np.float32)
    fi = np.concatenate([np.stack([f[0][0] + f_off[i], f[0][1] + v_off[i]]) for i, f in enumerate(forceds)], 1)
    fv = np.concatenate([f[1] for f in forceds]).astype(np.float32)
    packed = ops.pack_rows(fi, fv, int(f_off[-1]), int(v_off[-1]))
    g = BipartiteGraph(torch.from_numpy(np.stack([rows, cols])).to(dev), torch.from_numpy(vals).to(dev), int(k_off[-1]),
                       int(v_off[-1]))
    q = torch.from_numpy(np.concatenate([np.asarray(r.scores) for r in results])).to(dev)
    order, n_kept = ops.select_cuts(q, g, torch.from_numpy(k_off.astype(np.int32)).to(dev),
                                    tuple(torch.from_numpy(a).to(dev) for a in packed),
                                    torch.from_numpy(f_off.astype(np.int32)).to(dev), max_cuts=int(max(k_off[1:] - k_off[:-1])))
    order, n_kept = order.cpu().numpy(), n_kept.cpu().numpy()
    for i, r in enumerate(results):
        assert np.array_equal(order[k_off[i]:k_off[i + 1]], r.order) and n_kept[i] == r.n_kept, i


def test_limits_and_bad_thresholds(dev, model):
    rng = np.random.default_rng(3)
    inp, _ = state_with_cuts("setcov", 0, rng, 4097, extras=False)
    with pytest.raises(_lib.GcnnError, match="4096"):
        model.select_cuts(inp)
    g = BipartiteGraph(torch.zeros((2, 0), dtype=torch.int32, device=dev), torch.zeros(0, device=dev), 4097, 10)
    with pytest.raises(_lib.GcnnError, match="4096"):
        ops.select_cuts(torch.zeros(4097, device=dev), g)
    inp, _ = state_with_cuts("setcov", 0, rng, 20)
    for bad in (float("nan"), float("inf"), None):
        with pytest.raises(ValueError):
            model.select_cuts(inp, p_max=bad)
        with pytest.raises(ValueError):
            model.select_cuts(inp, p_max_ub=bad)
    # a sample larger than the max_cuts the caller promised is flagged, not read past
    g = BipartiteGraph(torch.zeros((2, 0), dtype=torch.int32, device=dev), torch.zeros(0, device=dev), 30, 10)
    order, n_kept = ops.select_cuts(torch.rand(30, device=dev), g, torch.tensor([0, 10, 30], dtype=torch.int32, device=dev),
                                    max_cuts=10)
    assert n_kept.cpu().tolist() == [10, -1]


def test_every_selection_launch_is_recorded(dev, model):
    assert launchnames.launch_names(SELECT) == SELECT_NAMES
    rng = np.random.default_rng(11)
    for K in (5, 64, 65, 1000):   # one kernel pair on every size: there is no small-K / large-K variant to tell apart
        inp, edges = state_with_cuts("combauc", 1, rng, K)
        forced = forced_rows(rng, 1, inp[8], edges)
        model.select_cuts(inp, (forced[0], forced[1], 1))   # warm
        with _lib.launch_profile() as prof:
            model.select_cuts(inp, (forced[0], forced[1], 1))
        names = [n for n, _ in prof.launches]
        assert [n for n in names if n.startswith("k_sel_")] == ["k_sel_pairs", "k_sel_filter"], names
        assert "k_rank_scores" not in names   # the filter ranks for itself
