"""The PreNorm statistics cases of tests/prenormcases.py, checked on the host: every case has the sizes, planted outliers and empty rows
it claims; a block-strided two-pass sum with per-block partials, restated in NumPy, stays within the bounds of
tests/test_gpu_prenorm_edges.py against `math.fsum`; and the same restatement with each defect the cases were chosen against leaves
those bounds on the case said to catch it -- so the device test can tell a defective kernel from a correct one.  CPU only."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import prenormcases as P
from oracle import gcnn_oracle as O
from gpucommon import fp64_moments, oracle_layer_inputs

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcnn-cut-selector_amd", "csrc")


def _params(seed=41, randomize=42):
    return O.randomize_params(O.init_params(seed, np.float32), randomize)


# ---- the thresholds are the source's -----------------------------------------------------------------------------------------------
def test_constants_are_those_of_the_kernels_and_the_plan():
    misc = open(os.path.join(CSRC, "k_misc.hpp")).read()
    capi = open(os.path.join(CSRC, "gcnn_capi.hip")).read()
    assert int(re.search(r"#define ST_MAX_BLOCKS (\d+)", misc).group(1)) == P.ST_MAX_BLOCKS
    body = misc[misc.index("void stats_body"):misc.index("void k_stats(")]
    assert re.findall(r"\+= (?:\(size_t\))?nblk \* (\d+)", body) == [str(P.THREADS), str(P.THREADS), str(P.BLOCK_EDGES)]
    work = re.search(r"const int work = a\.src == ST_EDGE \? cdiv\(a\.n, (\d+)\) : \(a\.src == ST_FLAT \? cdiv\(a\.n, (\d+)\) : "
                     r"cdiv\(a\.n, (\d+)\)\)", capi)
    assert [int(g) for g in work.groups()] == [P.BLOCK_EDGES, P.FLAT_ROWS, P.THREADS]
    assert "std::min(work, ST_MAX_BLOCKS)" in capi
    expand = re.search(r"expand_grid\(const ExpandArgs& x\) \{ return std::min\(cdiv\(x\.n_seg, (\d+)\), (\d+)\)", capi)
    assert [int(g) for g in expand.groups()] == [P.THREADS, P.ST_MAX_BLOCKS]
    assert re.search(r"r < a\.n_seg; r \+= nblk \* (\d+)", misc).group(1) == str(P.THREADS)
    assert P.SEAM == {"cols": P.ST_MAX_BLOCKS * P.THREADS, "flat": P.ST_MAX_BLOCKS * P.THREADS // P.EMB,
                      "edge": P.ST_MAX_BLOCKS * P.THREADS // P.EDGE_LANES, "expand": P.ST_MAX_BLOCKS * P.THREADS}


def _trips(source, n):
    return P.cdiv(n, P.grid(source, n) * P.PER_BLOCK[source])


def test_sizes_sit_where_the_cases_say():
    cols, flat, edge = P.SEAM["cols"], P.SEAM["flat"], P.SEAM["edge"]
    s = P.sizes(P.case("seam-small")["state"])
    assert (s["C"], s["V"], s["K"]) == (flat + 1, flat - 1, flat) and (s["E1"], s["E2"]) == (edge + 1, edge)
    assert [_trips("flat", s[k]) for k in "CVK"] == [2, 1, 1] and [_trips("edge", s[k]) for k in ("E1", "E2")] == [2, 1]
    assert all(P.grid("flat", s[k]) == P.ST_MAX_BLOCKS for k in "CVK") and P.grid("edge", s["E2"]) == P.ST_MAX_BLOCKS
    assert max(s.values()) < cols                                  # its raw layers stay below their seam

    s = P.sizes(P.case("seam-rows")["state"])
    assert (s["C"], s["V"], s["E1"]) == (cols + 1, cols + 2, cols + 3) and s["K"] == 40
    assert [_trips("cols", s[k]) for k in ("C", "E1", "V")] == [2, 2, 2]            # layers 0, 1, 2 with f = 4, 1, 14
    assert _trips("expand", s["C"]) == 2 and _trips("flat", s["C"]) == _trips("flat", s["V"]) == 65   # one full, 64 more
    assert _trips("edge", s["E1"]) == 17

    s = P.sizes(P.case("seam-cuts")["state"])
    assert (s["K"], s["E2"]) == (cols + 2, cols + 6) and s["C"] < 1000 and s["V"] < 1000
    assert _trips("cols", s["K"]) == _trips("cols", s["E2"]) == _trips("expand", s["K"]) == 2

    assert P.sizes(P.case("constant")["state"])["V"] == cols + 1
    want = {"one": (1, 1, 1, 1, 1), "no_cut_edges": (0, 1, 1), "no_cuts": (0, 0, 1), "no_cons_edges": (1, 1, 0)}
    for t in P.TINY:
        s = P.sizes(P.case("tiny-" + t)["state"])
        got = (s["C"], s["V"], s["K"], s["E1"], s["E2"]) if t == "one" else (min(s["E2"], 1), min(s["K"], 1), min(s["E1"], 1))
        assert got == want[t], (t, s)
    # what the older tests reach, at their largest batch (combauc x 3, test_gpu_prenorm_guard.py): no cap and no second trip in any
    # layer but 9, whose 21,714 cut edges take a second ST_EDGE trip -- without a planted value, under rtol 1e-6
    from gcnn_cut_selector_amd import synthetic
    s = P.sizes(synthetic.make_batch("combauc", 3)[0])
    assert [layer for layer, (src, key) in P.LAYER.items() if P.cdiv(s[key], P.PER_BLOCK[src]) >= P.ST_MAX_BLOCKS] == [9]
    assert _trips("edge", s["E2"]) == 2 and max(s.values()) < cols and max(s["C"], s["V"], s["K"]) < flat


@pytest.mark.parametrize("name", ["seam-small", "seam-rows", "seam-cuts"])
def test_edge_lists_are_sorted_and_outliers_sit_on_the_seams(name):
    case = P.case(name)
    st, s = case["state"], P.sizes(case["state"])
    for ei, n_left, lens in ((st[1], s["C"], case["lens"][0]), (st[5], s["K"], case["lens"][1])):
        key = ei[0].astype(np.int64) * (s["V"] + 1) + ei[1]
        assert np.all(np.diff(key) > 0) and ei[0].max() < n_left and ei[1].max() < s["V"] and ei.min() >= 0
        assert np.array_equal(np.bincount(ei[0], minlength=n_left), lens)
    coef = {1: st[2].reshape(-1), 4: st[6].reshape(-1)}
    n_planted = 0
    for layer in case["layers"]:
        src, key = P.LAYER[layer]
        want = P.seam_positions(src, s[key])
        planted = case["planted"][layer]
        assert len(planted) == len(want) > 0
        for (pos, e, col), at in zip(planted, want):
            if layer in (0, 2, 3):
                x = P.raw_input(st, layer)
                assert pos == at and abs(x[pos, col]) >= 1000
            elif src in ("cols", "edge"):
                assert pos == at == e and abs(coef[1 if key == "E1" else 4][e]) >= 1000
            else:
                which, ei = (4, st[5]) if layer == 10 else (1, st[1])
                recv = ei[1] if layer == 8 else ei[0]
                assert recv[e] == pos and abs(coef[which][e]) >= 1000
                assert pos == at or not np.any(recv == at)         # the seam row itself, unless nothing reaches it
                assert not np.any((recv > pos) & (recv <= at))
            n_planted += 1
    # nothing else is large: the bulk is standard normal
    big = sum(int((np.abs(np.asarray(a)) > 100).sum()) for a in (st[0], st[2], st[3], st[4], st[6]))
    assert 0 < big <= n_planted
    for a in (st[0], st[2], st[3], st[4], st[6]):
        a = np.asarray(a)
        assert np.abs(a[np.abs(a) < 100]).max() < 6.0 and (a.size < 1000 or 0.9 < a[np.abs(a) < 100].std() < 1.1)


def test_empty_rows_and_the_hub_are_where_the_cases_say():
    lens1, lens2 = P.case("seam-small")["lens"]
    flat = P.SEAM["flat"]
    assert lens1[flat] > 0 and lens1[flat - 1] > 0 and lens1.size == flat + 1     # layer 6's second trip is one row, and it has edges
    assert lens2[-1] == 0 and lens2[0] == 0 and (lens1 == 0).sum() > 100 and (lens2 == 0).sum() > 100
    assert lens1.max() == 3000
    lens1, _ = P.case("seam-rows")["lens"]
    seam = P.SEAM["expand"]
    assert np.all(lens1[seam - 4:] == 0) and lens1.size == seam + 1               # empty segments on both sides of the seam
    assert ((lens1 == 0) | (lens1 == 1)).mean() > 0.75 and lens1[P.SEAM["flat"] - 1] == lens1[P.SEAM["flat"]] == 1
    _, lens2 = P.case("seam-cuts")["lens"]
    assert lens2[seam - 1] == 1 and lens2[seam] == 2 and lens2[seam + 1] == 1 and lens2.size == seam + 2   # second trip writes ids
    assert np.all(lens2[seam - 4:seam - 1] == 0)
    st = P.case("seam-cuts")["state"]
    assert np.bincount(st[5][1], minlength=st[8]).min() > 1000                    # every variable is a hub sender


def test_constant_columns_are_exact_in_any_order():
    st = P.case("constant")["state"]
    v = st[3]
    for col, c in P.CONSTANT_COLS.items():
        P.assert_constant_exact(v[:, col], c)
        for blocks in (1, 7, P.ST_MAX_BLOCKS):
            mean = P.strided_sum(P.items_of("cols", v[:, col]), blocks) / v.shape[0]
            assert mean == float(c) and P.strided_sum(P.items_of("cols", v[:, col]), blocks, centre=mean) == 0.0
    assert float(P.CONSTANT) != 0.3 and float(P.CONSTANT) == float(np.float32(0.3))


def test_offset_columns_are_exact_in_fp32():
    st = P.case("offset")["state"]
    for layer, col in P.OFFSET_COLS.items():
        x = P.raw_input(st, layer)[:, col].astype(np.float64)
        k = (x - P.OFFSET) / P.OFFSET_STEP
        assert np.all(k == np.round(k)) and np.abs(k).max() < 64 and 0.2 < x.var() < 0.5


# ---- the restatement against fsum, intact and with each defect --------------------------------------------------------------------------
def _raw_check(name, layer, **defect):
    """[(column, |mean error| / bound, |variance error| / bound)] of the restated pass over one raw layer of a case."""
    x = P.raw_input(P.case(name)["state"], layer)
    out = []
    for u in range(x.shape[1]):
        mean, var, mean_abs = P.exact_stats(x[:, u])
        bm, bv = P.raw_bounds(x.shape[0], var, mean_abs)
        got_mean, got_var = P.strided_stats("cols", x[:, u], x.shape[0], **defect)
        out.append((u, abs(got_mean - mean) / bm if bm else float(got_mean != mean),
                    abs(got_var - var) / bv if bv else float(got_var != var)))
    return out


@pytest.mark.parametrize("name", P.NAMES)
def test_restated_pass_meets_the_derived_bound_on_raw_layers(name):
    for layer in P.case(name)["layers"]:
        if layer <= 4:                      # (a layer without elements gives no column to check)
            for u, em, ev in _raw_check(name, layer):
                assert em <= 1.0 and ev <= 1.0, (name, layer, u, em, ev)


def _outside(rows, cols=None):
    return all(em > 1.0 or ev > 1.0 for u, em, ev in rows if cols is None or u in cols)


def test_single_trip_cols_loop_is_seen_by_seam_rows_and_seam_cuts():
    for name, layers in (("seam-rows", (0, 1, 2)), ("seam-cuts", (3, 4))):
        for layer in layers:
            rows = _raw_check(name, layer, single_trip=True)
            assert _outside(rows), (name, layer, rows)
            assert min(max(em, ev) for _, em, ev in rows) > 1e3      # not by a whisker: the lost rows hold a planted value
    assert not _outside(_raw_check("seam-small", 0, single_trip=True))   # below the seam there is no second trip to lose


def test_uncapped_grid_under_a_final_of_1024_rows_is_seen_by_seam_rows():
    for layer in (0, 1, 2):
        rows = _raw_check("seam-rows", layer, uncapped=True)
        assert _outside(rows) and min(max(em, ev) for _, em, ev in rows) > 1e3, (layer, rows)


def test_uncentred_second_pass_is_seen_by_offset():
    for layer, col in P.OFFSET_COLS.items():
        rows = _raw_check("offset", layer, no_centre=True)
        assert _outside(rows, {col}) and [ev for u, _, ev in rows if u == col][0] > 1e12, (layer, rows)


def test_float_accumulators_are_seen_by_offset_and_float_finals_by_constant():
    """`float acc[]` in stats_body: a thread of the constant case adds at most two equal values, which fp32 holds exactly, so only
    the offset case sees it (the squared deviations round to 24 bits).  `float s` in the final kernel: the chain over 1,024 block
    partials rounds in both cases."""
    for layer, col in P.OFFSET_COLS.items():
        for how in (dict(acc=np.float32), dict(final=np.float32)):
            assert _outside(_raw_check("offset", layer, **how), {col}), (layer, how)
    v = P.case("constant")["state"][3]
    col = [c for c, val in P.CONSTANT_COLS.items() if val != 0][0]
    mean, var = P.strided_stats("cols", v[:, col], v.shape[0], acc=np.float32)
    assert (mean, var) == (float(P.CONSTANT), 0.0)
    mean, var = P.strided_stats("cols", v[:, col], v.shape[0], final=np.float32)
    assert mean != float(P.CONSTANT) and var != 0.0


@functools.lru_cache(maxsize=None)
def _conv_layers(name):
    """A small case: the fp64 inputs of layers 5 .. 10, their moments, and the bounds with the distance of the oracle's fp32
    evaluation (its activations in fp32, summed in fp64 as the device sums them)."""
    params, state = _params(), P.case(name)["state"]
    x64 = oracle_layer_inputs(params, state, torch.float64, range(5, 11))
    m32 = oracle_layer_inputs(params, state, torch.float32, range(5, 11), reduce=fp64_moments)
    out = {}
    for layer, x in x64.items():
        mean, var = (float(a[0]) for a in fp64_moments(x))
        gap = (abs(float(m32[layer][0][0]) - mean), abs(float(m32[layer][1][0]) - var))
        out[layer] = (x.numpy(), mean, var, P.conv_bounds(mean, var, *gap))
    return params, state, out


def _conv_check(name, layer, x=None, **defect):
    _, state, per = _conv_layers(name)
    x0, mean, var, (bm, bv) = per[layer]
    src, key = P.LAYER[layer]
    got_mean, got_var = P.strided_stats(src, x0 if x is None else x, P.sizes(state)[key], **defect)
    return abs(got_mean - mean) / bm, abs(got_var - var) / bv


@pytest.mark.parametrize("name", ["seam-small", "tiny-one"])
def test_restated_pass_meets_the_oracle_bound_on_conv_layers(name):
    for layer in range(5, 11):
        em, ev = _conv_check(name, layer)
        assert em <= 1e-3 and ev <= 1e-3, (layer, em, ev)      # fp64 sums of fp64 values: orders inside a 1e-6 bound


def test_single_trip_flat_and_edge_loops_are_seen_by_seam_small():
    for layer in (5, 6, 7):                                     # the layers of seam-small with a second trip
        em, ev = _conv_check("seam-small", layer, single_trip=True)
        assert em > 10 and ev > 100, (layer, em, ev)          # one planted edge lost: tens and hundreds of bounds
    for layer in (8, 9, 10):                                    # below and on the cap: one trip
        assert max(_conv_check("seam-small", layer, single_trip=True)) <= 1e-3


@pytest.mark.parametrize("name,factor", [("seam-small", 1.0), ("tiny-one", 1e3)])
def test_missing_edge_shift_and_missing_emb_in_the_count_are_seen_by_every_edge_layer(name, factor):
    """Without `esh` every joint pre-activation moves by esh * esc * w: far outside the bound on a state without planted values
    (tiny-one); on seam-small the planted values raise the standard deviation, and with it the mean's absolute tolerance, so the
    shift is outside by a small factor only."""
    params, state, per = _conv_layers(name)
    for layer, conv, edge in ((5, "cons_conv", "cons_edge"), (7, "var_conv", "cons_edge"), (9, "cut_conv", "cut_edge")):
        esh, esc = (float(params[f"{edge}_prenorm/{k}"][0]) for k in ("shift", "scale"))
        assert abs(esh) > 0.01                                  # random shifts (O.randomize_params)
        w = np.asarray(params[f"{conv}_feat_edge/kernel"], np.float64).reshape(1, -1)
        without = per[layer][0].reshape(-1, P.EMB) - esh * esc * w                 # J = PL + (c + esh) esc w + PR
        em, ev = _conv_check(name, layer, x=without)
        assert max(em, ev) > factor, (layer, em, ev)
        n = P.sizes(state)[P.LAYER[layer][1]]
        em, ev = _conv_check(name, layer, count=n)              # count = ne instead of ne * EMB
        assert em > 1e3 and ev > 1e3, (layer, em, ev)
