"""tests/rowcases.py proved on the host: over the case list every branch of the launchers' form arithmetic is taken on both sides at
adjacent sizes, every case has the form it is named for and a planted row in every seam tile, the restatement agrees with the host
code, a restatement with one of the named defects loses, doubles or swaps a planted row on a named case, and the planting is strong
enough for the bounds of tests/test_gpu_row_seams.py."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest
import torch

from oracle import gcnn_oracle as O
import gradparity
import rowcases as R
from test_wgradcases import BOUND, FACTOR, strength

CASES = R.cases()
IDS = [c["id"] for c in CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured by test_planting_is_strong_enough: the smallest factor over all cases, components and gradient tensors
MIN_FACTOR_CASE = "C/32769"
SCORE_BOUND = lambda s: 1e-4 * max(1.0, abs(s))     # the GPU test's: rtol = atol = 1e-4


@pytest.fixture(scope="module")
def params():
    return O.randomize_params(O.init_params(11, np.float32), 12)     # gpucommon.make_model(11)'s weights


def _form(cid, name):
    return next(f for _, l, f in R.launches_under(R.case(cid)) if l["name"] == name)


def _launch(cid, name, path="fused"):
    c = R.case(cid)
    l = next(l for p in (path, "autograd_fwd", "autograd_bwd") for l in R.launches(c["C"], c["V"], c["K"], p) if l["name"] == name)
    return l, R.form_of(l)


# ---- coverage: both sides of every branch, at adjacent sizes ---------------------------------------------------------------------------
SINGLE_OF = {"C": ("k_conv_fwd<proj> v->c", "k_conv_bwd {C}"), "V": ("k_conv_fwd<proj> c->v",), "K": ("k_conv_turn", "k_conv_fwd<readout>", "k_conv_bwd {K}")}


def test_single_row_set_cases_have_the_forms_they_are_named_for():
    for s in "CVK":
        for name in SINGLE_OF[s]:
            never_splits = name.startswith("k_conv_bwd")
            f = {n: _launch(f"{s}/{n}", name)[1] for n in R.LARGE_SIZES}
            f.update({n: _launch(f"n{n}", name)[1] for n in R.SMALL_SIZES})
            for n in (1, 15, 16):
                assert f[n]["grid"] == 1 and f[n]["ntile"][0] == 1, (name, n)
            assert f[17]["ntile"][0] == 2 and f[80]["ntile"][0] == 5
            if never_splits:      # 80 rows: two blocks of four waves, three waves without a tile
                assert not any(f[n]["split"] for n in f)
                assert (f[80]["nb"], f[80]["nwaves"]) == ([2, 0], 4)
                assert (f[4096]["nb"][0], f[4096]["nwaves"]) == (64, 4)
            else:                 # one four-wave block per tile up to 256 tiles
                assert all(f[n]["split"] and f[n]["grid"] == f[n]["ntile"][0] for n in (1, 15, 16, 17, 80, 4096))
            # 4,097 rows: 65 four-wave blocks, three of which have a wave without a tile
            assert (f[4097]["split"], f[4097]["nb"][0], f[4097]["nwaves"]) == (False, 65, 4)
            idle = [b for b in range(65) if any(not R.tiles_of(f[4097], 0, b, w, 4097)[0] for w in range(4))]
            assert idle == [62, 63, 64]
            # 16,384: one tile per wave of 256 four-wave blocks; 16,385: eight waves spread over 256 blocks, one wave 4 owns tile 1,024
            assert (f[16384]["nb"][0], f[16384]["nwaves"], f[16384]["spread"]) == (256, 4, False)
            assert all(len(R.tiles_of(f[16384], 0, b, w, 16384)[0]) == 1 for b in range(256) for w in range(4))
            assert (f[16385]["nb"][0], f[16385]["nwaves"], f[16385]["spread"], f[16385]["share"]) == (256, 8, True, False)
            assert R.owner(f[16385], 0, 1024) == (0, 4, 0)
            assert sum(bool(R.tiles_of(f[16385], 0, b, w, 16385)[0]) for b in range(256) for w in range(4, 8)) == 1
            # 32,768: one tile per wave of 256 eight-wave blocks, written through; 32,769: plain stores, a second trip for block 0 wave 0
            assert (f[32768]["nb"][0], f[32768]["nwaves"], f[32768]["spread"], f[32768]["share"]) == (256, 8, False, False)
            assert all(len(R.tiles_of(f[32768], 0, b, w, 32768)[0]) == 1 for b in range(256) for w in range(8))
            assert (f[32769]["nb"][0], f[32769]["nwaves"], f[32769]["share"], f[32769]["trim"]) == (256, 8, True, False)
            assert R.owner(f[32769], 0, 2048) == (0, 0, 1)
            assert [(b, w) for b in range(256) for w in range(8) if len(R.tiles_of(f[32769], 0, b, w, 32769)[0]) > 1] == [(0, 0)]
            assert R.write_through((32768, 40)) and not R.write_through((32769, 40)) and R.write_through((40,))


def test_two_program_cases_have_the_forms_they_are_named_for():
    bwd, tail = R.PAIRS
    f = _form("pair/trim", bwd)
    assert sum(R.form((32768, 4096), (5, 2), can_split=False, defect="no_trim")["nb"]) == 257      # 244 + 13
    assert (f["nb"], f["trim"], f["share"], f["grid"]) == ([243, 13], True, True, 256)
    f = _form("pair/trim", tail)
    assert R.form((32768, 4096), (3, 2), can_split=False, defect="no_trim")["nb"] == [237, 20]
    assert (f["nb"], f["trim"], f["share"]) == ([236, 20], True, True)
    for name in R.PAIRS:
        f = _form("pair/256", name)
        assert (f["nb"], f["trim"], f["share"], f["spread"]) == ([248, 8], False, True, False), name
        f = _form("pair/onetile", name)
        assert (f["ntile"], f["nb"], f["trim"]) == ([2048, 1], [255, 1], True), name
        a, b = _form("pair/1024", name), _form("pair/1025", name)
        assert (a["total"], a["nwaves"], a["spread"], a["nb"]) == (1024, 4, False, [250, 6]), name
        assert (b["total"], b["nwaves"], b["spread"]) == (1025, 8, True) and sum(b["nb"]) == 256, name
    f = _form("pair/zero", tail)
    assert f["ntile"] == [257, 0] and f["nb"] == [65, 0] and f["blk0"] == [0, 65, 65]
    # and every case's k_conv_bwd {C} is a two-program launch whose second program has no row
    for c in CASES:
        if c["C"] > 0:
            assert _launch(c["id"], "k_conv_bwd {C}")[1]["nb"][1] == 0


def test_embedding_cases_have_the_forms_they_are_named_for():
    a, b = _form("emb/256", "k_embed_fwd"), _form("emb/257", "k_embed_fwd")
    assert a["split"] and a["ntile"] == [125, 81, 50] and a["blk0"] == [0, 125, 206, 256]
    assert not b["split"] and b["ntile"] == [125, 81, 51] and b["nwaves"] == 4 and b["nb"] == [32, 21, 13]
    la, lb = _launch("emb/8191", "k_embed_fwd")[0], _launch("emb/8192", "k_embed_fwd")[0]
    assert (la["cap"], lb["cap"]) == (256, 2 * R.CUS - 3)
    a, b = _form("emb/8191", "k_embed_fwd"), _form("emb/8192", "k_embed_fwd")
    assert (a["total"], b["total"]) == (8191, 8192) and a["grid"] == 256 and b["grid"] == 509
    assert a["share"] and b["share"] and len(set(a["ntile"])) > 1


def test_every_branch_is_taken_on_both_sides():
    seen = {k: set() for k in ("split", "nwaves", "spread", "share", "trim", "cap", "wt")}
    for c in CASES:
        for _, l, f in R.launches_under(c):
            for k in ("split", "nwaves", "spread", "share", "trim"):
                seen[k].add(f[k])
            seen["cap"].add(l["cap"])
            seen["wt"].add(R.write_through(l["n"]))
    assert all(len(v) == 2 for v in seen.values()), seen


@pytest.mark.parametrize("cid", IDS)
def test_every_seam_tile_holds_a_planted_row(cid):
    c = R.case(cid)
    key = {"C": "c", "V": "v", "K": "k"}
    under = R.launches_under(c)
    assert under and 1 <= len(c["comps"]) <= 8
    for _, l, f in under:
        for p, s in enumerate(l["sets"]):
            if s is None or l["n"][p] == 0:
                continue
            planted = {q[key[s]] for q in c["comps"]}
            n = l["n"][p]
            assert n - 1 in planted, (cid, l["name"], s)
            for name, tile in R.seam_tiles(f, p, n).items():
                assert planted & set(range(16 * tile, min(n, 16 * tile + 16))), (cid, l["name"], s, name, tile)
            if n > 2 and (n - 1) % 16 > 1:
                assert 16 * ((n - 1) // 16) in planted, (cid, l["name"], s, "first row of the last tile")
    for k in "kvc":
        rows = sorted(q[k] for q in c["comps"] if q[k] is not None)
        assert all(b - a > 1 for a, b in zip(rows, rows[1:])), (cid, k)
    assert R.audit(c) == []


@pytest.mark.parametrize("cid", IDS)
def test_restatement_stores_every_tile_once(cid):
    c = R.case(cid)
    for path in ("fused", "autograd_fwd", "autograd_bwd", "nograd", "score_state"):
        for l in R.launches(c["C"], c["V"], c["K"], path):
            f = R.form_of(l)
            assert f["grid"] == f["blk0"][-1] <= max(l["cap"], 0 if not f["split"] else f["total"])
            for p, n in enumerate(l["n"]):
                cov = R.coverage(f, p, n)
                assert sorted(cov) == [(t, t) for t in range(R.ntiles(n))], (cid, l["name"], p)
                for t in {0, R.ntiles(n) - 1} if n else ():      # owner() is the inverse of tiles_of()
                    b, w, trip = R.owner(f, p, t)
                    assert R.tiles_of(f, p, b, max(w, 0), n)[0][trip] == t


@pytest.mark.parametrize("cid", IDS)
def test_components_are_isolated(cid):
    case = R.case(cid)
    state, y, comps = R.build(case)
    cei, kei = state[1], state[5]
    assert (state[7], state[8], state[9]) == (case["C"], case["V"], case["K"])
    for e in (cei, kei):      # sorted, no duplicate edge
        lin = e[0].astype(np.int64) * case["V"] + e[1]
        assert np.all(np.diff(lin) > 0)
    for c in comps:
        assert y[c["k"]] == R.y_star(case) and 0 <= c["y0"] < 0.2
        assert kei[1][kei[0] == c["k"]].tolist() == [c["v"]] and kei[0][kei[1] == c["v"]].tolist() == [c["k"]]
        assert cei[0][cei[1] == c["v"]].tolist() == ([c["c"]] if c["c"] is not None else [])
        if c["c"] is not None:
            assert cei[1][cei[0] == c["c"]].tolist() == [c["v"]]
    others = np.setdiff1d(np.arange(case["K"]), [c["k"] for c in comps])
    assert np.all(y[others] < 0.2)
    # no ordinary constraint is on a path to a cut: its variables are no cut's
    planted_c = [c["c"] for c in comps if c["c"] is not None]
    assert not set(cei[1][~np.isin(cei[0], planted_c)].tolist()) & set(kei[1].tolist())
    # settled: every ordinary cut's target is its own score, the planted ones keep y*
    s = np.linspace(-1, 1, case["K"])
    _, y2, _ = R.build(case, scores=s)
    assert np.array_equal(y2[others], s.astype(np.float32)[others]) and all(y2[c["k"]] == R.y_star(case) for c in comps)


# ---- fidelity: the restatement against the host code ---------------------------------------------------------------------------------
DRIVER = r"""
#include <algorithm>
#include <cstdio>
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
#define GCNN_KNOB(name, dflt) (dflt)
%s
int main() {
    int g, n[3], ns[3], cap, can_split;
    while (scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d", &g, n, n + 1, n + 2, ns, ns + 1, ns + 2, &cap, &can_split) == 9) {
        int blk0[4] = {0, 0, 0, 0};
        RowsForm f = can_split ? rows_form(n, ns, g, blk0, [&] { return cap; }) : RowsForm{false, rows_blocks(n, ns, g, blk0, cap)};
        printf("%%d %%d", (int)f.split, f.nwaves);
        for (int i = 0; i <= g; ++i) printf(" %%d", blk0[i]);
        printf("\n");
    }
    return 0;
}
"""


def test_form_agrees_with_the_host_code(tmp_path):
    """Way used: the text of rows_blocks, rows_split and rows_form is cut out of gcnn_capi.hip at test time (from the definition of
    rows_blocks to the comment above rows_write_through), compiled with the host compiler into a stand-alone program with GCNN_KNOB
    defined to return its default, and run here on the CPU over a grid of launches that includes every launch of every case."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = open(os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc", "gcnn_capi.hip")).read()
    a = src.index("static int rows_blocks(")
    b = src.index("// The write-through form of a training launch", a)
    text = src[a:b]
    assert "static bool rows_split(" in text and "static RowsForm rows_form(" in text and "hip" not in text
    (tmp_path / "rows_form.cpp").write_text(DRIVER % text)
    exe = str(tmp_path / "rows_form")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, str(tmp_path / "rows_form.cpp")], check=True, capture_output=True, text=True)
    grid = []
    for c in CASES:
        for path in ("fused", "autograd_fwd", "autograd_bwd", "score_state"):
            grid += [(l["n"], l["stages"], l["cap"], l["can_split"]) for l in R.launches(c["C"], c["V"], c["K"], path)]
    assert len(grid) > 400
    sizes = sorted({0, 1, 15, 16, 17, 80, 255, 256, 257, 4080, 4096, 4097, 8191, 16368, 16384, 16385, 16400, 32752, 32768, 32769, 40000, 70000, 131072})
    for n in sizes:       # one row set, as the forward launches and as the backward launches pass it
        grid += [((n,), (4,), 256, True), ((n,), (10,), 256, True), ((n, 0), (5, 2), 256, False)]
    rng = np.random.default_rng(5)
    for a_ in sizes:
        for b_ in sizes:
            grid += [((a_, b_), (5, 2), 256, False), ((a_, b_), (3, 2), 256, False)]
            c_ = int(rng.choice(sizes))
            for cap in (256, 509):
                grid.append(((a_, b_, c_), (4, 3, 3), cap, True))
    for t in range(1000, 1060):     # two programs across 1,024 tiles in total, and across the share and trim conditions
        grid += [((16 * t, 16 * 24), (5, 2), 256, False), ((16 * 2000 + t, 16 * (t - 990)), (3, 2), 256, False)]
    lines = []
    for n, st, cap, cs in grid:
        n3, s3 = list(n) + [0] * (3 - len(n)), list(st) + [1] * (3 - len(st))
        lines.append(" ".join(map(str, [len(n)] + n3 + s3 + [cap, int(cs)])))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60)
    got = [list(map(int, line.split())) for line in r.stdout.splitlines()]
    assert len(got) == len(grid)
    for (n, st, cap, cs), g in zip(grid, got):
        f = R.form(n, st, cap, cs)
        assert [int(f["split"]), f["nwaves"]] + f["blk0"] == g, (n, st, cap, cs, f, g)


# ---- defects break the restatement -------------------------------------------------------------------------------------------------------
NAMED = {"tile_floor": ["n1", "n15", "n17", "C/4097", "V/16385", "K/32769"],
         "row_le": ["n15", "n17", "K/4097", "V/32769"],
         "stride_nblk": ["n80", "V/32769", "pair/trim", "emb/8192"],
         "next_ops": ["V/32769", "C/32769", "pair/trim", "emb/8191"],
         "no_rebase": ["pair/trim", "pair/256", "pair/onetile", "pair/1025", "emb/257"],
         "no_trim": ["pair/trim", "pair/onetile"]}


@pytest.mark.parametrize("defect", sorted(NAMED))
def test_defect_loses_doubles_or_swaps_a_planted_row(defect):
    for cid in NAMED[defect]:
        bad = R.audit(R.case(cid), defect)
        assert bad, (defect, cid)
    assert defect in R.DEFECTS


def test_thresholds_off_by_one_move_the_planted_rows():
    """Split taken at 257 tiles and 8 waves taken at 1,024 tiles are consistent in themselves (no row is lost): they show as another
    partition, in which the planted rows sit with other blocks, waves and trips."""
    for defect, cids, names in (("split257", ("C/4097", "V/4097", "K/4097", "emb/257"), None), ("waves8_at_1024", ("C/16384", "V/16384", "K/16384", "pair/1024"), None)):
        assert defect in R.DEFECTS
        for cid in cids:
            c = R.case(cid)
            moved = 0
            for _, l, f in R.launches_under(c):
                g = R.form_of(l, defect)
                if l["can_split"] or defect != "split257":
                    assert (f["split"], f["nwaves"], f["nb"]) != (g["split"], g["nwaves"], g["nb"]), (defect, cid, l["name"])
                for p, s in enumerate(l["sets"]):
                    if s is not None:
                        moved += sum(R.owner(f, p, q[s.lower()] // 16) != R.owner(g, p, q[s.lower()] // 16) for q in c["comps"])
            assert moved, (defect, cid)
    assert set(NAMED) | {"split257", "waves8_at_1024"} == set(R.DEFECTS)


# ---- the planting is strong enough ----------------------------------------------------------------------------------------------------------
_SCORES = {}


def score_fn(state, key=None):
    """The fp64 scores of make_model(11) on a state (kept per `key`)."""
    if key is None or key not in _SCORES:
        p = O.randomize_params(O.init_params(11, np.float32), 12)
        got = O.scores({k: v.astype(np.float64) for k, v in p.items()}, state, torch.float64)
        if key is None:
            return got
        _SCORES[key] = got
    return _SCORES[key]


def build(case, y_star, boost=None):
    """rowcases.settled for `strength`: without a constraint (C = 0) the constraint embedding, the convolution v -> c and the message
    layers of the convolution c -> v see no row, so their gradients are zero whatever the kernels do; a component then targets the rest."""
    state, y, comps = R.settled(case, lambda st: score_fn(st, (case["id"], case["seed"], boost or R.boost(case))), y_star, boost)
    if case["C"] == 0:
        rest = tuple(n for n in gradparity.NAMES if not n.startswith(("cons_", "var_conv_feat_")))
        for c in comps:
            c["targets"] = rest
    return state, y, comps


class RowHook:
    """A ReLU hook of the oracle that, at one site (the output of a row program), zeroes the rows `rows` (a tile that no wave stored, as
    far as the next launch is concerned) or replaces each by its neighbour's (a swap)."""

    def __init__(self, site, rows, partner=None):
        self.site, self.rows, self.partner = site, torch.as_tensor(rows), None if partner is None else torch.as_tensor(partner)

    def __call__(self, site, z, magnitude, rows):
        out = torch.relu(z)
        if site == self.site:
            out = out.clone()
            out[self.rows] = 0 if self.partner is None else out[self.partner]
        return out


# the outputs of the row programs: the embeddings X and the convolutions' X', per row set
SITES = {"c": ("cons_emb_2", "cons_conv_out_2"), "v": ("var_emb_2", "var_conv_out_2"), "k": ("cut_emb_2", "cut_conv_out_2")}


def score_strength(case, params, boost=None):
    """The smallest factor over 1e-4 max(1, |s|) by which the planted cuts' fp64 scores move when one planted row of a row program's
    output is lost or replaced by its (ordinary) neighbour's: (factor, site, kind)."""
    state, _, comps = R.build(case, None, boost)
    p = O.to_torch({k: v.astype(np.float64) for k, v in params.items()}, torch.float64)
    inputs = O.as_inputs(state, torch.float64)
    with torch.no_grad():
        s = O.forward(p, inputs).numpy()
        ks = [c["k"] for c in comps]
        worst = (np.inf, None, None)
        n_of = {"c": case["C"], "v": case["V"], "k": case["K"]}
        for key, sites in SITES.items():
            rows = [c[key] for c in comps if c[key] is not None]
            if not rows:
                continue
            mine = [c["k"] for c in comps if c[key] is not None]
            planted = set(rows)
            partner = [next((q for q in (r + 1, r - 1) if 0 <= q < n_of[key] and q not in planted), None) for r in rows]
            for site in sites:
                for kind in ("lost", "swapped"):
                    if kind == "swapped" and None in partner:
                        continue       # a set of one row has no neighbour
                    got = O.forward(p, inputs, relu_hook=RowHook(site, rows, partner if kind == "swapped" else None)).numpy()
                    f = min(abs(got[k] - s[k]) / SCORE_BOUND(s[k]) for k in mine)
                    if f < worst[0]:
                        worst = (float(f), site, kind)
    return worst


@pytest.fixture(scope="module")
def factors(params):
    out = {}
    for cid in IDS:
        t = time.perf_counter()
        out[cid] = strength(R.case(cid), params, R.y_star(R.case(cid)), build=build) + score_strength(R.case(cid), params)
        out[cid] += (time.perf_counter() - t,)
    return out


@pytest.mark.parametrize("cid", IDS)
def test_planting_is_strong_enough(factors, cid):
    f, tensor, comp, gap, fs, site, kind, secs = factors[cid]
    print(f"\n{cid}: y* = {R.y_star(R.case(cid))}: smallest factor over the gradient bound {f:.1f} ({tensor}, component {comp}); "
          f"3 gap / (1e-4 ref) at most {gap:.3f}; smallest factor over the score bound {fs:.1f} ({site} {kind}); proof took {secs:.1f} s")
    assert f >= FACTOR, (cid, f, tensor, comp)
    assert fs >= FACTOR, (cid, fs, site, kind)
    # the 1e-4 term decides every tensor on the device, with room: the settled cuts' residuals are fp32 rounding, other on the device
    # than in the fp32 oracle that `gap` is measured with, and weigh more the smaller y* is (else: a larger y*, or R.RESEED)
    assert gap <= R.GAP_SHARE, (cid, gap)


@pytest.mark.parametrize("cid", IDS)
def test_y_star_and_boost_are_the_smallest_powers_of_two(params, cid):
    """From 1 up: the other targets are 0 .. 0.2 and the other rows' features standard normal."""
    c = R.case(cid)
    assert np.log2(R.y_star(c)) % 1 == 0 and np.log2(R.boost(c)) % 1 == 0 and R.y_star(c) >= 1 and R.boost(c) >= 1
    if R.y_star(c) > 1:       # at half of it the factor is missed, or the 3 gap term of the bound is more than its share
        f = strength(c, params, R.y_star(c) / 2, build=build)
        assert f[0] < FACTOR or f[3] > R.GAP_SHARE
    if R.boost(c) > 1:
        assert score_strength(c, params, R.boost(c) / 2)[0] < FACTOR


@pytest.mark.parametrize("cid", IDS)
def test_a_relu_flip_on_the_device_could_be_proven(params, cid):
    """At most gradparity.MAX_AMBIGUOUS units of the fp64 oracle lie within rounding of 0 with a flip that is visible in a gradient
    tensor: whatever branch the fp32 kernels take there, `gradparity.check` can enumerate it (else: R.RESEED)."""
    c = R.case(cid)
    state, y, _ = build(c, R.y_star(c))
    units = gradparity.ambiguous_units({k: v.astype(np.float64) for k, v in params.items()}, state, y)
    print(f"\n{cid}: {len(units)} ambiguous visible ReLU units {[u[:3] for u in units]}")
    assert len(units) <= gradparity.MAX_AMBIGUOUS


def test_smallest_factor(factors):
    worst = min(factors, key=lambda cid: factors[cid][0])
    slow = max(factors, key=lambda cid: factors[cid][-1])
    print(f"\nsmallest factor over all cases: {factors[worst][0]:.1f} ({worst}, {factors[worst][1]}); longest proof {factors[slow][-1]:.1f} s ({slow})")
    assert worst == MIN_FACTOR_CASE
    assert factors[slow][-1] < 90, "a case too large in the sets not under test"
