"""States at the seams of the row programs, and a restatement of their index arithmetic (host only, NumPy only).

The row programs: `k_embed_fwd`, `k_conv_fwd`, `k_conv_turn`, `k_conv_bwd`, `k_tail_bwd` with their `_wt` and `_split` forms and
`k_infer_s1/s3` (csrc/k_rows.hpp, csrc/k_rows_split.hpp), launched by `rows_split`, `rows_blocks`, `rows_form` and
`rows_write_through` (csrc/gcnn_capi.hip).

THE RESTATEMENT says which wave of which block walks which 16-row tile -- index bookkeeping only, none of the kernels' float
arithmetic:
  form(n, nstage, cap)      rows_split (<= 256 tiles over the launch's row sets: one four-wave block per tile) or rows_blocks (8
                            waves above 1,024 tiles; spread while sum_want < cap and > 1,024 tiles; shares by tiles x stages once
                            sum_want > cap; the excess over cap taken from the largest program): split, nwaves, nb[], blk0[], grid
                            and which of the branches (spread, share, trim) were taken
  emb_cap(tiles)            the embedding launch's cap: 256, or 2 CUs - 3 from 8,192 tiles
  write_through(n)          the launch's largest row set has at most 32,768 rows
  launches(C, V, K, path)   the row-program launches of a path ("fused", "autograd_fwd", "autograd_bwd", "nograd", "score_state"),
                            each with its row sets and stage counts as gcnn_capi.hip passes them
  owner(form, p, tile)      (block, wave, trip) of a tile of program p: tile = bid + nblk wave, then += nblk NWAVES per trip
  tiles_of(form, p, ...)    the inverse: the tiles of a wave, including the one it prefetches past its last
  coverage(form, p, n)      every (tile stored, tile whose operands went into it) of program p, over its blocks, waves and trips
  audit(case)               what goes wrong for the planted rows: nothing, for the restatement itself
Every function takes `defect`, one of DEFECTS: the restatement with that one line changed.  tests/test_rowcases.py requires every
defect to lose, double or swap a planted row on a named case (`split257` and `waves8_at_1024` are consistent in themselves, as
`cost_f16` of tests/wgradcases.py is: they show as another partition, the planted rows sit with other blocks, waves and trips).

PLANTED COMPONENTS are those of tests/wgradcases.py: a cut k* adjacent only to variable v*, which is adjacent only to constraint
c*, nothing else touching the three, the target of k* a power of two (y_star(case), per case).  The three rows are given
independently; the builder is vectorised (no per-row draw), and a case makes large only the row sets its launch needs (the others
have SMALL rows).  Per case up to eight components sit on the rows `seam_rows` names for the launches under test: row n - 1, the
first row of the last tile, a tile of the last wave that has one, the first tile of a second trip, the last tile of the first
program and the first tile of the second.  No two planted rows of a row set are neighbours.
What is done so that the planted rows, and only they, decide the comparison with the fp64 oracle:
  * the planted rows' features are boost(case) times standard normal ones: a planted row of a forward program's output that is lost
    or replaced by its neighbour's then moves its cut's score by ten times the GPU test's 1e-4 (the model's scores hardly depend on a
    constraint two hops away otherwise);
  * the ordinary constraints and the ordinary cuts use disjoint halves of the free variables, so an ordinary constraint is on no path
    to a cut and has a gradient of exactly zero;
  * `settled`: the ordinary cuts take their own fp64 score as target, so their gradient is of rounding size.
  The ordinary rows still run through every kernel, and the cross-form comparison of tests/test_gpu_row_seams.py sees each of them.

A case is a dict: id, C, V, K, comps [{k, v, c}], under (the launches it is named for: [(path, launch name)]), seed."""
import functools

import numpy as np

TILE = 16
SPLIT_MAX_TILES = 256
CAP = 256
WAVES8_ABOVE = 1024       # tiles
WT_MAX_ROWS = 256 * 8 * 16
EMB_CAP_TILES = 8192
CUS = 256                 # MI355X
SMALL = 40                # rows of a row set that is not under test
DEFECTS = ("tile_floor", "row_le", "stride_nblk", "next_ops", "no_rebase", "no_trim", "split257", "waves8_at_1024")
# the planted target per case: the smallest power of two, from 1 up, that tests/test_rowcases.py proves strong enough: a factor >= 10
# over the GPU test's bound for every gradient tensor, and the bound's 3 gap term at most GAP_SHARE of its 1e-4 term; cases not listed
# take Y_STAR
GAP_SHARE = 0.25
Y_STAR = 1.0
Y_STARS = {
    "K/4097": 8.0, "K/16384": 32.0, "K/16385": 32.0, "V/32768": 4.0, "K/32768": 16.0, "K/32769": 16.0, "pair/trim": 2.0, "pair/256": 2.0,
    "emb/257": 2.0}
# the factor on the planted rows' features per case: the smallest power of two at which a planted row of any forward row program's
# output, lost or replaced by its neighbour's, moves its cut's fp64 score by at least 10 times the GPU test's 1e-4 (cases not listed: 1)
BOOSTS = {
    "n1": 8.0, "n15": 32.0, "n16": 32.0, "n17": 16.0, "n80": 32.0, "C/4096": 32.0, "V/4096": 16.0, "K/4096": 32.0,
    "C/4097": 16.0, "V/4097": 32.0, "K/4097": 8.0, "C/16384": 16.0, "V/16384": 8.0, "K/16384": 32.0, "C/16385": 16.0,
    "V/16385": 32.0, "K/16385": 32.0, "C/32768": 256.0, "V/32768": 64.0, "K/32768": 64.0, "C/32769": 32.0, "V/32769": 16.0,
    "K/32769": 8.0, "pair/trim": 16.0, "pair/256": 64.0, "pair/onetile": 16.0, "pair/zero": 2.0, "pair/1024": 32.0,
    "pair/1025": 8.0, "emb/256": 16.0, "emb/257": 16.0, "emb/8191": 64.0, "emb/8192": 32.0}
# cases rebuilt from another seed: no boost up to 1,024 reached the score factor, or (tests/wgradcases.py RESEED) the fp32 oracle sat so far
# from the fp64 one that the bound's 3 gap term would have decided instead of the 1e-4 term
RESEED = {
    "K/32768": 1, "pair/trim": 2, "emb/8192": 1}


def cdiv(a, b):
    return -(-a // b)


def ntiles(n):
    return cdiv(n, TILE) if n > 0 else 0


# ---- rows_split, rows_blocks, rows_form, rows_write_through ---------------------------------------------------------------------------
def form(n, nstage, cap=CAP, can_split=True, defect=None, waves=0, split_max=SPLIT_MAX_TILES):
    """The form of a launch over the row sets n[] with stage counts nstage[].  `can_split`: the launcher asks rows_split first (the
    forward launches; k_conv_bwd and k_tail_bwd never split).  `waves`, `split_max`: GCNN_ROWS_WAVES / GCNN_SPLIT_MAX_TILES of the
    tuning build.  grid: the row blocks the launch starts (the embedding launch adds its three fuse_weights blocks behind them)."""
    ntile = [ntiles(x) for x in n]
    total = sum(ntile)
    base = dict(ntile=ntile, total=total, spread=False, share=False, trim=False)
    if can_split and total <= split_max + (defect == "split257"):
        return dict(base, split=True, nwaves=4, nb=list(ntile), blk0=_cum(ntile), grid=total)
    eight = total >= WAVES8_ABOVE if defect == "waves8_at_1024" else total > WAVES8_ABOVE
    nwaves = waves if waves in (4, 8) else 8 if eight else 4
    want = [cdiv(t, nwaves) for t in ntile]
    work = [t * s for t, s in zip(ntile, nstage)]
    sum_want, sum_work = sum(want), sum(work)
    spread = sum_want < cap and total > WAVES8_ABOVE
    share = sum_want > cap
    nb = list(want)
    if share or spread:
        for i in range(len(n)):
            if nb[i] > 0:
                nb[i] = max(1, min(ntile[i] if spread else want[i], cdiv(cap * work[i], sum_work)))
    trim = False
    if share or spread:
        tot = sum(nb)
        while tot > cap and defect != "no_trim":
            big = 0
            for i in range(1, len(n)):
                if nb[i] > nb[big]:
                    big = i
            if nb[big] <= 1:
                break
            nb[big] -= 1
            tot -= 1
            trim = True
    grid = sum(nb)
    if defect == "no_trim":
        grid = min(grid, cap)        # the 257th block never runs
    return dict(base, split=False, nwaves=nwaves, nb=nb, blk0=_cum(nb), grid=grid, spread=spread, share=share, trim=trim)


def _cum(nb):
    out = [0]
    for b in nb:
        out.append(out[-1] + b)
    return out


def emb_cap(tiles, cus=CUS):
    return 2 * cus - 3 if tiles >= EMB_CAP_TILES else 256


def write_through(n):
    return max(n) <= WT_MAX_ROWS


def launches(C, V, K, path, cus=CUS):
    """[{name, sets, n, stages, can_split, cap}] in launch order."""
    emb = dict(name="k_embed_fwd", sets=("V", "C", "K"), n=(V, C, K), stages=(4, 3, 3), can_split=True,
               cap=emb_cap(ntiles(V) + ntiles(C) + ntiles(K), cus))
    one = lambda name, s, n, st: dict(name=name, sets=(s,), n=(n,), stages=(st,), can_split=True, cap=CAP)
    two = lambda name, sets, n, st: dict(name=name, sets=sets, n=n, stages=st, can_split=False, cap=CAP)
    fwd = [emb, one("k_conv_fwd<proj> v->c", "C", C, 4), one("k_conv_fwd<proj> c->v", "V", V, 4)]
    bwd = [two("k_conv_bwd {V, K}", ("V", "K"), (V, K), (5, 2)), two("k_conv_bwd {C}", ("C", None), (C, 0), (5, 2)),
           two("k_tail_bwd {V, C}", ("V", "C"), (V, C), (3, 2))]
    if path == "fused":
        out = fwd + [one("k_conv_turn", "K", K, 10)] + (bwd if K > 0 else [])
    elif path in ("autograd_fwd", "nograd"):
        out = fwd + [one("k_conv_fwd<readout>", "K", K, 4)]
    elif path == "autograd_bwd":
        out = ([two("k_conv_bwd {K}", ("K", None), (K, 0), (5, 2))] + bwd) if K > 0 else []
    elif path == "score_state":
        out = [dict(emb, name="k_infer_s1")] + fwd[1:] + [one("k_conv_fwd<readout>", "K", K, 4)]
    else:
        raise KeyError(path)
    return [l for l in out if sum(l["n"]) > 0]


def form_of(launch, defect=None, **knobs):
    return form(launch["n"], launch["stages"], launch["cap"], launch["can_split"], defect, **knobs)


# ---- the kernels' tile loops ---------------------------------------------------------------------------------------------------------
def owner(f, p, tile):
    """(block of the launch, wave, trip) that walks `tile` of program p; wave -1: the four waves of a split block share the tile."""
    if f["split"]:
        return f["blk0"][p] + tile, -1, 0
    nblk = f["nb"][p]
    trip, r = divmod(tile, nblk * f["nwaves"])
    wave, bid = divmod(r, nblk)
    return f["blk0"][p] + bid, wave, trip


def tiles_of(f, p, block, wave, n, defect=None):
    """The tiles wave `wave` of block `block` (an index into the launch) walks in program p of n rows, in trip order, and behind them
    the tile past its last whose operands it asks for (it loads nothing there)."""
    nblk = f["nb"][p]
    ntile = (n >> 4) if defect == "tile_floor" else ntiles(n)
    bid = block - (0 if defect == "no_rebase" else f["blk0"][p])
    if f["split"]:
        tile, stride = bid, nblk
    else:
        tile, stride = bid + nblk * wave, nblk * (1 if defect == "stride_nblk" else f["nwaves"])
    out = []
    while tile < ntile:
        out.append(tile)
        tile += stride
    return out, tile


def coverage(f, p, n, defect=None):
    """[(tile stored, tile whose operands went into it)] of program p over the blocks the launch starts for it."""
    out = []
    stride = f["nb"][p] * (1 if f["split"] or defect == "stride_nblk" else f["nwaves"])
    for block in range(f["blk0"][p], min(f["blk0"][p + 1], f["grid"])):
        for wave in range(1 if f["split"] else f["nwaves"]):
            tiles, _ = tiles_of(f, p, block, wave, n, defect)
            out += [(t, t + stride if defect == "next_ops" else t) for t in tiles]
    return out


def row_audit(f, p, n, rows, defect=None, what=""):
    """What happens to the rows `rows` of program p: a list of strings, empty when each is stored once from its own operands."""
    bad = []
    cov = coverage(f, p, n, defect)
    for r in rows:
        mine = [src for dst, src in cov if dst == r // TILE]
        if not mine:
            bad.append(f"{what}: row {r} (tile {r // TILE}) is stored by no wave")
        elif len(mine) > 1:
            bad.append(f"{what}: row {r} (tile {r // TILE}) is stored {len(mine)} times")
        elif mine[0] != r // TILE:
            bad.append(f"{what}: row {r} is made of the operands of row {r + TILE * (mine[0] - r // TILE)}"
                       + (" (past the set: zeros)" if mine[0] >= ntiles(n) else ""))
        if defect == "row_le" and mine and r == n - 1 and n % TILE:
            bad.append(f"{what}: row {n}, past the set, is computed and stored beside planted row {r}, and counted in its tile's sums")
    return bad


def seam_tiles(f, p, n):
    """{name: tile} of the seams of program p of n rows."""
    nt = ntiles(n)
    if nt == 0:
        return {}
    out = {"last": nt - 1}
    if not f["split"]:
        stride = f["nb"][p] * f["nwaves"]
        out["last wave"] = min(nt, stride) - 1        # the highest tile of the first trip: its wave is the last one that has a tile
        if stride < nt:
            out["second trip"] = stride
    if len([b for b in f["nb"] if b > 0]) > 1:
        out["last of first" if p == 0 else "first of second"] = nt - 1 if p == 0 else 0
    return out


def seam_rows(f, p, n):
    """Rows to plant for program p, most important first: n - 1, the first row of the last tile, a row of each other seam tile."""
    t = seam_tiles(f, p, n)
    if not t:
        return []
    rows = [n - 1, TILE * t["last"]]
    rows += [TILE * tile + min(7, n - 1 - TILE * tile) for name, tile in t.items() if name != "last"]
    return rows


def apart(rows, taken=()):
    got = []
    for r in rows:
        if all(abs(r - g) > 1 for g in got) and all(abs(r - g) > 1 for g in taken):
            got.append(r)
    return got


# ---- states ------------------------------------------------------------------------------------------------------------------------------
def y_star(case):
    return Y_STARS.get(case["id"], Y_STAR)


def boost(case):
    return BOOSTS.get(case["id"], 1.0)


def build(case, y_star_=None, boost_=None, scores=None):
    """(state 10-tuple, targets, components) -- tests/wgradcases.py `build` without its per-row draws: an ordinary row takes 1-4
    (constraints) or 1-6 (cuts) consecutive free variables from a random start.  The features of the planted rows are boost(case)
    times standard normal ones, so that a planted row lost or swapped in a forward program shows in its cut's score.
    `scores`: the model's fp64 scores of this state (the state does not depend on them); the ordinary cuts then take their own
    score as target instead of 0 .. 0.2 (`settled`)."""
    C, V, K = case["C"], case["V"], case["K"]
    ys = y_star(case) if y_star_ is None else y_star_
    bs = boost(case) if boost_ is None else boost_
    rng = np.random.default_rng(case["seed"])
    comps = [dict(c, star=None, leaves=[], targets=None) for c in case["comps"]]
    for key in "kvc":
        rows = [c[key] for c in comps if c[key] is not None]
        assert len(set(rows)) == len(rows), "components share a node"
    fv = np.setdiff1d(np.arange(V), [c["v"] for c in comps])

    def edges(n, planted, hi, fv):
        """planted: {row: variable}"""
        free = np.setdiff1d(np.arange(n), list(planted))
        deg = np.minimum(rng.integers(1, hi + 1, free.size), fv.size)
        ptr = np.concatenate([[0], np.cumsum(deg)])
        rows = np.repeat(free, deg)
        k = np.arange(ptr[-1]) - np.repeat(ptr[:-1], deg)
        cols = fv[(np.repeat(rng.integers(0, max(fv.size, 1), free.size), deg) + k) % max(fv.size, 1)] if fv.size else rows[:0]
        rows = np.concatenate([rows, np.fromiter(planted.keys(), np.int64, len(planted))])
        cols = np.concatenate([cols, np.fromiter(planted.values(), np.int64, len(planted))])
        order = np.lexsort((cols, rows))
        return np.stack([rows[order], cols[order]]).astype(np.int32)

    # the ordinary constraints take every other free variable and the ordinary cuts the rest: no ordinary constraint is on a path to a
    # cut, so its rows run through every kernel with a gradient of exactly zero (else the thousands of ordinary rows of a large
    # constraint set, each on a path to every ordinary cut, would outweigh the one planted row in every constraint-side tensor)
    cei = edges(C, {c["c"]: c["v"] for c in comps if c["c"] is not None}, 4, fv[1::2])
    kei = edges(K, {c["k"]: c["v"] for c in comps}, 6, fv[0::2])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    state = (f(C, 4), cei, f(cei.shape[1], 1), f(V, 14), f(K, 6), kei, f(kei.shape[1], 1), C, V, K)
    for key, idx in (("c", 0), ("v", 3), ("k", 4)):
        state[idx][[c[key] for c in comps if c[key] is not None]] *= np.float32(bs)
    y = rng.uniform(0, 0.2, K)
    if scores is not None:
        y = np.asarray(scores, np.float32).astype(np.float64)
    for c in comps:
        c["y0"] = float(y[c["k"]])
        y[c["k"]] = ys
    return state, y, comps


def settled(case, score_fn, y_star_=None, boost_=None):
    """`build` with every ordinary cut's target at its own score, `score_fn(state)` giving the model's fp64 scores.  With targets of
    0 .. 0.2 each of the thousands of ordinary rows of a large constraint or cut set weighs 1e-4 or more of some gradient tensor, and the
    fp64 oracle of such a state has 50 to 200 ReLU units within rounding of 0 whose flip is visible in a tensor (measured with
    tests/gradparity.py `ambiguous_units`): far more than a flip can be proven for, so whole-model parity under the 1e-4 bound would
    rest on luck.  Settled, the ordinary rows still run through every kernel but carry a gradient of rounding size; the gradients are
    those of the planted components, and an ambiguous unit can only sit under a planted row."""
    state, _, _ = build(case, y_star_, boost_)
    return build(case, y_star_, boost_, scores=score_fn(state))


# ---- the case list -------------------------------------------------------------------------------------------------------------------------
def _unique_launches(C, V, K):
    seen, out = set(), []
    for path in ("fused", "autograd_fwd", "autograd_bwd"):
        for l in launches(C, V, K, path):
            if l["name"] not in seen:
                seen.add(l["name"])
                out.append((path, l))
    return out


def wanted_rows(C, V, K, under):
    """{row set: rows to plant}: the seam rows of the launches named in `under` first, then those of the step's other launches."""
    want = {"C": [], "V": [], "K": []}
    ls = _unique_launches(C, V, K)
    for first in (True, False):
        for path, l in ls:
            if (l["name"] in under) == first:
                f = form_of(l)
                for p, s in enumerate(l["sets"]):
                    if s is not None:
                        want[s] += seam_rows(f, p, l["n"][p])
    return {s: apart(dict.fromkeys(r))[:8] for s, r in want.items()}


def plant(C, V, K, under):
    """Up to eight components: each row set's wanted rows, a set that runs out of them lending ordinary rows (position 5 or 9 of a
    tile that holds no wanted row, where there is one)."""
    want = wanted_rows(C, V, K, under)
    n_of = dict(C=C, V=V, K=K)
    rows = {}
    for s, w in want.items():
        filler = apart([r for t in range(ntiles(n_of[s])) for r in (TILE * t + 5, TILE * t + 9) if r < n_of[s]][:64], taken=w)
        if len(w) + len(filler) < 8:       # a tiny set: any row that is nobody's neighbour
            filler = apart(list(range(n_of[s])), taken=w)
        rows[s] = (w + apart(filler, taken=w))[:8]
    count = min(8, max(len(w) for w in want.values()), *(len(rows[s]) for s in "VK"), *((len(rows["C"]),) if C > 0 else ()))
    return [dict(k=rows["K"][i], v=rows["V"][i], c=rows["C"][i] if C > 0 else None) for i in range(count)]


SINGLE = ("k_conv_fwd<proj> v->c", "k_conv_fwd<proj> c->v", "k_conv_turn", "k_conv_fwd<readout>", "k_conv_bwd {C}", "k_conv_bwd {K}")
OF_SET = {"C": ("k_conv_fwd<proj> v->c", "k_conv_bwd {C}"), "V": ("k_conv_fwd<proj> c->v",),
          "K": ("k_conv_turn", "k_conv_fwd<readout>", "k_conv_bwd {K}")}
PAIRS = ("k_conv_bwd {V, K}", "k_tail_bwd {V, C}")
SMALL_SIZES = (1, 15, 16, 17, 80)
LARGE_SIZES = (4096, 4097, 16384, 16385, 32768, 32769)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(cid, C, V, K, under):
        out.append(dict(id=cid, C=C, V=V, K=K, under=tuple(under), comps=plant(C, V, K, under),
                        seed=sum(map(ord, cid)) + 1000 * RESEED.get(cid, 0)))

    # one row set per launch: the three sets at n rows each (small n), or one set at n rows beside two of SMALL rows
    for n in SMALL_SIZES:
        add(f"n{n}", n, n, n, SINGLE)
    for n in LARGE_SIZES:
        for s in "CVK":
            add(f"{s}/{n}", *(n if s == q else SMALL for q in "CVK"), OF_SET[s])
    # two-program launches: k_conv_bwd {V, K} (stages 5, 2) and k_tail_bwd {V, C} (stages 3, 2)
    add("pair/trim", 4096, 32768, 4096, PAIRS)                    # 244 + 13 and 237 + 20 = 257 blocks: the trim takes one from the first program
    add("pair/256", 16 * 99, 16 * 2046, 16 * 165, PAIRS)          # the rounded shares sum to exactly 256: 248 + 8 in both launches
    add("pair/onetile", 16, 32768, 16, PAIRS)                     # a second program of one tile (256 + 1 blocks, trimmed to 255 + 1)
    add("pair/zero", 0, 4097, SMALL, PAIRS[1:])                   # no constraint: k_tail_bwd's second program has no row
    add("pair/1024", 384, 16000, 384, PAIRS)                      # 1,000 + 24 tiles: four waves
    add("pair/1025", 400, 16000, 400, PAIRS)                      # 1,000 + 25 tiles: eight waves, spread
    # embeddings: 256 / 257 tiles over three unequal sets (split or not), 8,191 / 8,192 tiles (the cap)
    add("emb/256", 1296, 2000, 800, ("k_embed_fwd",))
    add("emb/257", 1296, 2000, 801, ("k_embed_fwd",))
    add("emb/8191", 160, 16 * 8171, 160, ("k_embed_fwd",))
    add("emb/8192", 160, 16 * 8172, 160, ("k_embed_fwd",))
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)


def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def launches_under(case_):
    """[(path, launch, form)] of the launches a case is named for."""
    return [(path, l, form_of(l)) for path, l in _unique_launches(case_["C"], case_["V"], case_["K"]) if l["name"] in case_["under"]]


def audit(case_, defect=None):
    """What goes wrong for the planted rows under `defect` in any row-program launch of the fused and the autograd step (nothing,
    for the restatement itself)."""
    key = {"C": "c", "V": "v", "K": "k"}
    bad = []
    for path, l in _unique_launches(case_["C"], case_["V"], case_["K"]):
        f = form_of(l, defect)
        for p, s in enumerate(l["sets"]):
            if s is not None and l["n"][p] > 0:
                rows = [c[key[s]] for c in case_["comps"]]
                bad += row_audit(f, p, l["n"][p], rows, defect, f"{l['name']} [{s}]")
    return bad
