"""Graphs at the seams of the edge passes, two value fills for them, and a restatement of the walk (host only, NumPy only).

The passes: `k_edge_fwd`, `k_edge_fwd_block`, the long-row blocks (`edge_long_rows`) and `k_edge_bwd_send` (csrc/k_edge.hpp) with the
host's `launch_edge_fwd` / `launch_edge_bwd_send` (csrc/gcnn_capi.hip); and the standalone scatter-sum pass (`k_seg_sum`).

THE RESTATEMENT says which edge of an owner's segment [beg, end) is added by which lane group, chunk, step and slot -- index
bookkeeping only:
  edge_slots / fwd_plan / send_plan    the launch formulas: lane slots S, block-per-segment rule, main grid (cap 8,192), long blocks
  walk(n, S, U)                        one lane group over n edges: chunks of G = 16 S, full steps of U S edges, one masked step
  shares(n, NG)                        the contiguous shares of the NG lane groups of a block that serves one row together
  row_paths(lens, plan)                which rows the main blocks serve (item, trip), which the finder (block, round), which nobody
  multiplicity(ptr, plan, U)           all of it composed: how often every edge of the list is added
Every function takes `defect`, one of DEFECTS; tests/test_edgecases.py requires each to change an exact expected output on a named
case.  S = lanes / 16, G = 16 S, F = 4 S (forward step), B = 2 S (backward step), T = 32 S (long threshold, S < 4).

TWO FILLS.  grid_fill: every value on a dyadic grid (coef k/4 in [-1.5, 0.5] with e_shift 0.5, e_scale 2, so c is k/2 in [-2, 2];
w k/4 in [-2, 2]; PL, PR integers in [-4, 4]; dS integers in [-2, 2]; s1 = +-0.5), so J is k/8 with |J| <= 12 and every sum the
kernels form is exact in fp32 in any order while sum |terms| < 2^24 grid units -- `expected` asserts that from the data and works
in integers.  Ties J == 0 occur by themselves (3 to 4 % of the elements) and are forced on the edges of `ties` (c = 0 against a table row that is
the negative of the other, signed zeros included).  float_fill: standard normal values and 256 matched pairs (a receiver of degree
1 whose sender has degree 1) with P_recv = -fl32(fma(c, w, P_send)) rounded exactly, so that the kernels' own expression gives 0.

A case is a dict: id, S, n_left, n_var, el / ev / l_ptr (edges sorted by left row), v_ptr / pv (the by-variable order is
el[pv], ev[pv]), known (longest segments given to the library), pair_l / pair_v, ties (edge positions in the by-left order), rows
(kind per left row: "craft", "tied", "fill", "pair")."""
import functools
from fractions import Fraction

import numpy as np

EMB = 64
EDGE_U, EDGE_UB = 4, 2
EDGE_MAX_GRID, MAX_GRID = 8192, 2048
SLOTS4_DEG, SLOTS2_DEG = 40, 12
LONG_NT = 256                # rows a finder block looks at per round
BLOCK_MAX_OWN, BLOCK_DEG, INFER_S4_OWN = 4096, 48, 16384
N_PAIRS, N_TIE_VARS, N_GEN = 256, 8, 248          # the variable side: general rows, tie rows, pair rows (512 in all)
E_SHIFT, E_SCALE = 0.5, 2.0
S1 = (0.5, -0.5)
DEFECTS = ("masked_drop_last", "slot_past_end", "thresh_lt", "tie_active", "neg_max", "share_overlap", "one_trip", "one_round",
           "long_dw_left_out")
NONE, MAIN, LONG, BLOCK = 0, 1, 2, 3


def cdiv(a, b):
    return -(-a // b)


# ---- launch formulas ----------------------------------------------------------------------------------------------------------------
def edge_slots(n_own, n_edges):
    avg = n_edges / max(n_own, 1)
    return 4 if avg >= SLOTS4_DEG else 2 if avg >= SLOTS2_DEG else 1


def long_threshold(slots):
    return 0x7fffffff if slots >= 4 else 32 * slots


def long_grid(n_own):
    return (max(1, min(cdiv(n_own, 4), MAX_GRID)) + 7) & ~7


def _main(slots, n_own, max_deg):
    grid = min(cdiv(cdiv(n_own, 4 // slots), 4), EDGE_MAX_GRID)
    need = slots < 4 and (max_deg <= 0 or max_deg > long_threshold(slots))
    return dict(kind="main", slots=slots, grid=grid, lb=long_grid(n_own) if need else 0, n_own=n_own)


def fwd_plan(n_own, n_edges, max_deg, count):
    """launch_edge_fwd (without an inference plan): kind "block" (a block per segment) or "main"; the launch's recorded name."""
    if n_own <= BLOCK_MAX_OWN and n_edges >= BLOCK_DEG * n_own:
        return dict(kind="block", slots=4, grid=n_own, lb=0, n_own=n_own, name="k_edge_fwd_block<count>" if count else "k_edge_fwd_block")
    p = _main(4 if (not count and n_own <= INFER_S4_OWN) else edge_slots(n_own, n_edges), n_own, max_deg)
    p["name"] = ("k_edge_fwd<count> + long segments" if p["lb"] else "k_edge_fwd<count>") if count else "k_edge_fwd"
    return p


def send_plan(n_own, n_edges, max_deg):
    """launch_edge_bwd_send; n_parts = grid + lb partial rows of d w_edge, the main blocks' first."""
    p = _main(edge_slots(n_own, n_edges), n_own, max_deg)
    p["name"] = "k_edge_bwd_send + long segments" if p["lb"] else "k_edge_bwd_send"
    return p


def xcd_remap(bid, nblk):
    bid = np.asarray(bid)
    q, r, x, i = nblk >> 3, nblk & 7, bid & 7, bid >> 3
    return np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + i


def main_items(plan, defect=None):
    """Work items (one wave's 4 / S owners) the main blocks reach, every trip of every wave of every block."""
    rpw = 4 // plan["slots"]
    nwork, nblk = cdiv(plan["n_own"], rpw), plan["grid"]
    first = (xcd_remap(np.arange(nblk), nblk)[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    trips = 1 if defect == "one_trip" else cdiv(nwork, nblk * 4)
    items = (first[None, :] + (np.arange(trips) * nblk * 4)[:, None]).reshape(-1)
    return items[items < nwork]


# ---- the walk -----------------------------------------------------------------------------------------------------------------------
def walk(n, slots, unroll, defect=None):
    """(offsets, full) of every term one lane group adds over a segment (or share) of n edges: offsets into it, with multiplicity;
    full: the term belongs to a full step.  A chunk is the G edges loaded one per lane; a step takes unroll * slots of them."""
    G, step = 16 * slots, unroll * slots
    off, full = [], []
    for base in range(0, n, G):
        cnt = min(G, n - base)
        i0 = 0
        while i0 + step <= cnt:
            off += range(base + i0, base + i0 + step)
            full += [True] * step
            i0 += step
        if i0 < cnt:
            lim = cnt - 1 if defect == "masked_drop_last" else cnt
            for i in range(i0, i0 + step):          # i = i0 + u * slots + slot
                if i < lim:
                    off.append(base + i)
                    full.append(False)
                elif i == cnt and defect == "slot_past_end":     # the masked lane's shuffle fetched the chunk's first edge
                    off.append(base)
                    full.append(False)
    return np.asarray(off, np.int64), np.asarray(full, bool)


def shares(n, ng, defect=None):
    """[(b, e)] of the ng lane groups that serve one row of n edges together."""
    share = cdiv(n, ng)
    out = []
    for grp in range(ng):
        b = min(n - 1 if defect == "share_overlap" and n > 0 else n, grp * share)
        out.append((b, min(n, b + share)))
    return out


@functools.lru_cache(maxsize=None)
def segment_terms(n, path, slots, unroll, defect=None):
    """(offsets, full, group) of every term added for a row of n edges served on `path`."""
    if path == NONE:
        z = np.zeros(0, np.int64)
        return z, z.astype(bool), z
    if path == MAIN:
        off, full = walk(n, slots, unroll, defect)
        return off, full, np.zeros(off.size, np.int64)
    if path == BLOCK:
        slots = 4
    offs, fulls, grps = [], [], []
    for g, (b, e) in enumerate(shares(n, 256 // (16 * slots), defect)):
        off, full = walk(e - b, slots, unroll, defect)
        offs.append(off + b)
        fulls.append(full)
        grps.append(np.full(off.size, g, np.int64))
    return np.concatenate(offs), np.concatenate(fulls), np.concatenate(grps)


def row_paths(lens, plan, defect=None):
    """Per owner row: NONE, MAIN, LONG or BLOCK; and the trip of the item loop (main rows) / the finder's round (long rows)."""
    lens = np.asarray(lens)
    r = np.arange(lens.size)
    if plan["kind"] == "block":
        return np.full(lens.size, BLOCK), np.zeros(lens.size, np.int64)
    slots, thr = plan["slots"], long_threshold(plan["slots"])
    trip = (r // (4 // slots)) // (plan["grid"] * 4)
    main = (lens < thr) if defect == "thresh_lt" else (lens <= thr)
    if defect == "one_trip":
        main &= trip == 0
    path = np.where(main, MAIN, NONE)
    rnd = np.zeros(lens.size, np.int64)
    if plan["lb"]:
        rnd = (r // plan["lb"]) // LONG_NT        # thread t of block b looks at row (q0 + t) * lb + b in round q0 / 256
        lng = lens > thr
        if defect == "one_round":
            lng &= rnd == 0
        path = np.where(lng, LONG, path)
    return path, np.where(path == LONG, rnd, trip)


def multiplicity(ptr, plan, unroll, defect=None):
    """How often every edge of an owner-ordered list is added."""
    lens = np.diff(ptr)
    path, _ = row_paths(lens, plan, defect)
    mult = np.zeros(int(ptr[-1]), np.int64)
    for p in np.unique(path):
        for n in np.unique(lens[path == p]):
            if n == 0:
                continue
            off, _, _ = segment_terms(int(n), int(p), plan["slots"], unroll, defect)
            m = np.bincount(off, minlength=n)
            rows = np.flatnonzero((path == p) & (lens == n))
            mult[ptr[rows][:, None] + np.arange(n)[None, :]] = m[None, :]
    return mult


def classify(case, e, unroll, known=None):
    """("full" | "masked", "main" | "long" | "block") of edge e (by-left order) in the pass whose owners are the left rows."""
    l = int(case["el"][e])
    n = int(case["l_ptr"][l + 1] - case["l_ptr"][l])
    plan = left_plan(case, unroll, known)
    path = int(row_paths(np.diff(case["l_ptr"]), plan)[0][l])
    off, full, _ = segment_terms(n, path, plan["slots"], unroll)
    hit = np.flatnonzero(off == e - case["l_ptr"][l])
    assert hit.size == 1
    return ("full" if full[hit[0]] else "masked"), {MAIN: "main", LONG: "long", BLOCK: "block"}[path]


def max_degs(case, known=None):
    known = case["known"] if known is None else known
    return (int(np.diff(case["l_ptr"]).max()), int(np.diff(case["v_ptr"]).max())) if known else (0, 0)


def left_plan(case, unroll, known=None):
    """The plan of the pass that walks the crafted list: the counting forward (unroll 4) or the sender pass (unroll 2)."""
    md = max_degs(case, known)[0]
    E = case["el"].size
    return fwd_plan(case["n_left"], E, md, True) if unroll == EDGE_U else send_plan(case["n_left"], E, md)


def plans(case, recv_is_left):
    """{"fwd": counting forward, "infer": forward without counts, "send": sender pass} of one orientation."""
    ml, mv = max_degs(case)
    E = case["el"].size
    n_recv, m_recv, n_send, m_send = (case["n_left"], ml, case["n_var"], mv) if recv_is_left else (case["n_var"], mv, case["n_left"], ml)
    return dict(fwd=fwd_plan(n_recv, E, m_recv, True), infer=fwd_plan(n_recv, E, m_recv, False), send=send_plan(n_send, E, m_send))


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
def _seed(cid):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(cid.replace("unknown/seams", "seams").replace("unknown/long", "long")))


def _graph(cid, S, rows, known=True):
    """rows: [(length, kind)] of the left side in row order; kind "pair" rows have length 1 and are matched to the pair variables
    in order; "tied" rows get forced ties on their first, middle and last edge, "longtie" rows (long crafted rows) in the middle."""
    rng = np.random.default_rng(_seed(cid))
    lens = np.asarray([n for n, _ in rows], np.int64)
    kinds = np.asarray([k for _, k in rows])
    n_left = lens.size
    l_ptr = np.zeros(n_left + 1, np.int64)
    np.cumsum(lens, out=l_ptr[1:])
    E = int(l_ptr[-1])
    el = np.repeat(np.arange(n_left), lens)
    ev = rng.integers(0, N_GEN, E)
    pair_l = np.flatnonzero(kinds == "pair")
    assert pair_l.size == N_PAIRS and (lens[pair_l] == 1).all()
    pair_v = N_GEN + N_TIE_VARS + rng.permutation(N_PAIRS)
    ev[l_ptr[pair_l]] = pair_v
    ties, tie_var = [], []
    for i, l in enumerate(np.flatnonzero((kinds == "tied") | (kinds == "longtie"))):
        n = int(lens[l])
        pos = {n // 2} if kinds[l] == "longtie" else {0, n // 2, n - 1}
        for p in sorted(pos):
            ties.append(int(l_ptr[l]) + p)
            tie_var.append(N_GEN + i % N_TIE_VARS)
    ties = np.asarray(ties, np.int64)
    ev[ties] = tie_var
    n_var = N_GEN + N_TIE_VARS + N_PAIRS
    pv = np.argsort(ev, kind="stable")
    v_ptr = np.zeros(n_var + 1, np.int64)
    np.cumsum(np.bincount(ev, minlength=n_var), out=v_ptr[1:])
    assert (np.diff(v_ptr)[pair_v] == 1).all()
    assert edge_slots(n_left, E) == S, (cid, E / n_left)
    return dict(id=cid, S=S, n_left=n_left, n_var=n_var, el=el, ev=ev, l_ptr=l_ptr, v_ptr=v_ptr, pv=pv, known=known, pair_l=pair_l,
                pair_v=pair_v, ties=ties, rows=kinds)


def _shuffled(cid, rows):
    order = np.random.default_rng(_seed(cid) + 7).permutation(len(rows))
    return [rows[i] for i in order]


def _pairs():
    return [(1, "pair")] * N_PAIRS


def _tied(S):
    """Twins that carry the forced ties: first, middle and last edge on full and masked steps of both passes."""
    G, F, B = 16 * S, 4 * S, 2 * S
    return [(n, "tied") for n in (1, B + 1, F + 1, G + 1, G + F + 1)]


def _fill_until(rows, lo, hi, ok, seed):
    """Filler rows of lo .. hi edges until ok(rows) holds."""
    rng = np.random.default_rng(seed)
    rows = list(rows)
    for _ in range(100000):
        if ok(rows):
            return rows
        rows.append((int(rng.integers(lo, hi + 1)), "fill"))
    raise AssertionError("filler never met the conditions")


def _mean(rows):
    return sum(n for n, _ in rows) / len(rows)


def _seam_ok(S, min_rows):
    lo, hi = {1: (0, SLOTS2_DEG), 2: (SLOTS2_DEG, SLOTS4_DEG), 4: (SLOTS4_DEG, 1e9)}[S]

    def ok(rows):
        n = len(rows)
        grid = min(cdiv(cdiv(n, 4 // S), 4), EDGE_MAX_GRID)
        return n >= min_rows and lo + 1 <= _mean(rows) < hi - 1 and grid % 8 != 0 and (S == 4 or n % (4 // S) != 0)
    return ok


FILL_DEG = {1: (1, 5), 2: (20, 39), 4: (44, 60)}
LONG_LENS = (255, 256, 257, 493, 1000, 2049)


def seam_lengths(S):
    """Every length 0 .. 2 G + 1 that the main blocks serve: for S < 4 the threshold T = 2 G ends the list (2 G + 1 = T + 1 is a
    long row and belongs to the long cases); for S = 4 also the long rows of the other classes, in the main kernel."""
    G = 16 * S
    return list(range(0, 2 * G + (2 if S == 4 else 1))) + (list(LONG_LENS) if S == 4 else [])


def long_lengths(S):
    T = 32 * S
    return [T + 1, T + 2, 2 * T] + list(LONG_LENS)


def _seams(cid, S, ascending=False, known=True):
    rows = [(n, "craft") for n in seam_lengths(S)] + _tied(S) + _pairs()
    rows = _fill_until(rows, *FILL_DEG[S], _seam_ok(S, {1: 700, 2: 0, 4: 4200}[S]), _seed(cid))
    rows = sorted(rows, key=lambda r: r[0]) if ascending else _shuffled(cid, rows)
    return _graph(cid, S, rows, known)


def _long(cid, S, known=True):
    rows = [(n, "craft") for n in seam_lengths(S)] + _tied(S) + _pairs()
    lng = [(n, "longtie") for n in long_lengths(S)]
    rows = _fill_until(rows, *FILL_DEG[S], lambda r: _seam_ok(S, 0)(r + lng), _seed(cid))
    rows = _shuffled(cid, rows)
    mid = len(rows) // 2                           # long rows at row 0, next to each other in the middle, at the last row
    rows = [lng[0]] + rows[:mid] + lng[2:] + rows[mid:] + [lng[1]]
    return _graph(cid, S, rows, known)


def _block(cid):
    rows = [(n, "craft") for n in (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)] + _tied(4) + _pairs()
    rows = _fill_until(rows, 100, 140, lambda r: sum(n for n, _ in r) >= BLOCK_DEG * len(r) + 64, _seed(cid))
    assert len(rows) <= BLOCK_MAX_OWN
    return _graph(cid, 4, _shuffled(cid, rows))


TRIP_FILL = {1: 1, 2: 12, 4: 40}


def _trip(cid, S):
    """One trip of the item loop (4 * 8,192 items of 4 / S owners) and 37 owners more; seam lengths in the rows behind the trip."""
    G, F, lo = 16 * S, 4 * S, TRIP_FILL[S]
    first = 4 * EDGE_MAX_GRID * (4 // S)
    head = _pairs() + _tied(S)
    head += [(lo + i % 2, "fill") for i in range(first - len(head))]
    head = _shuffled(cid, head)
    tail = [(n, "craft") for n in (0, 1, F - 1, F, F + 1, G - 1, G, G + 1, 2 * G, 1, F + 1)] + [(n, "tied") for n in (F + 1, G + 1)]
    tail += [(lo + i % 2, "fill") for i in range(37 - len(tail))]
    tail = _shuffled(cid + "/tail", tail)
    return _graph(cid, S, head + tail)


def _finder2(cid):
    """One round of the finder (256 rows per thread block of 2,048) and 512 owners more, long rows in reach of the second round only."""
    n = LONG_NT * MAX_GRID + 512
    rows = [(1, "fill")] * n
    for i in range(N_PAIRS):
        rows[1000 + 2001 * i] = (1, "pair")
    rows[5], rows[LONG_NT * MAX_GRID + 7], rows[n - 1] = (33, "longtie"), (100, "longtie"), (493, "longtie")
    rows[11], rows[LONG_NT * MAX_GRID + 30] = (5, "tied"), (3, "tied")
    return _graph(cid, 1, rows)


@functools.lru_cache(maxsize=None)
def case(cid):
    p = cid.split("/")
    if p[0] == "seams":
        return _seams(cid, int(p[1][1:]), ascending=p[-1] == "asc")
    if p[0] == "long":
        return _long(cid, int(p[1][1:]))
    if p[0] == "unknown":
        S = int(p[2][1:])
        return _seams(cid, S, known=False) if p[1] == "seams" else _long(cid, S, known=False)
    if p[0] == "block":
        return _block(cid)
    if p[0] == "trip":
        return _trip(cid, int(p[1][1:]))
    if p[0] == "finder2":
        return _finder2(cid)
    raise KeyError(cid)


SMALL = ("seams/S1", "seams/S2", "seams/S4", "seams/S1/asc", "seams/S2/asc", "seams/S4/asc", "long/S1", "long/S2",
         "unknown/seams/S1", "unknown/seams/S2", "unknown/long/S1", "unknown/long/S2", "block")
LARGE = ("trip/S1", "trip/S2", "trip/S4", "finder2/S1")
IDS = SMALL + LARGE
FLOAT_IDS = tuple(c for c in IDS if c != "finder2/S1")       # the second finder round runs on the grid fill only


def csr(case, by_left):
    """(ptr, oth, order): the owner-ordered list; order maps its positions to positions of the by-left order."""
    if by_left:
        return case["l_ptr"], case["ev"], np.arange(case["el"].size)
    return case["v_ptr"], case["el"][case["pv"]], case["pv"]


# ---- fills --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_fill(cid):
    c = case(cid)
    rng = np.random.default_rng(_seed(cid) + 1)
    E = c["el"].size
    q = rng.integers(-6, 3, E)                      # coef = q / 4; c = (coef + 0.5) * 2 = (q + 2) / 2
    q[c["ties"]] = -2
    w4 = rng.integers(-8, 9, EMB)
    PL = rng.integers(-4, 5, (c["n_left"], EMB)).astype(np.float32)
    PR = rng.integers(-4, 5, (c["n_var"], EMB)).astype(np.float32)
    for k in range(N_TIE_VARS):                     # tie variable k: a row with zeros of both signs; its partners hold the negative
        PR[N_GEN + k, ::k + 2] = -0.0 if k % 2 else 0.0
    PR[N_GEN:N_GEN + N_TIE_VARS, 5] = -0.0
    tl, tv = c["el"][c["ties"]], c["ev"][c["ties"]]
    PL[tl] = -PR[tv]
    PL[tl[::3], 5] = -0.0                           # and both zeros negative: J = -0
    f = dict(coef=(q / 4).astype(np.float32), w=(w4 / 4).astype(np.float32), PL=PL, PR=PR,
             dS_l=rng.integers(-2, 3, (c["n_left"], EMB)).astype(np.float32), dS_v=rng.integers(-2, 3, (c["n_var"], EMB)).astype(np.float32),
             c2=(q + 2).astype(np.int32), w4=w4.astype(np.int32))
    assert np.array_equal((f["coef"] + np.float32(E_SHIFT)) * np.float32(E_SCALE) * 2, f["c2"])
    return f


def round_f32(x: Fraction) -> float:
    """x rounded to the nearest fp32, ties to even, by integer arithmetic (normal and subnormal range)."""
    if x == 0:
        return 0.0
    sign, ax = (-1 if x < 0 else 1), abs(x)
    e = ax.numerator.bit_length() - ax.denominator.bit_length()
    if Fraction(2) ** e > ax:
        e -= 1                                       # 2^e <= ax < 2^(e+1)
    scale = Fraction(2) ** (max(e, -126) - 23)
    q = ax / scale
    n, rem = divmod(q.numerator, q.denominator)
    if 2 * rem > q.denominator or (2 * rem == q.denominator and n % 2):
        n += 1
    return sign * float(n * scale)


def fma_f32(a, b, c):
    """fl32(a * b + c) element-wise for fp32 arrays, rounded once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    out = [round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())]
    return np.asarray(out, np.float64).astype(np.float32).reshape(a.shape)


def prenorm_c(coef):
    return (coef + np.float32(E_SHIFT)) * np.float32(E_SCALE)


@functools.lru_cache(maxsize=None)
def float_fill(cid, recv_is_left):
    c = case(cid)
    rng = np.random.default_rng(_seed(cid) + 2)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    f = dict(coef=f32(c["el"].size), w=f32(EMB), PL=f32(c["n_left"], EMB), PR=f32(c["n_var"], EMB))
    pl, pv = c["pair_l"], c["pair_v"]
    cw = prenorm_c(f["coef"][c["l_ptr"][pl]])[:, None]
    if recv_is_left:
        f["PL"][pl] = -fma_f32(cw, f["w"][None, :], f["PR"][pv])
    else:
        f["PR"][pv] = -fma_f32(cw, f["w"][None, :], f["PL"][pl])
    f["dS_l"], f["dS_v"] = np.ones((c["n_left"], EMB), np.float32), np.ones((c["n_var"], EMB), np.float32)
    return f


# ---- expected values ----------------------------------------------------------------------------------------------------------------
CHUNK = 1 << 16


def _seg_add(out, keys, x):
    """out[k] += sum of the rows of x with key k."""
    if keys.size == 0:
        return
    if (keys[1:] < keys[:-1]).any():
        order = np.argsort(keys, kind="stable")
        keys, x = keys[order], x[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    out[keys[starts]] += np.add.reduceat(x, starts, axis=0, dtype=np.int64 if x.dtype.kind in "iub" else x.dtype)


def _to_left_order(case, by_left, mult):
    if mult is None or by_left:
        return mult
    out = np.empty_like(mult)
    out[case["pv"]] = mult
    return out


def expected(cid, s1, recv_is_left, defect=None):
    """The exact outputs of one orientation on the grid fill, from integer arithmetic: S, N, d_recv, d_send, d_w, dw_main, dw_tail
    (fp32 arrays).  With a defect: what a library with that defect would give."""
    c, f = case(cid), grid_fill(cid)
    p = plans(c, recv_is_left)
    walk_d = defect if defect in ("masked_drop_last", "slot_past_end", "thresh_lt", "share_overlap", "one_trip", "one_round") else None
    rptr, sptr = csr(c, recv_is_left)[0], csr(c, not recv_is_left)[0]
    mf = mb = None
    if walk_d:
        mf = _to_left_order(c, recv_is_left, multiplicity(rptr, p["fwd"], EDGE_U, walk_d))
        mb = _to_left_order(c, not recv_is_left, multiplicity(sptr, p["send"], EDGE_UB, walk_d))
    long_send = row_paths(np.diff(sptr), p["send"])[0] == LONG
    n_recv, n_send = rptr.size - 1, sptr.size - 1
    i8 = np.int8                                      # |J| <= 12 in eighths: every per-edge quantity fits a byte
    PL8, PR8, w4 = (8 * f["PL"]).astype(i8), (8 * f["PR"]).astype(i8), f["w4"].astype(i8)
    dS = (f["dS_l"] if recv_is_left else f["dS_v"]).astype(i8)
    A, N, T = (np.zeros((n, EMB), np.int64) for n in (n_recv, n_recv, n_send))
    DW = np.zeros((2, EMB), np.int64)
    pos = s1 > 0 or defect == "neg_max"
    for a in range(0, c["el"].size, CHUNK):
        l, v, c2 = c["el"][a:a + CHUNK], c["ev"][a:a + CHUNK], f["c2"][a:a + CHUNK, None].astype(i8)
        J8 = c2 * w4[None, :] + PL8[l] + PR8[v]
        act = (J8 > 0) if pos else (J8 < 0)
        if defect == "tie_active":
            act |= J8 == 0
        recv, send = (l, v) if recv_is_left else (v, l)
        h, cnt = J8 * act, act.view(i8)
        t = dS[recv] * act
        if mf is not None:
            h, cnt, t = h * mf[a:a + CHUNK, None], cnt * mf[a:a + CHUNK, None], t * mb[a:a + CHUNK, None]
        _seg_add(A, recv, h)
        _seg_add(N, recv, cnt)
        _seg_add(T, send, t)
        ct, ls = c2 * t, long_send[send]
        DW[0] += ct.sum(0, dtype=np.int64)
        if ls.any():
            DW[1] += ct[ls].sum(0, dtype=np.int64)
    DW[0] -= DW[1]
    if defect is None:
        # Every partial sum is exact in fp32 whatever the order: sum |terms| < 2^24 units, per output.  The terms of S have one sign
        # (sum |terms| = |sum|); |t| <= 2 and |c t| <= 2 |c| bound the sender pass from the degrees and the coefficients.
        sdeg = np.diff(sptr)
        for name, m in (("S", np.abs(A).max(initial=0)), ("N", N.max(initial=0)), ("d_send", 2 * sdeg.max(initial=0)),
                        ("d_w", 2 * int(np.abs(f["c2"]).sum()))):
            assert m < 1 << 24, (cid, name, int(m))
    if defect == "long_dw_left_out":
        DW[1] = 0
    f32, s = np.float32, np.float32(s1)
    dw_main, dw_tail = DW[0].astype(f32) * f32(s1 / 2), DW[1].astype(f32) * f32(s1 / 2)
    return dict(S=A.astype(f32) * f32(s1 / 8), N=N.astype(f32), d_recv=(dS * N).astype(f32) * s, d_send=T.astype(f32) * s,
                d_w=(DW[0] + DW[1]).astype(f32) * f32(s1 / 2), dw_main=dw_main, dw_tail=dw_tail)


def reference_S(cid, s1, recv_is_left):
    """fp64 reference of the forward on the float fill."""
    c, f = case(cid), float_fill(cid, recv_is_left)
    n_recv = c["n_left"] if recv_is_left else c["n_var"]
    S = np.zeros((n_recv, EMB))
    PL, PR, w = f["PL"].astype(np.float64), f["PR"].astype(np.float64), f["w"].astype(np.float64)
    cc = (f["coef"].astype(np.float64) + np.float64(np.float32(E_SHIFT))) * np.float64(np.float32(E_SCALE))
    for a in range(0, c["el"].size, CHUNK):
        l, v = c["el"][a:a + CHUNK], c["ev"][a:a + CHUNK]
        J = PL[l] + cc[a:a + CHUNK, None] * w[None, :] + PR[v]
        _seg_add(S, l if recv_is_left else v, np.maximum(s1 * J, 0.0))
    return S


# ---- scatter-sum --------------------------------------------------------------------------------------------------------------------
SEG_U, SEG_SLOTS, SEG_MAX_GRID = 16, 4, 8192
SCATTER_LENS = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000)
SCATTER_IDS = ("lens", "trip")


def seg_trips(n_recv):
    """Trips of k_seg_sum's item loop (a wave per receiver, four per block)."""
    return cdiv(n_recv, 4 * min(cdiv(n_recv, 4), SEG_MAX_GRID))


@functools.lru_cache(maxsize=None)
def scatter_case(sid):
    """(lens, index sorted by receiver, integer-valued messages in that order, d_out)."""
    rng = np.random.default_rng(len(sid))
    if sid == "lens":
        lens = np.asarray(SCATTER_LENS + SCATTER_LENS[::-1])
    else:
        lens = rng.integers(0, 3, 4 * SEG_MAX_GRID + 5)
        lens[-5:] = (0, 1, 5, 65, 129)
    idx = np.repeat(np.arange(lens.size), lens)
    msg = rng.integers(-8, 9, (idx.size, EMB)).astype(np.float32)
    d_out = rng.integers(-8, 9, (lens.size, EMB)).astype(np.float32)
    return lens, idx, msg, d_out


def scatter_expected(sid):
    lens, idx, msg, _ = scatter_case(sid)
    out = np.zeros((lens.size, EMB), np.int64)
    _seg_add(out, idx, msg.astype(np.int64))
    return out.astype(np.float32)
