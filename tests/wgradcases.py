"""States at the seams of the weight-gradient tail of a training step, and a restatement of its index arithmetic (host only, NumPy only).

The tail: `k_wgrad` with its four job bodies and the `d w_edge` pre-reduction, `k_reduce` with `fold_block` / `fold_chain`
(csrc/k_wgrad.hpp), and the host's `place_wg` / `conv_backward_edges` / `launch_edge_bwd_send` (csrc/gcnn_capi.hip).

THE RESTATEMENT says which input row ends in which sum -- index bookkeeping only, none of the kernels' float arithmetic:
  pending(C, V, K)          the 22 weight-gradient jobs in collection order (gcnn_backward), with the tensors each one feeds
  place(pend, ...)          place_wg: order (sharing rule), nblocks with the costs 10 and 16 + ceil(f2/4), the slots, the bisect,
                            nb, rows, blk0, slab0; `forced` is GCNN_WG_ROWS of the tuning build
  locate(job, r)            wgrad_body read backwards: (block, wave, batch, position in the batch, slab) of row r
  slab_rows(job)            wgrad_body + wg_body read forwards: {slab: rows added into it, with multiplicity}
  strided4(lo, hi)          the four-part strided sum of k_reduce / dw_reduce_block (16-row unroll and tail loop)
  fold_indices(np, step)    fold_chain's trips of 8 * step slabs over the parts of a block
  send_plan / sender_row    launch_edge_bwd_send's grid (lane slots, main blocks, long blocks) and the partial row a sender lands in
  dw_terms(plan)            dw_reduce_block's chunks and k_reduce's main and tail_n terms
  tensor_sums(case)         all of it composed: {tensor: rows (or partial rows) that reach it, with multiplicity}
Every function takes `defect`, one of DEFECTS: the restatement with that one line changed.  tests/test_wgradcases.py requires every
defect to lose or double a planted row (or to read a slab nobody wrote, or to move a planted partial row into the wrong term) on a
named case.

PLANTED COMPONENTS.  Weight gradients are affine in the targets once the forward pass is fixed, and a cut's target enters only
through 2 (s_k - y_k) / K.  A component is a cut k* adjacent only to variable v*, which is adjacent only to constraint c*; nothing
else touches the three.  With the target y* (Y_STAR) of k* large against the 0 .. 0.2 of the others, its gradient is a large
share of every tensor and flows through exactly one row of every job: k* in the seven cut-row jobs, v* in the variable-row jobs,
c* in the constraint-row jobs, one edge per convolution in d w_edge.  A case holds up to eight components at different rows.
Star components (d w_edge long-segment cases only): v* (or c*) also has LONG_DEG leaf neighbours of its own, so that the sender
segment holding the planted edge is longer than the long-segment threshold; such a component targets that convolution's
`feat_edge/kernel` only.

A case is a dict: id, lib ("product" | "wg16"), C, V, K, comps, known (longest segment known to the host), seed."""
import functools

import numpy as np

EMB = 64
WG_WAVES, WG_ROWS, WG_MAX_SLABS, WG_MAX_JOBS = 4, 64, 1024, 28
BATCH = 16                # rows per batch of loads (4 MFMA steps of 4 rows); the ring holds two
CUS = 256                 # MI355X
COST_PLAIN, COST_F, COST_F2 = 16, 10, 16      # sixteenths of the plain product's cost per row; f2 adds ceil(f2 / 4)
DW_CHUNK = 128
FOLD_BLOCKS = 33
EDGE_MAX_GRID, MAX_GRID = 8192, 2048
SLOTS4_DEG, SLOTS2_DEG = 40, 12
Y_STAR = 256.0              # the planted target: the smallest power of two that tests/test_wgradcases.py proves strong enough
LONG_DEG = 40             # leaves of a star component (> 32: long for one lane slot)
# cases rebuilt from another seed: tests/test_wgradcases.py measured a factor below 10 over the bound, or an fp32 oracle so far from the
# fp64 one (a ReLU unit near 0 under a planted row) that the bound's 3 gap term would have decided instead of the 1e-4 term
RESEED = {"aloneV/n1000/5": 1, "wg16/1-1-128": 1}
DEFECTS = ("live_le", "rend_short", "no_wrap", "no_zero_slab", "dw127", "long_with_main", "tail_short", "fold7", "cost_f16")
CONVS = ("cons_conv", "var_conv", "cut_conv")     # cv[0] (v -> c), cv[1] (c -> v), cv[2] (v -> k)


def cdiv(a, b):
    return -(-a // b)


# ---- the jobs as gcnn_backward collects them ---------------------------------------------------------------------------------------
def pending(C, V, K):
    """[{name, set, n, x, d, f, f2, fold, outs}] in collection order; x / d name the operands (the sharing rule compares them);
    outs: [(tensor, rows of the tensor the job's G covers as a slice, or "bias")]; fold: the convolution whose fold blocks read
    the job's slabs."""
    n_of = dict(C=C, V=V, K=K)
    out = []

    def job(name, rs, x, d, outs, f=0, f2=0, fold=None):
        if n_of[rs] > 0:
            out.append(dict(name=name, set=rs, n=n_of[rs], x=x, d=d, f=f, f2=f2, fold=fold, outs=outs))

    job("readout", "K", "Xk2", "gO1", [("out_1/kernel", "w"), ("out_1/bias", "b")])
    # (conv, receiver set, left set; operand names after conv_setup)
    io = {"cut_conv": ("K", "Z1k", "gXk2", "S3", "gZ1k", "Xk", "Xv2", "gPL3", "gPR3", "K"),
          "var_conv": ("V", "Z1v", "gXv2", "S2", "gZ1v", "Xc2", "Xv", "gPL2", "gPR2", "C"),
          "cons_conv": ("C", "Z1c", "gXc2", "S1", "gZ1c", "Xc", "Xv", "gPL1", "gPR1", "C")}
    for conv in ("cut_conv", "var_conv", "cons_conv"):
        recv, z1, gout, s, gz1, xl, xv, gpl, gpr, left = io[conv]
        xrecv = xl if recv == left else xv
        job(f"{conv}/out_2", recv, z1, gout, [(f"{conv}_out_2/kernel", "w"), (f"{conv}_out_2/bias", "b")])
        job(f"{conv}/fold", recv, s, gz1, [(f"{conv}_out_1/bias", "b")], fold=conv)
        job(f"{conv}/w1b", recv, xrecv, gz1, [(f"{conv}_out_1/kernel", "w1b")])
        job(f"{conv}/left", left, xl, gpl, [(f"{conv}_feat_left/kernel", "w"), (f"{conv}_feat_left/bias", "b")])
        job(f"{conv}/right", "V", xv, gpr, [(f"{conv}_feat_right/kernel", "w")])
    for rs, pre, f in (("C", "cons", 4), ("V", "var", 14), ("K", "cut", 6)):
        job(f"{pre}/emb_1", rs, f"{pre}_feats", f"gE1{rs}", [(f"{pre}_emb_1/kernel", "w"), (f"{pre}_emb_1/bias", "b")], f=f)
    for rs, pre, f in (("C", "cons", 4), ("V", "var", 14), ("K", "cut", 6)):
        job(f"{pre}/emb_2", rs, f"{pre}_feats", f"gX{rs}", [(f"{pre}_emb_2/kernel", "w"), (f"{pre}_emb_2/bias", "b")], f2=f)
    return out


def fold_outs(conv):
    """Tensors the fold blocks make of a fold job's slabs: (tensor, step of fold_chain)."""
    return [(f"{conv}_feat_final/kernel", 4), (f"{conv}_out_1/kernel", 4), (f"{conv}_feat_final/bias", 16)]


def nblocks(q, r, defect=None):
    c = (COST_PLAIN if defect == "cost_f16" else COST_F) if q["f"] else COST_F2 + cdiv(q["f2"], 4) if q["f2"] else COST_PLAIN
    return max(1, cdiv(q["n"] * c, 16 * r * WG_WAVES))


def place(pend, share=1, forced=0, defect=None):
    """place_wg: the jobs in launch order, each with nb, rows, blk0, slab0; and the chunk size the launch settled on."""
    used, order, last = [False] * len(pend), [], -1
    for _ in pend:
        pick = -1
        if last >= 0 and share:
            for i, q in enumerate(pend):
                if not used[i] and q["n"] == pend[last]["n"] and (q["x"] == pend[last]["x"] or q["d"] == pend[last]["d"]):
                    pick = i
                    break
        if pick < 0:
            for i, q in enumerate(pend):
                if not used[i] and (pick < 0 or q["n"] > pend[pick]["n"]):
                    pick = i
        used[pick] = True
        order.append(pick)
        last = pick
    slots = max(min(2 * CUS, WG_MAX_SLABS - WG_MAX_JOBS), len(pend))
    blocks_at = lambda r: sum(nblocks(q, r, defect) for q in pend)
    rows = WG_ROWS
    if blocks_at(rows) > slots:
        lo = hi = rows // 16
        while blocks_at(hi * 16) > slots and hi < (1 << 24):
            hi *= 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if blocks_at(mid * 16) > slots:
                lo = mid
            else:
                hi = mid
        rows = hi * 16
    if forced >= 16 and forced % 16 == 0 and blocks_at(forced) <= WG_MAX_SLABS:
        rows = forced
    jobs, blk, slab = [], 0, 0
    for i in order:
        q = dict(pend[i])
        nb = min(nblocks(q, rows, defect), cdiv(q["n"], 16 * WG_WAVES))
        q.update(nb=nb, rows=(cdiv(q["n"], nb * WG_WAVES) + 15) & ~15, blk0=blk, slab0=slab)
        blk += nb
        slab += nb
        jobs.append(q)
    return jobs, rows


# ---- wgrad_body / wg_body ----------------------------------------------------------------------------------------------------------
def row_block(j, bx, defect=None):
    """lb of block bx (an index into the weight-gradient blocks of the launch) of job j."""
    lb = bx - j["blk0"] + (j["blk0"] & 7) % j["nb"]
    if lb >= j["nb"] and defect != "no_wrap":
        lb -= j["nb"]
    return lb


def chunk(j, lb, wv, defect=None):
    rbeg = min(j["n"], (lb * WG_WAVES + wv) * j["rows"])
    rend = min(j["n"], rbeg + j["rows"])
    if defect == "rend_short" and rend > rbeg:
        rend -= 1
    return rbeg, rend


def locate(j, r):
    """(block, wave, batch, position, slab) of row r of job j."""
    ch, off = divmod(r, j["rows"])
    lb, wv = divmod(ch, WG_WAVES)
    t = (lb - (j["blk0"] & 7) % j["nb"]) % j["nb"]
    return j["blk0"] + t, wv, off // BATCH, off % BATCH, j["slab0"] + lb


def chunk_rows(rbeg, rend, defect=None):
    """Rows one wave adds up, with multiplicity: the two-batch ring over [rbeg, rend), loads clamped to rend - 1, `live` deciding."""
    got = []
    for row0 in range(rbeg, rend, 2 * BATCH):
        for u in range(2):
            if row0 + u * BATCH < rend:
                r = np.arange(row0 + u * BATCH, row0 + (u + 1) * BATCH)
                live = r <= rend if defect == "live_le" else r < rend
                got.append(np.minimum(r, rend - 1)[live])
    return np.concatenate(got) if got else np.zeros(0, np.int64)


def slab_rows(j, defect=None):
    """{slab: rows added into it}; a slab a block never stores is absent.  Rows of a block that falls outside the job (no wrap)
    are lost."""
    out = {}
    for bx in range(j["blk0"], j["blk0"] + j["nb"]):
        lb = row_block(j, bx, defect)
        parts = [chunk_rows(*chunk(j, lb, wv, defect), defect) for wv in range(WG_WAVES)]
        rows = np.concatenate(parts)
        if defect == "no_zero_slab" and rows.size == 0:
            continue
        out.setdefault(j["slab0"] + lb, []).append(rows)
    return {s: np.concatenate(v) for s, v in out.items()}


# ---- k_reduce, dw_reduce_block, fold_chain -------------------------------------------------------------------------------------------
def strided4(lo, hi, defect=None):
    """Indices in [lo, hi) the four parts add, in their order: part q takes lo + q, + 4, ...; four at a time while p + 12 < hi,
    then one at a time."""
    got = []
    for part in range(4):
        p = lo + part
        while p + 12 < hi:
            got += [p, p + 4, p + 8, p + 12]
            p += 16
        while p < (hi - 1 if defect == "tail_short" else hi):
            got.append(p)
            p += 4
    return got


def fold_indices(np_, step, defect=None):
    """Slabs [0, np_) as the groups of a fold block add them: group g starts at slab g and takes trips of 8 * step."""
    got = []
    for first in range(step):
        p = first
        while p < np_:
            got += [p + u * step for u in range(8) if p + u * step < np_]
            p += (7 if defect == "fold7" else 8) * step
    return got


# ---- the sender pass and d w_edge -------------------------------------------------------------------------------------------------------
def xcd_remap(bid, nblk):
    q, r, x, i = nblk >> 3, nblk & 7, bid & 7, bid >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + i


def send_plan(n_own, n_edges, max_deg):
    """launch_edge_bwd_send: lane slots, main blocks (= main partial rows), long blocks (= long partial rows)."""
    if n_own <= 0:
        return dict(slots=0, nmain=0, nlong=0, n_own=0)
    avg = n_edges / max(n_own, 1)
    slots = 4 if avg >= SLOTS4_DEG else 2 if avg >= SLOTS2_DEG else 1
    grid = min(cdiv(cdiv(n_own, 4 // slots), 4), EDGE_MAX_GRID)
    need = slots < 4 and (max_deg <= 0 or max_deg > 32 * slots)
    lb = ((max(1, min(cdiv(n_own, 4), MAX_GRID)) + 7) & ~7) if need else 0
    return dict(slots=slots, nmain=grid, nlong=lb, n_own=n_own)


def sender_row(plan, u, seg_len):
    """The partial row of d w_edge that sender u's edges are added into."""
    if plan["nlong"] and seg_len > 32 * plan["slots"]:
        return plan["nmain"] + u % plan["nlong"]
    item = u // (4 // plan["slots"])
    pos = (item // 4) % plan["nmain"]
    return _inverse_remap(plan["nmain"])[pos]


@functools.lru_cache(maxsize=None)
def _inverse_remap(nblk):
    inv = np.empty(nblk, np.int64)
    inv[[xcd_remap(b, nblk) for b in range(nblk)]] = np.arange(nblk)
    assert sorted(xcd_remap(b, nblk) for b in range(nblk)) == list(range(nblk))
    return inv


def sender_for_row(plan, row):
    """The first sender whose (short) segment lands in main partial row `row`."""
    return 4 * (4 // plan["slots"]) * xcd_remap(row, plan["nmain"])


def dw_terms(plan, defect=None):
    """{"main": partial rows that reach d w_edge through k_reduce's first term, "tail": through its tail_n term}, with multiplicity,
    and the chunk lists [(kind, p0, p1)]."""
    nmain, nparts = plan["nmain"], plan["nmain"] + plan["nlong"]
    nmc, nlc = cdiv(nmain, DW_CHUNK), cdiv(plan["nlong"], DW_CHUNK)      # the host's counts
    per = 127 if defect == "dw127" else DW_CHUNK
    chunks = []
    for c in range(nmc + nlc):
        if defect == "long_with_main":
            p0, lim = c * per, nparts
        else:
            p0, lim = (c * per, nmain) if c < nmc else (nmain + (c - nmc) * per, nparts)
        chunks.append(("main" if c < nmc else "tail", p0, max(p0, min(lim, p0 + per))))
    rows_of = [strided4(p0, p1, None) for _, p0, p1 in chunks]
    main = [r for c in strided4(0, nmc, defect) for r in rows_of[c]]
    tail = [r for c in strided4(0, nlc, defect) for r in rows_of[nmc + c]]
    return dict(main=main, tail=tail, chunks=chunks)


# ---- states ------------------------------------------------------------------------------------------------------------------------------
def comp(p, star=None):
    """A component with k*, v* and c* all at row p; star: "v" (v* has LONG_DEG leaf constraints) or "c" (c* has LONG_DEG leaf variables)."""
    return dict(k=p, v=p, c=p, star=star)


def _targets_of(c):
    return None if c["star"] is None else ("cons_conv_feat_edge/kernel",) if c["star"] == "v" else ("var_conv_feat_edge/kernel",)


def build(case, y_star=Y_STAR):
    """(state 10-tuple, targets, components with their leaves filled in)."""
    C, V, K = case["C"], case["V"], case["K"]
    rng = np.random.default_rng(case["seed"])
    comps = [dict(c) for c in case["comps"]]
    taken = {"C": {c["c"] for c in comps}, "V": {c["v"] for c in comps}, "K": {c["k"] for c in comps}}
    assert all(len(taken[s]) == len(comps) for s in taken), "components share a node"
    free = {s: [i for i in range(n) if i not in taken[s]] for s, n in (("C", C), ("V", V), ("K", K))}
    cons_e, cut_e = [], []
    for c in comps:   # leaves come off the end of the free rows
        c["leaves"] = []
        if c["star"]:
            rs = "C" if c["star"] == "v" else "V"
            c["leaves"] = [free[rs].pop() for _ in range(LONG_DEG)]
        cons_e.append((c["c"], c["v"]))
        cut_e.append((c["k"], c["v"]))
        cons_e += [(l, c["v"]) if c["star"] == "v" else (c["c"], l) for l in c["leaves"]]
    fv = np.asarray(free["V"], np.int64)

    def ordinary(rows, hi):
        for r in rows:
            if fv.size:
                d = int(rng.integers(1, hi + 1))
                yield from ((r, int(v)) for v in rng.choice(fv, min(d, fv.size), replace=False))

    cons_e += list(ordinary(free["C"], 4))
    cut_e += list(ordinary(free["K"], 6))

    def coo(e):
        a = np.asarray(sorted(set(e)), np.int64).reshape(-1, 2).T
        return a.astype(np.int32)

    cei, kei = coo(cons_e), coo(cut_e)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    state = (f(C, 4), cei, f(cei.shape[1], 1), f(V, 14), f(K, 6), kei, f(kei.shape[1], 1), C, V, K)
    y = rng.uniform(0, 0.2, K)
    for c in comps:
        c["y0"] = float(y[c["k"]])
        y[c["k"]] = y_star
        c["targets"] = _targets_of(c)
    return state, y, comps


def degrees(state):
    """(by-constraint, by-variable over constraint edges, by-cut, by-variable over cut edges) segment lengths."""
    cei, kei, C, V, K = state[1], state[5], state[7], state[8], state[9]
    return (np.bincount(cei[0], minlength=C), np.bincount(cei[1], minlength=V), np.bincount(kei[0], minlength=K),
            np.bincount(kei[1], minlength=V))


def send_plans(case, state):
    """{conv: plan} of the three sender passes: cons_conv and cut_conv send from the variables, var_conv from the constraints."""
    dc, dv1, _, dv2 = degrees(state)
    md = (lambda d: int(d.max()) if case["known"] and d.size else 0)
    E1, E2 = state[1].shape[1], state[5].shape[1]
    return {"cons_conv": send_plan(case["V"], E1, md(dv1)), "var_conv": send_plan(case["C"], E1, md(dc)),
            "cut_conv": send_plan(case["V"], E2, md(dv2))}


def planted_partials(case, state, comps):
    """{conv: [(component index, partial row)]} of the planted edges."""
    dc, dv1, _, dv2 = degrees(state)
    plans = send_plans(case, state)
    out = {c: [] for c in CONVS}
    for i, c in enumerate(comps):
        out["cons_conv"].append((i, sender_row(plans["cons_conv"], c["v"], dv1[c["v"]])))
        out["var_conv"].append((i, sender_row(plans["var_conv"], c["c"], dc[c["c"]])))
        out["cut_conv"].append((i, sender_row(plans["cut_conv"], c["v"], dv2[c["v"]])))
    return out


def placed(case, defect=None, share=1):
    return place(pending(case["C"], case["V"], case["K"]), share=share, forced=16 if case["lib"] == "wg16" else 0, defect=defect)


def tensor_sums(case, state, defect=None):
    """{tensor: (rows that reach it with multiplicity, unwritten slabs it reads)} for the weight-gradient tensors (rows of the job's
    row set) and {conv_feat_edge/kernel: {"main": partial rows, "tail": partial rows}}."""
    jobs, _ = placed(case, defect)
    out = {}
    for j in jobs:
        sr = slab_rows(j, defect)
        via = lambda idx: (np.concatenate([sr[j["slab0"] + s] for s in idx if j["slab0"] + s in sr] + [np.zeros(0, np.int64)]),
                           sorted({j["slab0"] + s for s in idx if j["slab0"] + s not in sr}))
        for tensor, _ in j["outs"]:
            out[tensor] = via(strided4(0, j["nb"], defect))
        if j["fold"]:
            for tensor, step in fold_outs(j["fold"]):
                out[tensor + ("#w1a" if tensor.endswith("out_1/kernel") else "")] = via(fold_indices(j["nb"], step, defect))
    for conv, plan in send_plans(case, state).items():
        if plan["n_own"] > 0:
            out[f"{conv}_feat_edge/kernel"] = dw_terms(plan, defect)
    return out


def audit(case, defect=None):
    """What goes wrong for the planted rows under `defect` (nothing, for the restatement itself): a list of strings."""
    state, _, comps = build(case)
    sums = tensor_sums(case, state, defect)
    jobs, _ = placed(case, defect)
    row_of = {"K": "k", "V": "v", "C": "c"}
    bad = []
    for j in jobs:
        names = [t for t, _ in j["outs"]] + ([t + ("#w1a" if t.endswith("out_1/kernel") else "") for t, _ in fold_outs(j["fold"])] if j["fold"] else [])
        for t in names:
            rows, unwritten = sums[t]
            if unwritten:
                bad.append(f"{t}: reads slabs {unwritten} that no block stored")
            for c in comps:
                if c["targets"] is None:
                    m = int((rows == c[row_of[j["set"]]]).sum())
                    if m != 1:
                        bad.append(f"{t}: row {c[row_of[j['set']]]} of job {j['name']} counted {m} times")
    plans = send_plans(case, state)
    for conv, rows in planted_partials(case, state, comps).items():
        terms = sums.get(f"{conv}_feat_edge/kernel")
        for i, r in rows:
            want = "main" if r < plans[conv]["nmain"] else "tail"
            for kind in ("main", "tail"):
                m = terms[kind].count(r)
                if m != (kind == want):
                    bad.append(f"{conv} d w_edge: partial row {r} (component {i}) counted {m} times in the {kind} term")
    return bad


# ---- the case list -------------------------------------------------------------------------------------------------------------------------
def seam_rows(jobs, n_of):
    """{row set: rows at which some job of that set has a seam}: first and last row of every chunk, both sides of every batch seam."""
    out = {"C": set(), "V": set(), "K": set()}
    for j in jobs:
        s = out[j["set"]]
        for ch in range(j["nb"] * WG_WAVES):
            rbeg = min(j["n"], ch * j["rows"])
            rend = min(j["n"], rbeg + j["rows"])
            if rbeg < rend:
                s.update((rbeg, rend - 1))
                for b in range(rbeg + BATCH, rend, BATCH):
                    s.update((b - 1, b))
    return {k: sorted(v) for k, v in out.items()}


def _split(rows, size=8):
    return [rows[i:i + size] for i in range(0, len(rows), size)]


def bisect_sizes():
    """(n below, n above): the largest C = V = n (K = 200) whose 64-row chunks still fit one resident round, and the next."""
    fits = lambda n: sum(nblocks(q, WG_ROWS) for q in pending(n, n, 200)) <= 512
    lo, hi = 64, 1 << 16
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo, hi


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(cid, lib, C, V, K, comps, known=True):
        out.append(dict(id=cid, lib=lib, C=C, V=V, K=K, comps=comps, known=known, seed=sum(map(ord, cid.replace("unknown", "known"))) + 1000 * RESEED.get(cid, 0)))     # (the unknown twin is the same state)

    # product library: the three row sets at n rows each, a component at every seam row of any job, eight per case; the two sides
    # of a seam (rows p, p + 1) go to different cases, so that a planted row's neighbours are ordinary rows
    def parts(rows):
        return [q for par in (0, 1) for q in _split([r for r in rows if r % 2 == par]) if q]

    for n in (1, 16, 17, 63, 64, 65, 127, 128, 129, 1000):
        jobs, _ = place(pending(n, n, n))
        rows = sorted(set().union(*seam_rows(jobs, n).values()) | {0, n - 1})
        for i, part in enumerate(parts(rows)):
            add(f"n{n}/{i}", "product", n, n, n, [comp(p) for p in part])
    # each row set on its own: the first and last row of every chunk of that set's jobs at 1,000 rows (the sets' jobs partition
    # differently: 64- and 96-row chunks, four, three and five blocks), the component's other two nodes on ordinary rows (position
    # 5 of a batch, never a seam)
    plain = lambda i: 16 * (3 + 2 * i) + 5
    jobs, _ = place(pending(1000, 1000, 1000))
    for rs in "KVC":
        ends = sorted({r for j in jobs if j["set"] == rs for ch in range(j["nb"] * WG_WAVES)
                       for r in (ch * j["rows"], min(1000, (ch + 1) * j["rows"]) - 1) if ch * j["rows"] < 1000})
        for i, part in enumerate(parts(ends)):
            add(f"alone{rs}/n1000/{i}", "product", 1000, 1000, 1000,
                [{"k": plain(q), "v": plain(q), "c": plain(q), "star": None, rs.lower(): p} for q, p in enumerate(part)])
    # the bisect: just below and just above; the last chunk of the longest job, row 0 (lb = 0: the block that wrapped) and chunk ends;
    # all three sets at once, then each on its own
    def apart(rows):
        got = []
        for r in rows:
            if all(abs(r - g) > 1 for g in got):
                got.append(r)
        return got

    for tag, n in zip(("below", "above"), bisect_sizes()):
        jobs, rows = place(pending(n, n, 200))
        longest = max(jobs, key=lambda j: j["nb"])
        last = (longest["n"] - 1) // longest["rows"] * longest["rows"]
        big = apart([n - 1, last, 0, rows - 1, 2 * rows, 3 * rows - 1])
        small = [199, 0, 63, 128, 191, 150]
        add(f"bisect/{tag}", "product", n, n, 200, [dict(k=k, v=p, c=p, star=None) for k, p in zip(small, big)])
        for rs in "KVC":
            add(f"alone{rs}/bisect/{tag}", "product", n, n, 200,
                [{"k": plain(q), "v": plain(q), "c": plain(q), "star": None, rs.lower(): p}
                 for q, p in enumerate(small[:5] if rs == "K" else big[:5])])
    # tuning library, GCNN_WG_ROWS = 16: 64 rows per slab; slabs per row set (C, V, K)
    for slabs in ((1, 3, 4), (5, 12, 13), (16, 17, 32), (32, 33, 3), (1, 1, 128), (1, 1, 129)):
        C, V, K = (64 * s for s in slabs)
        # per row set: the first row, the last, and the last row before / the first row of each seam slab (k_reduce's unroll ends
        # at slab 16, fold_chain's first trip at slab 32 (step 4) and 128 (step 16)); the sets are zipped into components, a set
        # that runs out of wanted rows lends ordinary ones
        rows = []
        for s in slabs:
            want = sorted({0, 64 * s - 1} | {64 * q + 63 for q in (15, 31, 127) if q < s} | {64 * q for q in (16, 32, 128) if q < s})
            rows.append(want + [r for r in range(5, 64 * s, 7) if all(abs(r - w) > 1 for w in want)][:8 - len(want)])
        add("wg16/" + "-".join(map(str, slabs)), "wg16", C, V, K,
            [dict(c=rows[0][i], v=rows[1][i], k=rows[2][i], star=None) for i in range(8)])
    # d w_edge: main partial rows 127 / 128 / 129 and 256 / 257 (one lane slot: 16 senders per main block)
    for nmain in (127, 128, 129, 256, 257):
        n = 16 * nmain
        plan = send_plan(n, 3 * n, 4)
        assert plan["nmain"] == nmain and plan["slots"] == 1
        senders = sorted({sender_for_row(plan, r) for r in (0, 127, 128, nmain - 1) if r < nmain})
        for known in (True, False):
            add(f"dw/{nmain}/{'known' if known else 'unknown'}", "product", n, n, 96, [dict(k=3 * i, v=s, c=s, star=None) for i, s in enumerate(senders)], known)
        if True:                    # a long-segment pass that has work: the planted edge in the first and the last long row
            nlong = send_plan(n, 3 * n, 0)["nlong"]
            comps = [dict(k=0, v=nlong, c=nlong, star="v"), dict(k=3, v=nlong - 1, c=nlong - 1, star="v"),
                     dict(k=6, v=2 * nlong, c=2 * nlong, star="c"), dict(k=9, v=2 * nlong - 1, c=2 * nlong - 1, star="c"),
                     dict(k=12, v=senders[-1] + 3, c=senders[-1] + 3, star=None)]
            add(f"dw/{nmain}/long", "product", n, n, 96, comps)
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)


def case(cid):
    return next(c for c in cases() if c["id"] == cid)
