"""What every block of every call layout needs, in Python integers from the dims (helper for test_host_sanitizers.py): the size of
each array or block behind each offset of the 20 layout structs of include/gcnn_hip.h, restated from the header's descriptions of
the uploads, downloads and arenas.  `blocks_of(fid, words, L)` returns regions -- (name, total, [(offset, size), ...]) -- and
the test asserts, per region, that no block starts before the one in front of it ends and that the last ends inside the total.
Sizes are what the kernels read and write (the library may round them up); where a block's size is a device-dependent query
(the radix sort's temporary storage) it is 0 here, a lower bound."""
from __future__ import annotations

EMB = 64
SEL_MAX_CUTS, IPLAN_MAX_VARS = 4096, 32768
IB_TABLE = 4 * 7 * 72
MB_TABLE = 4 * (7 * 72 + 16 + 64)


def al(x, a=16):
    return (x + a - 1) // a * a


def chunks(n):
    return -(-n // 256)


def workspace_floats(c, v, k, e1, e2):
    """gcnn_workspace_floats: activations and gradients (64 floats a row: 14 C-row arrays, 16 V-row, 14 K-row), 12 ReLU masks (2 floats
    a row), 1,024 weight-gradient slabs, per convolution the edge-weight partials, their pre-reduction, the active-edge counts and
    the folded weights, the PreNorm partial sums, the explicit ids of the longer edge list, the loss head's partials."""
    a4 = lambda x: al(x, 4)  # noqa: E731
    total = 14 * a4(EMB * c) + 16 * a4(EMB * v) + 14 * a4(EMB * k) + 4 * (a4(2 * c) + a4(2 * v) + a4(2 * k))
    total += a4(1024 * (EMB * EMB + 2 * EMB))
    fuse = (EMB * EMB + EMB) + 2 * EMB * EMB + EMB
    for rows in (c, v, k):
        total += a4(16384 * EMB) + a4(16384 // 128 * EMB) + a4(rows * EMB) + a4(fuse)
    total += a4(2 * (1024 * 16 + 2 * 16)) + a4(max(e1, e2)) + a4((k + 15) // 16 * 2 * EMB)
    return total


def select_ws(cuts, forced, max_cuts):
    return max((cuts + forced) * ((max_cuts + 63) // 64) * 16, 16)


def lp_scratch(R, V, K):
    return (al(16 * R) + al(32 * K) + al(16 * (chunks(V) + 1)) + al(16 * (chunks(R) + 1)) + al(16 * (chunks(K) + 1)) + al(8 * K) +
            al(4 * (chunks(V) + chunks(R) + chunks(K) + 1)))


def hyb_scratch(V, K):
    return al(32 * K) + al(4 * K) + al(8 * (chunks(V) + 1)) + al(4 * (chunks(V) + chunks(K) + 1))


def lpa_scratch(V, b):
    dR, dN, dE = b[0], b[1], b[3]
    return (al(16 * dR) + al(16 * (chunks(dR) + 1)) + al(4 * (chunks(dR) + 1)) + al(8 * V) + al(4 * (chunks(V) + 1)) + al(4 * V) + al(8 * dN) +
            2 * al(4 * dE))


def lpd_scratch(R, V, C):
    return 2 * al(16 * (chunks(R) + 1)) + al(4 * V) + al(4 * (chunks(V) + 1)) + al(4 * C) + al(4 * R)


def forced_sizes(f, fe):
    return [4 * (f + 1), 4 * fe, 4 * fe]


def lp_snap_sizes(d):
    R, V, K, NR, NK, inc = d[0], d[1], d[2], d[3], d[4], d[5]
    P = V if inc else 0
    return [16, 4 * (R + 1), 4 * NR, 8 * NR, 8 * R, 8 * R, 8 * R, R, V, 8 * V, 8 * V, 8 * V, V, 8 * V, 8 * V, 8 * P, 8 * P, 4 * (K + 1), 4 * NK,
            8 * NK, 8 * K, 8 * K]


def state_dims(d):
    return (d[7], d[1], d[2], d[8], d[4])      # n_state_rows, n_cols, n_cuts, n_state_edges, cut_nnz


def after_append(d, b):
    d = list(d)
    d[0] += b[0]; d[3] += b[1]; d[7] += b[2]; d[8] += b[3]  # noqa: E702
    return d


def after_remove(d, m):
    d = list(d)
    d[0] -= m[0]; d[3] -= m[1]; d[7] -= m[2]; d[8] -= m[3]  # noqa: E702
    return d


# ---- regions of each struct -------------------------------------------------------------------------------------------------------

def infer_regions(L, dims, pre="", forced=None, out_tail=0, more_arena=()):
    """gcnn_infer_layout for `dims`; forced = (F, FE, offsets) behind the inputs; out_tail bytes behind the flags; more_arena blocks."""
    c, v, k, e1, e2 = dims
    sizes = [4 * (2 * v + 8 + c + 1 + k + 1), 16 * c, 8 * e1, 4 * e1, 56 * v, 24 * k, 8 * e2, 4 * e2]
    ins = list(zip(L.in_off, sizes))
    if forced:
        ins += list(zip(forced[2], forced_sizes(forced[0], forced[1])))
    outs = list(zip(L.out_off, [4 * k, 4 * k, 16 + out_tail]))
    dev = [4 * (v + 1), 4 * e1, 4 * e1, 4 * e1, L.out_bytes, 4 * workspace_floats(*dims)]
    arena = [(0, L.in_bytes)] + list(zip(L.dev_off[2:], dev)) + list(more_arena)
    zero = [(L.dev_off[0], 4 * (c + 1)), (L.dev_off[1], 4 * (k + 1))]
    return [(pre + "in", L.in_bytes, ins), (pre + "out", L.out_bytes, outs), (pre + "arena", L.arena_bytes, arena),
            (pre + "zero block", L.in_off[1], [(L.in_off[0], 4 * (2 * v + 8))] + zero)]


def union_regions(L, dims_list, nf, nfe, mode, pre="", n_close=1, table=IB_TABLE, sel_offsets=False, fwd_ws=None, extra=(), out_bytes=None):
    """gcnn_ibatch_layout of a union: extra = [(offset, size)] behind the selection workspace; out_bytes: the download block's size
    where a caller has enlarged L.out_bytes afterwards."""
    n = len(dims_list)
    c, v, k, e1, e2 = (sum(d[i] for d in dims_list) for i in range(5))
    f, fe = sum(nf), sum(nfe)
    max_cuts = max([d[2] for d in dims_list if d[2] <= SEL_MAX_CUTS] + [0])
    zero = al(16 * n) + al(4 * (c + n_close)) + al(4 * (k + n_close)) + (al(4 * (k + 1)) if sel_offsets else 0)
    sizes = [table, zero, 16 * c, 8 * e1, 4 * e1, 56 * v, 24 * k, 8 * e2, 4 * e2] + forced_sizes(f, fe)
    outs = [4 * k, 4 * k, 4 * n, 16 * n]
    if fwd_ws is None:
        fwd_ws = 4 * workspace_floats(c, v, k, e1, e2)
    down = L.out_bytes if out_bytes is None else out_bytes
    dev = [4 * e1, 4 * e1, 4 * e2, 4 * e1, 4 * e1, 4 * e1, 4 * (v + n_close), 4 * e1, 4 * e1, 4 * fe, 0, down, fwd_ws,
           select_ws(k, f, max_cuts) if mode == 2 else 0]
    arena = [(0, L.in_bytes)] + list(zip(L.dev_off[:14], dev)) + list(extra)
    totals = (L.total.n_cons, L.total.n_vars, L.total.n_cuts, L.total.n_cons_edges, L.total.n_cut_edges, L.n_forced, L.n_forced_entries,
              L.n_states, L.max_cuts)
    assert totals == (c, v, k, e1, e2, f, fe, n, max_cuts), (totals, (c, v, k, e1, e2, f, fe, n, max_cuts))
    return [(pre + "in", L.in_bytes, list(zip(L.in_off, sizes))), (pre + "out", down, list(zip(L.out_off, outs))),
            (pre + "arena", L.arena_bytes, arena)]


def round_regions(L, d, present, nf, nfe, extra_out=0, pre=""):
    """gcnn_lp_round_layout for the LP `d`; returns the regions."""
    R, V, K, NK = d[0], d[1], d[2], d[4]
    opt = lambda bit: 8 * V if present & bit else 0  # noqa: E731
    sizes = [16, 8 * R, R, V, 8 * V, 8 * V, opt(1), opt(2), opt(4), opt(8), 4 * (K + 1), 4 * NK, 8 * NK, 8 * K, 8 * K]
    sel = nf >= 0
    ins = list(zip(L.in_off, sizes)) + list(zip(L.forced_off, forced_sizes(nf if sel else 0, nfe if sel else 0)))
    outs = list(zip(L.out_off, [4 * K, 4 * K, 16, 16, 16, 4 * K + extra_out]))
    sd = state_dims(d)
    dev = [L.in_bytes, 56 * V, 24 * K, 8 * NK, 4 * NK, 4 * (K + 1), L.out_bytes, 4 * workspace_floats(*sd), 16, lp_scratch(0, V, K),
           select_ws(K, nf, K) if sel else 0]
    return [(pre + "in", L.in_bytes, ins), (pre + "out", L.out_bytes, outs), (pre + "arena", L.arena_bytes, list(zip(L.dev_off, dev)))]


def append_block(L, b, base=0):
    dR, dN = b[0], b[1]
    sizes = [4 * (dR + 1), 4 * dN, 8 * dN, 8 * dR, 8 * dR]
    return list(zip([o for o in L.block_off], sizes)), base + L.block_bytes


def lp_regions(L, d, nf, nfe, pre=""):
    sel = nf >= 0
    K = d[2]
    snaps = list(zip(L.snap_off, lp_snap_sizes(d)))
    out = [(pre + "snapshot", L.snap_bytes, snaps), (pre + "in", L.in_bytes, snaps + list(zip(L.forced_off, forced_sizes(nf if sel else 0, nfe if sel else 0)))),
           (pre + "scratch", L.scratch_bytes, [(0, lp_scratch(d[0], d[1], d[2]))])]
    if L.call_supported:
        sd = state_dims(d)
        out += infer_regions(L.state, sd, pre + "state.", out_tail=32 + al(4 * K))
        out.append((pre + "out", L.out_bytes, list(zip(L.out_off, [4 * K, 4 * K, 16, 16, 16, 4 * K]))))
        out.append((pre + "arena", L.arena_bytes, [(0, L.state.arena_bytes), (L.ws_off, select_ws(K, nf, K) if sel else 0), (L.lp_off, L.in_bytes),
                                                   (L.scratch_off, L.scratch_bytes)]))
    return out


def lpset_regions(L, S_arena, dims_list, nf, nfe, mode, front, pre="lp."):
    """gcnn_lp_batch_layout around a union whose arena is S_arena bytes."""
    n = len(dims_list)
    K = sum(d[2] for d in dims_list)
    f, fe = (sum(nf), sum(nfe)) if mode == 2 else (0, 0)
    assert L.table_bytes >= front + 16 and L.n_snapshots == n
    ins = [(0, L.table_bytes)] + [(L.snap_base[s], sum(al(x) for x in lp_snap_sizes(d))) for s, d in enumerate(dims_list)]
    ins += list(zip(L.forced_off, forced_sizes(f, fe)))
    outs = list(zip(L.out_off, [4 * K, 4 * K, 4 * n, 16 * n, 16 * n, 4 * K]))
    arena = [(0, S_arena), (L.up_off, L.in_bytes), (L.out_dev_off, L.out_bytes)]
    arena += [(L.scratch_off + L.scratch_base[s], lp_scratch(d[0], d[1], d[2])) for s, d in enumerate(dims_list)]
    return [(pre + "in", L.in_bytes, ins), (pre + "out", L.out_bytes, outs), (pre + "arena", L.arena_bytes, arena)]


def mbatch_regions(ML, dims_list, nf, nfe, mode, model_of, n_models, pre=""):
    per = [[0] * 5 for _ in range(n_models)]
    for d, m in zip(dims_list, model_of):
        per[m] = [a + b for a, b in zip(per[m], d)]
    ws = [al(4 * workspace_floats(*p), 256) for p in per]
    e1, v = sum(d[3] for d in dims_list), sum(d[1] for d in dims_list)
    L = ML.u
    extra = [(L.dev_off[14], 4 * e1), (L.dev_off[15], 4 * (v + 1)), (ML.table_off, ML.table_bytes)]
    out = union_regions(L, dims_list, nf, nfe, mode, pre, n_close=n_models, table=al(MB_TABLE), sel_offsets=mode == 2, fwd_ws=sum(ws), extra=extra)
    end = L.dev_off[13]
    out.append((pre + "model workspaces", end, [(ML.ws_off[m], ws[m]) for m in range(n_models)]))
    assert ML.ws_off[0] >= L.dev_off[12] and ML.n_models == n_models and ML.table_bytes > 0
    return out


def ensemble_regions(EL, dims_list, nf, nfe, mode, n_models, pre=""):
    c, v, k, e1, e2 = (sum(d[i] for d in dims_list) for i in range(5))
    L, M = EL.u, n_models
    row = al(4 * k)
    ws = al(4 * workspace_floats(c, v, k, e1, e2), 256)
    solo_out = al(4 * k) * 2 + al(4 * len(dims_list)) + 16 * len(dims_list)
    out = union_regions(L, dims_list, nf, nfe, mode, pre, fwd_ws=al(M * row, 256) + M * ws, extra=[(EL.table_off, EL.table_bytes)], out_bytes=solo_out)
    assert EL.member_stride >= row and EL.n_models == M and EL.table_bytes > 0
    # the download reaches from the output block over the members' rows, which open the forward-workspace block
    rows = [(L.dev_off[11] + EL.member_off + m * EL.member_stride, 4 * k) for m in range(M)]
    out.append((pre + "download", L.dev_off[11] + L.out_bytes, [(L.dev_off[11], solo_out)] + rows))
    out.append((pre + "member block", L.dev_off[13], [(L.dev_off[12], M * row)] + [(EL.ws_off[m], ws) for m in range(M)]))
    return out


def plan(member, edit):
    """The solo call of one member of gcnn_lp_rounds(_edit): the dims after its edits and which blocks it carries."""
    d, present, nf, nfe, has_app, b = member[:10], member[10], member[11], member[12], member[13], member[14:22]
    has_rem, m = (member[22], member[23:31]) if edit else (0, None)
    mid = after_remove(d, m) if has_rem else list(d)
    after = after_append(mid, b) if has_app else mid
    return d, mid, after, present, nf, nfe, (b if has_app else None), (m if has_rem else None)


def solo_sizes(member, edit):
    """in_bytes, out_bytes, arena_bytes (lower bounds, from the blocks alone) of the member's solo call."""
    d, mid, after, present, nf, nfe, b, m = plan(member, edit)
    R, V, K, NK = after[0], after[1], after[2], after[4]
    sel = nf >= 0
    opt = lambda bit: 8 * V if present & bit else 0  # noqa: E731
    rin = sum(al(x) for x in [16, 8 * R, R, V, 8 * V, 8 * V, opt(1), opt(2), opt(4), opt(8), 4 * (K + 1), 4 * NK, 8 * NK, 8 * K, 8 * K] +
              forced_sizes(nf if sel else 0, nfe if sel else 0))
    extra = (16 if b else 0) + (16 if m else 0)
    rout = 2 * al(4 * K) + 48 + al(4 * K) + extra
    sd = state_dims(after)
    rarena = sum(al(x, 256) for x in [rin, 56 * V, 24 * K, 8 * NK, 4 * NK, 4 * (K + 1), rout, 4 * workspace_floats(*sd), 16, lp_scratch(0, V, K),
                                      select_ws(K, nf, K) if sel else 0])
    in_bytes, arena = rin, rarena
    if b:
        blk = al(8 * b[1] + 16 * b[0] + 4 * (b[0] + 1) + 4 * b[1], 256)
        in_bytes += blk
        arena = blk + al(arena, 256) + lpa_scratch(mid[1], b)
    if m:
        lst = al(4 * m[0], 256)
        in_bytes += lst
        arena = lst + al(arena, 256) + lpd_scratch(d[0], d[1], d[7])
    return in_bytes, rout, arena, after


def rounds_regions(L, members, edit):
    n = len(members)
    solo = [solo_sizes(mem, edit) for mem in members]
    ins = [(L.in_off[i], solo[i][0]) for i in range(n)]
    arena = [(0, L.in_bytes)] + [(L.arena_off[i], solo[i][2]) for i in range(n)]
    counts = []
    for i, mem in enumerate(members):
        d, mid, after, present, nf, nfe, b, m = plan(mem, edit)
        if m:
            counts.append((L.remove_counts_off[i], al(4 * d[1]) + al(4 * (chunks(d[1]) + 1))))
            assert L.arena_off[i] <= L.remove_scratch_off[i] and L.remove_scratch_off[i] + lpd_scratch(d[0], d[1], d[7]) <= L.arena_off[i] + solo[i][2]
        if b:
            counts.append((L.counts_off[i], al(8 * mid[1]) + al(4 * (chunks(mid[1]) + 1))))
            assert L.arena_off[i] <= L.scratch_off[i] and L.scratch_off[i] + lpa_scratch(mid[1], b) <= L.arena_off[i] + solo[i][2] + 256
        assert L.arena_off[i] <= L.member_round_off[i] < L.arena_off[i] + max(solo[i][2], 1)
        assert L.in_size[i] >= solo[i][0] and L.out_size[i] >= solo[i][1]
    arena += [(L.counts_base, L.counts_bytes), (L.out_base, L.out_bytes), (L.table_off, L.table_bytes)]
    outs = [(L.out_off[i], solo[i][1]) for i in range(n)]
    assert L.table_bytes > 0 and L.n == n
    return [("in", L.in_bytes, ins), ("out", L.out_bytes, outs), ("arena", L.arena_bytes, arena),
            ("counts", L.counts_base + L.counts_bytes, counts)]


# ---- the records ------------------------------------------------------------------------------------------------------------------

class _Words:
    def __init__(self, w):
        self.w, self.at = w, 0

    def take(self, n):
        self.at += n
        return self.w[self.at - n:self.at]

    def one(self, n):
        self.take(1)
        return self.take(n)

    def many(self, n_each, forced=True, models=False):
        n, k, mask = self.take(3)
        items = [self.take(n_each) for _ in range(k)]
        nf, nfe = (self.take(k), self.take(k)) if forced else ([0] * k, [0] * k)
        if mask & 2:
            nf = [0] * k
        if mask & 4:
            nfe = [0] * k
        mo = self.take(k) if models else None
        return items, nf, nfe, mo


def blocks_of(fid, words, L):
    """The regions of the accepted layout L that record (fid, words) produced."""
    r = _Words(words)
    if fid == 10:
        return infer_regions(L, r.one(5))
    if fid == 11:
        d, (nf, nfe) = r.one(5), r.take(2)
        ws = (L.ws_off, select_ws(d[2], nf, d[2]))
        out = infer_regions(L.infer, d, forced=(nf, nfe, L.forced_off), out_tail=16, more_arena=[ws])
        assert L.n_kept_off + 4 <= L.infer.out_bytes and L.n_kept_off >= L.infer.out_off[2] + 16
        return out
    if fid in (12, 13, 15):
        items, nf, nfe, mo = r.many(5, models=fid == 13)
        tail = r.take(1 if fid == 12 else 2)
        mode = tail[0]
        if mode != 2:
            nf, nfe = [0] * len(items), [0] * len(items)
        if fid == 12:
            return union_regions(L, items, nf, nfe, mode)
        if fid == 13:
            return mbatch_regions(L, items, nf, nfe, mode, mo, tail[1])
        return ensemble_regions(L, items, nf, nfe, mode, tail[1])
    if fid == 14:
        d, (nf, nfe, mode, nm) = r.one(5), r.take(4)
        sel = mode == 2
        return ensemble_regions(L, [d], [nf if sel else 0], [nfe if sel else 0], mode, nm)
    if fid == 16:
        d, (nf, nfe) = r.one(10), r.take(2)
        return lp_regions(L, d, nf, nfe)
    if fid in (17, 18, 27):
        items, nf, nfe, mo = r.many(10, models=fid == 18)
        tail = r.take(1 if fid == 17 else 2)
        mode = tail[0]
        if mode != 2:
            nf, nfe = [0] * len(items), [0] * len(items)
        sd = [state_dims(d) for d in items]
        if fid == 17:
            return union_regions(L.state, sd, nf, nfe, mode, "state.") + lpset_regions(L, L.state.arena_bytes, items, nf, nfe, mode, IB_TABLE)
        if fid == 18:
            return (mbatch_regions(L.models, sd, nf, nfe, mode, mo, tail[1], "models.") +
                    lpset_regions(L.lp, L.models.u.arena_bytes, items, nf, nfe, mode, MB_TABLE))
        return ensemble_regions(L.ens, sd, nf, nfe, mode, tail[1], "ens.") + lpset_regions(L.lp, L.ens.u.arena_bytes, items, nf, nfe, mode, IB_TABLE)
    if fid == 26:
        d, (nf, nfe, mode, nm) = r.one(10), r.take(4)
        sel = mode == 2
        f, fe = [nf if sel else 0], [nfe if sel else 0]
        return ensemble_regions(L.ens, [state_dims(d)], f, fe, mode, nm, "ens.") + lpset_regions(L.lp, L.ens.u.arena_bytes, [d], f, fe, mode, IB_TABLE)
    if fid == 19:
        d, (nf, nfe) = r.one(10), r.take(2)
        C, V, K, E1, E2 = state_dims(d)
        snaps = list(zip(L.snap_off, lp_snap_sizes(d)))
        ins = snaps + [(L.quality_off, 8 * K)] + list(zip(L.forced_off, forced_sizes(nf, nfe))) + [(L.table_off, L.table_bytes)]
        outs = [16 * C, 8 * E1, 4 * E1, 56 * V, 24 * K, 8 * E2, 4 * E2, 4 * K, 16, 8 * K, 24 * K, 4 * K, 16, 16]
        arena = [(0, L.in_bytes), (L.out_dev_off, L.out_bytes), (L.rows_off[0], 4 * (K + 1)), (L.rows_off[1], 4 * E2), (L.rows_off[2], 4 * E2),
                 (L.ws_off, select_ws(K, nf, K)), (L.lp_scratch_off, lp_scratch(d[0], V, K)), (L.hyb_scratch_off, hyb_scratch(V, K))]
        assert L.table_bytes > 0 and list(L.entry_snap) == [L.snap_off[i] for i in (17, 18, 19, 20, 21, 8, 9, 13)]
        return [("in", L.in_bytes, ins), ("out", L.out_bytes, list(zip(L.out_off, outs))), ("arena", L.arena_bytes, arena)]
    if fid == 20:
        d = r.one(10)
        sizes = [16 * d[7], 8 * d[8], 4 * d[8], 8 * d[0], 8 * d[0], 16, lp_scratch(d[0], 0, 0)]
        return [("derived", L.bytes, list(zip(L.off, sizes)))]
    if fid == 21:
        d, (present, nf, nfe) = r.one(10), r.take(3)
        return round_regions(L, d, present, nf, nfe)
    if fid == 22:
        d, b, (present, nf, nfe) = r.one(10), r.one(8), r.take(3)
        after = after_append(d, b)
        blocks, _ = append_block(L, b)
        out = round_regions(L.round, after, present, nf, nfe, 16, "round.")
        out.append(("block", L.block_bytes, blocks))
        out.append(("arena", L.arena_bytes, [(0, L.block_bytes), (L.round_off, L.round.arena_bytes), (L.scratch_off, L.scratch_bytes)]))
        assert L.scratch_bytes >= lpa_scratch(d[1], b) and L.in_bytes == L.block_bytes + L.round.in_bytes
        assert L.out_bytes == L.round.out_bytes and L.flags_off + 16 <= L.out_bytes and L.flags_off >= L.round.out_off[5] + 4 * after[2]
        return out
    if fid == 23:
        d, m = r.one(10), r.one(8)
        bmask = r.take(1)[0]
        b, (present, nf, nfe) = r.take(8), r.take(3)
        b = None if bmask & 1 else b
        mid = after_remove(d, m)
        after = after_append(mid, b) if b else mid
        out = round_regions(L.round, after, present, nf, nfe, 32 if b else 16, "round.")
        arena = [(0, L.list_bytes), (L.round_off, L.round.arena_bytes), (L.scratch_off, L.scratch_bytes)]
        if b:
            blocks, _ = append_block(L, b)
            out.append(("upload front", L.list_bytes + L.block_bytes, [(0, 4 * m[0])] + blocks))
            arena += [(L.list_bytes, L.block_bytes), (L.append_scratch_off, lpa_scratch(mid[1], b))]
            assert L.append_flags_off + 16 <= L.flags_off
        assert L.list_bytes >= 4 * m[0] and L.scratch_bytes >= lpd_scratch(d[0], d[1], d[7]) and L.flags_off + 16 <= L.out_bytes
        assert L.in_bytes == L.list_bytes + (L.block_bytes if b else 0) + L.round.in_bytes and L.out_bytes == L.round.out_bytes
        out.append(("arena", L.arena_bytes, arena))
        return out
    if fid in (24, 25):
        width = 22 if fid == 24 else 31
        items, _, _, _ = r.many(width, forced=False)
        return rounds_regions(L, items, fid == 25)
    if fid == 28:
        mem, (mode, nm) = r.one(31), r.take(2)
        in_bytes, out_bytes, arena_bytes, after = solo_sizes(mem, True)
        K = after[2]
        row = al(4 * K)
        ws = 4 * workspace_floats(*state_dims(after))
        arena = [(0, arena_bytes), (L.out_base, out_bytes)] + [(L.out_base + L.member_off + i * L.member_stride, 4 * K) for i in range(nm)]
        arena += [(L.ws_off[i], ws) for i in range(nm)] + [(L.table_off, L.table_bytes)]
        assert L.in_bytes >= in_bytes and L.solo_out_bytes >= out_bytes and L.solo_arena_bytes >= arena_bytes and L.member_stride >= row
        assert L.out_bytes == L.member_off + nm * L.member_stride and L.table_bytes > 0 and L.n_models == nm
        return [("arena", L.arena_bytes, arena)]
    if fid == 29:
        items, nf, nfe, _ = r.many(3)
        mode = r.take(1)[0]
        if mode != 2:
            nf, nfe = [0] * len(items), [0] * len(items)
        n, K, E = len(items), sum(d[1] for d in items), sum(d[2] for d in items)
        ins = [(0, L.table_bytes)]
        for s, (V, k, e) in enumerate(items):
            ins += list(zip(L.snap_off[s], [4 * (k + 1), 4 * e, 8 * e, 8 * k, 8 * k, V, 8 * V, 8 * V]))
        ins += list(zip(L.forced_off, forced_sizes(sum(nf), sum(nfe))))
        outs = list(zip(L.out_off, [8 * K, 24 * K, 4 * K, 4 * n, 16 * n]))
        arena = [(0, L.in_bytes), (L.out_dev_off, L.out_bytes), (L.rows_off[0], 4 * (K + 1)), (L.rows_off[1], 4 * E), (L.rows_off[2], 4 * E),
                 (L.ws_off, select_ws(K, sum(nf), max(d[1] for d in items)) if mode == 2 else 0)]
        arena += [(L.scratch_off + L.scratch_base[s], hyb_scratch(V, k)) for s, (V, k, e) in enumerate(items)]
        assert L.table_bytes > 0 and (L.total_cuts, L.total_nnz, L.n_snapshots) == (K, E, n)
        return [("in", L.in_bytes, ins), ("out", L.out_bytes, outs), ("arena", L.arena_bytes, arena)]
    raise ValueError(fid)


def fits(regions):
    """None, or the first block that starts before its predecessor ends or ends past its region's total."""
    for name, total, blocks in regions:
        blocks = sorted(blocks, key=lambda b: (b[0], b[1]))
        for (o, s), nxt in zip(blocks, blocks[1:] + [(total, 0)]):
            if o < 0 or s < 0 or o + s > nxt[0]:
                return name, (o, s), nxt[0], total
    return None
