"""Ensembles over many states (GPU): `ModelSet.score_ensemble_many` / `select_cuts_ensemble_many` and their LP forms through
gcnn_infer_ensemble_batch / gcnn_lp_ensemble_batch, and the one kernel of their own, k_eb_mean_rank.

Definition under test, for the keys k_0..k_{M-1} and the states s_0..s_{S-1} ONE call admits: `members[m]` of state i has the bits of
`models[k_m].score_states([s_0..])[i]` -- the same union in the same order -- (LP: `score_lps`, with `state_from_lp`'s state and
cut_index); the mean is the float32 loop of k_ens_mean over those rows; the rankings are Python's stable descending sort of the mean
(NaN as -inf); the selection is `ops.select_cuts` over the collated union's mean with the union's cut offsets and forced rows.  All
of these are `np.array_equal`.  A state's bits in two DIFFERENT unions are never compared: there the fp64 oracle on the state alone
holds at the project's 1e-4 (each member is within 1e-4 of its oracle, so the mean is within 1e-4 of the oracles' mean).

Kernel seams: the segments of one union have exactly 1, 2, 3, 255, 256, 257, 1,025 and 4,096 cuts -- below, at and above one
trip of the 256 threads, a power of two and one past it for the network's padding, and RK_MAX.  Their scores come from probe
models whose every weight is 0 or 1 but for two gains: the score of a cut is a function of its first three features alone,
so NaN, +-inf and exact ties can be planted per cut, also in the last cut of one state and the first of the next."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate, ops, synthetic  # noqa: E402
from gcnn_cut_selector_amd.infer import normalize_forced  # noqa: E402
from gcnn_cut_selector_amd.model import GCNN, ModelSet  # noqa: E402
from oracle import gcnn_oracle as O  # noqa: E402  (checker only)

from gpucommon import dev, general_batch, make_model, make_state, oracle_scores  # noqa: E402,F401
from test_gpu_ensemble import mean_loop, same  # noqa: E402
from test_gpu_ibatch import _bad_states, _forced_like_cuts, _mixed  # noqa: E402
from test_gpu_lpbatch import _forced_for  # noqa: E402

N_MODELS = 9                      # eight for the largest ensemble and one more for the refusal of nine keys
KEYS = [f"seed/{i}" for i in range(N_MODELS)]
SCORES, RANK, SELECT = _lib.IBATCH_SCORES, _lib.IBATCH_RANK, _lib.IBATCH_SELECT
THRESHOLDS = ((0.1, 0.5), (0.9, 0.95))
# the full S x M grid where the union is small, M = 5 on every S
CASES = [(S, M) for S in (1, 2, 3) for M in (1, 2, 5, 8)] + [(8, 1), (8, 5), (8, 8), (17, 5), (64, 5)]
LP_CASES = [(1, 5), (3, 1), (3, 2), (3, 5), (3, 8), (8, 5)]
LP_CUTS = (1, 64, 65, 257, 5, 12, 33, 40)
f32, i32 = np.float32, np.int32


@pytest.fixture(scope="module")
def farm(dev):  # noqa: F811
    made = [make_model(800 + i, dev) for i in range(N_MODELS)]
    models = {k: m for k, (m, _) in zip(KEYS, made)}
    return dict(models=models, params={k: p for k, (_, p) in zip(KEYS, made)}, mset=ModelSet(models), all=_mixed(64, first=64),
                members={}, oracle={}, snaps={}, alone={}, lp_members={}, lp_oracle={})


class _NoSolo:
    """Forbids (or, with `allow`, records) the single-state ensemble methods for the length of a block."""
    NAMES = ("score_ensemble", "select_cuts_ensemble", "score_lp_ensemble", "select_cuts_lp_ensemble")

    def __init__(self, mset, allow=False):
        self.mset, self.allow, self.seen = mset, allow, []

    def __enter__(self):
        for name in self.NAMES:
            plain = getattr(self.mset, name)

            def wrapped(keys, state, *a, _name=name, _plain=plain, **k):
                if not self.allow:
                    raise AssertionError(f"a state of a clean call fell back to {_name}")
                self.seen.append((_name, state))
                return _plain(keys, state, *a, **k)
            setattr(self.mset, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name in self.NAMES:
            delattr(self.mset, name)
        return False


def _members(farm, S, M):
    """[m][i]: `models[k_m].score_states(states[:S])[i]`, computed once per (S, m) and never written to."""
    for m in range(M):
        if (S, m) not in farm["members"]:
            farm["members"][S, m] = [np.asarray(r).copy() for r in farm["models"][KEYS[m]].score_states(farm["all"][:S])]
    return [farm["members"][S, m] for m in range(M)]


def _oracle_mean(farm, i, M, state=None, cache="oracle"):
    """The fp64 oracles' mean for state i alone (each member's oracle computed once)."""
    state = farm["all"][i] if state is None else state
    for m in range(M):
        if (i, m) not in farm[cache]:
            farm[cache][i, m] = oracle_scores(farm["params"][KEYS[m]], state)
    return np.mean([farm[cache][i, m] for m in range(M)], axis=0)


def _ranking(mean):
    key = np.where(np.isnan(mean), -np.inf, mean).tolist()
    return sorted(range(len(key)), key=key.__getitem__, reverse=True)


def _union_upload(inputs, forced, mode):
    """in_bytes of gcnn_infer_batch's upload of these states (+ forced rows in selection mode): what one call may upload."""
    n = len(inputs)
    dims = (_lib.Dims * n)(*(_lib.Dims(s[7], s[8], s[9], s[1].shape[1], s[5].shape[1]) for s in inputs))
    nf = nfe = None
    if forced is not None:
        packed = [normalize_forced(f, s[8]) for f, s in zip(forced, inputs)]
        nf, nfe = (C.c_int32 * n)(*(p[0].size - 1 for p in packed)), (C.c_int32 * n)(*(p[1].size for p in packed))
    L = _lib.IbatchLayout()
    assert _lib.lib().gcnn_infer_batch_layout_for(n, dims, nf, nfe, mode, C.byref(L)) == 0
    return int(L.in_bytes)


def _union_forced(inputs, forced, dev):  # noqa: F811
    """The states' forced rows stacked in the union's column space as device CSR, and the states' offsets over the rows."""
    ptrs, cols, vals, f_off, e, v = [], [], [], [0], 0, 0
    for inp, f in zip(inputs, forced):
        ptr, col, val = normalize_forced(f, inp[8])
        ptrs.append(ptr[:-1].astype(np.int64) + e)
        cols.append(col.astype(np.int64) + v)
        vals.append(val)
        e, v = e + col.size, v + inp[8]
        f_off.append(f_off[-1] + ptr.size - 1)
    csr = (np.concatenate(ptrs + [[e]]).astype(i32), np.concatenate(cols).astype(i32), np.concatenate(vals).astype(f32))
    return tuple(torch.from_numpy(a).to(dev) for a in csr), torch.from_numpy(np.array(f_off, i32)).to(dev)


def _select_reference(model, inputs, means, forced, p_max, p_max_ub):
    """`ops.select_cuts` over the collated union's mean with the union's cut offsets and forced rows: (order, n_kept) per state."""
    batch, k_off = general_batch(model, inputs)
    csr, f_off = _union_forced(inputs, forced, model.device)
    quality = torch.from_numpy(np.ascontiguousarray(np.concatenate(means))).to(model.device)
    order, kept = ops.select_cuts(quality, batch.cut_graph, torch.from_numpy(k_off).to(model.device), csr, f_off, p_max=p_max,
                                  p_max_ub=p_max_ub, max_cuts=max(inp[9] for inp in inputs))
    order, kept = order.cpu().numpy(), kept.cpu().numpy()
    return [(order[k_off[s]:k_off[s + 1]], int(kept[s])) for s in range(len(inputs))]


def _restated(inp, mean, forced, p_max, p_max_ub):
    """cutsel_restate's selection on the state's own mean; the case must lie inside the restatement's margins."""
    K, V = inp[9], inp[8]
    fi, fv, F = forced
    rec = {}
    order, n = R.select(mean, R.dense_rows(inp[5][0], inp[5][1], inp[6].reshape(-1), K, V), R.dense_rows(fi[0], fi[1], fv, F, V), p_max,
                        p_max_ub, record=rec)
    assert R.margins_ok(rec, p_max, p_max_ub), "the case sits on a margin of the restatement: choose another seed"
    return order, n


def _check_scored(got, inputs, ref, S, M):
    """Members, mean and rankings of one rank-mode call against their definitions; returns the means."""
    means = []
    for i, (q, inp) in enumerate(zip(got, inputs)):
        K = inp[9]
        assert q.dtype == f32 and q.shape == (K,) and q.members.dtype == f32 and q.members.shape == (M, K), (S, M, i)
        for m in range(M):
            assert same(q.members[m], ref[m][i]), (S, M, i, m)
        want = mean_loop([ref[m][i] for m in range(M)])
        assert same(np.asarray(q), want), (S, M, i)
        assert q.rankings.dtype == i32 and q.rankings.tolist() == _ranking(want), (S, M, i)
        means.append(want)
    return means


# ---- whole calls on host states ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,M", CASES)
def test_members_mean_rankings_selection_and_fp64(farm, S, M):
    mset, keys, inputs = farm["mset"], KEYS[:M], farm["all"][:S]
    first = farm["models"][keys[0]]
    ref = _members(farm, S, M)
    sess = mset.ensemble_batch_session()
    rng = np.random.default_rng(100 * S + M)
    forced = [_forced_like_cuts(rng, inp, min(3, inp[9])) for inp in inputs]
    with _NoSolo(mset):
        calls, up = sess.calls, sess.upload_bytes
        got = mset.score_ensemble_many(keys, inputs, rank=True)
        assert sess.calls == calls + 1, "exactly one C call"
        assert sess.upload_bytes - up == _union_upload(inputs, None, RANK), "the states go up once, whatever M is"
        assert sess.max_states_per_call >= S
        means = _check_scored(got, inputs, ref, S, M)
        plain = mset.score_ensemble_many(keys, inputs)
        assert sess.calls == calls + 2 and all(same(np.asarray(a), b) and a.rankings is None for a, b in zip(plain, means))
        for p_max, p_max_ub in THRESHOLDS:
            calls, up = sess.calls, sess.upload_bytes
            sel = mset.select_cuts_ensemble_many(keys, inputs, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=5)
            assert sess.calls == calls + 1 and sess.upload_bytes - up == _union_upload(inputs, forced, SELECT)
            want = _select_reference(first, inputs, means, forced, p_max, p_max_ub)
            for i, (res, inp, (order, n_kept)) in enumerate(zip(sel, inputs, want)):
                assert same(np.asarray(res.scores), means[i]) and all(same(res.members[m], ref[m][i]) for m in range(M)), (S, M, i)
                assert np.array_equal(res.order, order) and res.n_kept == n_kept and res.n_selected == min(n_kept, 5), (S, M, i)
                order, n = _restated(inp, means[i], forced[i], p_max, p_max_ub)
                assert np.array_equal(res.order, order) and res.n_kept == n, (S, M, i)
    # against fp64, every state alone
    for i, q in enumerate(got):
        np.testing.assert_allclose(np.asarray(q), _oracle_mean(farm, i, M), rtol=1e-4, atol=1e-4)


def test_launch_lists(farm):
    mset, inputs = farm["mset"], farm["all"][:5]
    forced = [None] * 5
    counts = {}
    for M in (1, 8):
        keys = KEYS[:M]
        for mode, call in ((RANK, lambda: mset.score_ensemble_many(keys, inputs, rank=True)),
                           (SCORES, lambda: mset.score_ensemble_many(keys, inputs)),
                           (SELECT, lambda: mset.select_cuts_ensemble_many(keys, inputs, forced))):
            call()                                                         # buffers and layouts exist
            with _NoSolo(mset), _lib.launch_profile() as prof:
                call()
            names = [n for n, _ in prof.launches]
            # the index pass and the by-variable stage of the union, each once, in front of everything
            assert names[:2] == ["k_ens_unpack", "k_ens_by_variable"] and names.count("k_ens_unpack") == 1, names
            assert names.count("k_ens_by_variable") == 1 and not [n for n in names if n.startswith("k_ib_") or n.startswith("k_infer_s")]
            if mode == RANK:       # the fused tail, once, in place of the mean and the ranking
                assert names.count("k_eb_mean_rank") == 1 and names[-1] == "k_eb_mean_rank", names
                assert "k_ens_mean" not in names and "k_ib_rank" not in names and "k_ens_rank" not in names, names
            else:
                assert names.count("k_ens_mean") == 1 and "k_eb_mean_rank" not in names and "k_ens_rank" not in names, names
                assert ({"k_sel_pairs", "k_sel_filter"} <= set(names)) == (mode == SELECT), names
            counts[M, mode] = len(names)
    # the M forward passes are one group: the chain is as long for eight members as for one
    for mode in (RANK, SCORES, SELECT):
        assert counts[1, mode] == counts[8, mode], counts
    assert counts[8, RANK] == counts[8, SCORES], counts


def test_one_state_equals_the_single_state_call_in_every_field(farm):
    mset, keys = farm["mset"], KEYS[:5]
    rng = np.random.default_rng(3)
    for i in (0, 2, 6, 8):
        state = farm["all"][i]
        forced = _forced_like_cuts(rng, state, min(3, state[9]))
        with _NoSolo(mset):
            many = mset.score_ensemble_many(keys, [state], rank=True)[0]
            many_sel = mset.select_cuts_ensemble_many(keys, [state], [forced], p_max=0.2, p_max_ub=0.6, max_selected=4)[0]
        one = mset.score_ensemble(keys, state, rank="device")
        one_sel = mset.select_cuts_ensemble(keys, state, forced, p_max=0.2, p_max_ub=0.6, max_selected=4)
        assert same(np.asarray(many), np.asarray(one)) and same(many.members, one.members) and many.cut_index is None is one.cut_index
        assert same(many.rankings, one.rankings)
        assert same(np.asarray(many_sel.scores), np.asarray(one_sel.scores)) and same(many_sel.members, one_sel.members)
        assert same(many_sel.order, one_sel.order) and (many_sel.n_kept, many_sel.n_selected) == (one_sel.n_kept, one_sel.n_selected)
        assert many_sel.cut_index is None is one_sel.cut_index


# ---- the seams of k_eb_mean_rank ---------------------------------------------------------------------------------------------------------
SEAM_CUTS = (1, 2, 3, 255, 256, 257, 1025, 4096)
GAIN = 100                        # the probe's last layer multiplies by 2^(GAIN + m); the features carry 2^-GAIN
TIE = 0.5


def _probe_weights(m):
    """A model whose score is a function of the cut's first three features alone.  Every weight is 0 but these: the units
    relu(x0), relu(-x0), relu(x1), relu(x2) pass unchanged through the cut embedding and the cut convolution's output module; out_1
    keeps the first three and multiplies the fourth by 2^GAIN; the readout is g * (relu(x0) - relu(-x0)) + sign * g * relu(x1) with
    g = 2^(GAIN + m) and sign = +1 for an even m, -1 for an odd one, and gives the fourth unit the weight 0.  So x0 = +-2^GAIN
    overflows to +-inf in every member, x1 = 2^GAIN to +inf in the even and -inf in the odd members (a NaN mean from two members
    on, formed by the kernel under test), and x2 = 2^GAIN to inf * 0 = NaN inside every member."""
    p = {n: np.zeros(s, f32) for n, s, _ in O.PARAM_SPEC}
    for n in p:
        if n.endswith("prenorm/scale"):
            p[n][:] = 1.0
    e1 = p["cut_emb_1/kernel"]
    e1[0, 0], e1[0, 1], e1[1, 2], e1[2, 3] = 1.0, -1.0, 1.0, 1.0
    for name, off in (("cut_emb_2/kernel", 0), ("cut_conv_out_1/kernel", O.EMB), ("cut_conv_out_2/kernel", 0), ("out_1/kernel", 0)):
        for u in range(4):
            p[name][off + u, u] = 1.0
    p["out_1/kernel"][3, 3] = f32(2.0 ** GAIN)
    g = f32(2.0 ** (GAIN + m))
    p["out_2/kernel"][:4, 0] = (g, -g, g if m % 2 == 0 else -g, 0.0)
    return [p[n] for n in O.PARAM_NAMES]


@pytest.fixture(scope="module")
def seams(dev):  # noqa: F811
    models = {}
    for m in range(8):
        models[f"probe/{m}"] = GCNN(device=dev)
        models[f"probe/{m}"].set_weights(_probe_weights(m))
    rng = np.random.default_rng(17)
    big, small = f32(2.0 ** GAIN), f32(2.0 ** -GAIN)
    states, planted = [], []
    for s, K in enumerate(SEAM_CUTS):
        state = list(make_state(6, 9, K, 40 + s)[0])
        z = rng.standard_normal(K).astype(f32)
        z[0] = z[-1] = TIE                       # a segment's first and last cut tie, and so do the two sides of every state boundary
        k = np.zeros((K, 6), f32)
        k[:, 0] = z * small
        spots = dict(nan=[], pinf=[], ninf=[], mixed=[])
        if K == 3:
            spots["nan"] = [1]
        if K >= 255:
            z[10:20] = z[30:40]                  # ties inside the segment
            k[:, 0] = z * small
            spots = dict(nan=[5, K - 2], pinf=[7, K - 3], ninf=[9, 128], mixed=[60])
        for j in spots["pinf"]:
            k[j, 0] = big
        for j in spots["ninf"]:
            k[j, 0] = -big
        for j in spots["nan"]:
            k[j, 2] = big                        # inf * 0 in the readout of every member
        for j in spots["mixed"]:
            k[j, 0], k[j, 1] = 0.0, big          # +inf in the even members, -inf in the odd ones
        state[4] = k
        states.append(tuple(state))
        planted.append(spots)
    keys = list(models)
    ref = [[np.asarray(r).copy() for r in models[k].score_states(states)] for k in keys]
    return dict(mset=ModelSet(models), keys=keys, states=states, planted=planted, ref=ref)


@pytest.mark.parametrize("M", [1, 2, 5, 8])
def test_kernel_seams(seams, M):
    mset, keys, states, ref = seams["mset"], seams["keys"][:M], seams["states"], seams["ref"]
    sess = mset.ensemble_batch_session()
    with _NoSolo(mset):
        # a call of other sizes through the same buffers first: what it left lies around, and inside, this call's segments
        mset.score_ensemble_many(keys, states[::-1][2:], rank=True)
        calls = sess.calls
        got = mset.score_ensemble_many(keys, states, rank=True)
        assert sess.calls == calls + 1
    # every segment of the union against the references' rows: a write outside a state's segment would land in a neighbour's
    means = _check_scored(got, states, ref, len(states), M)
    # what was planted is there: the test covers NaN, both infinities and exact ties, also across the state boundaries
    for s, (mean, spots) in enumerate(zip(means, seams["planted"])):
        K = mean.size
        nan, pinf = spots["nan"] + (spots["mixed"] if M > 1 else []), spots["pinf"] + (spots["mixed"] if M == 1 else [])
        assert np.isnan(mean[nan]).all() and (mean[pinf] == np.inf).all() and (mean[spots["ninf"]] == -np.inf).all(), (s, mean[nan], mean[pinf])
        assert mean[0] == mean[-1] == means[(s + 1) % len(means)][0] and np.isfinite(mean[0]), s
        order = got[s].rankings.tolist()
        if K >= 255:
            assert np.array_equal(mean[10:20], mean[30:40]) and order[:len(pinf)] == sorted(pinf)
            assert order[-len(nan) - 2:] == sorted(nan + spots["ninf"]), "NaN ranks as -inf, ties in index order"
        if K > 1:
            assert order.index(0) + 1 == order.index(K - 1), s         # the tie of the first and the last cut: index order
    with _NoSolo(mset):
        again = mset.score_ensemble_many(keys, states, rank=True)
    for a, b in zip(again, got):
        assert same(np.asarray(a), np.asarray(b)) and same(a.rankings, b.rankings) and same(a.members, b.members)


# ---- the LP forms ------------------------------------------------------------------------------------------------------------------------
def _snaps(farm, S):
    for i in range(S):
        if i not in farm["snaps"]:
            farm["snaps"][i] = synthetic.make_lp_snapshot(("setcov", "capfac")[i % 2], 500 + i, scale=0.2, incumbent=i % 2 == 1,
                                                          n_cuts=LP_CUTS[i])
            farm["alone"][i] = farm["models"][KEYS[0]].state_from_lp(farm["snaps"][i])
    return [farm["snaps"][i] for i in range(S)], [farm["alone"][i] for i in range(S)]


def _lp_members(farm, S, M):
    snaps, _ = _snaps(farm, S)
    for m in range(M):
        if (S, m) not in farm["lp_members"]:
            farm["lp_members"][S, m] = [np.asarray(r).copy() for r in farm["models"][KEYS[m]].score_lps(snaps)]
    return [farm["lp_members"][S, m] for m in range(M)]


@pytest.mark.parametrize("S,M", LP_CASES)
def test_lp_members_mean_cut_index_selection_and_fp64(farm, S, M):
    mset, keys = farm["mset"], KEYS[:M]
    first = farm["models"][keys[0]]
    snaps, alone = _snaps(farm, S)
    states = [a[0] for a in alone]
    ref = _lp_members(farm, S, M)
    sess = mset.ensemble_batch_session(lp=True)
    forced = [_forced_for(st, 10 * S + i) for i, st in enumerate(states)]
    with _NoSolo(mset):
        calls, up = sess.calls, sess.upload_bytes
        got = mset.score_lp_ensemble_many(keys, snaps, rank=True)
        assert sess.calls == calls + 1
        one_upload = sess.upload_bytes - up
        means = _check_scored(got, states, ref, S, M)
        for q, (_, index) in zip(got, alone):
            assert np.array_equal(q.cut_index, index)
        for p_max, p_max_ub in THRESHOLDS:
            calls = sess.calls
            sel = mset.select_cuts_lp_ensemble_many(keys, snaps, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=4)
            assert sess.calls == calls + 1
            want = _select_reference(first, states, means, forced, p_max, p_max_ub)
            for i, (res, st, (order, n_kept)) in enumerate(zip(sel, states, want)):
                assert same(np.asarray(res.scores), means[i]) and all(same(res.members[m], ref[m][i]) for m in range(M)), (S, M, i)
                assert np.array_equal(res.cut_index, alone[i][1]), (S, M, i)
                assert np.array_equal(res.order, order) and res.n_kept == n_kept and res.n_selected == min(n_kept, 4), (S, M, i)
                order, n = _restated(st, means[i], forced[i], p_max, p_max_ub)
                assert np.array_equal(res.order, order) and res.n_kept == n, (S, M, i)
    # the upload does not depend on M
    other = KEYS[:1] if M > 1 else KEYS[:8]
    up = sess.upload_bytes
    mset.score_lp_ensemble_many(other, snaps, rank=True)
    assert sess.upload_bytes - up == one_upload
    for i, (q, st) in enumerate(zip(got, states)):
        np.testing.assert_allclose(np.asarray(q), _oracle_mean(farm, i, M, st, "lp_oracle"), rtol=1e-4, atol=1e-4)


def test_lp_one_snapshot_equals_the_single_call_in_every_field(farm):
    mset, keys = farm["mset"], KEYS[:5]
    snaps, alone = _snaps(farm, 4)
    for snap, (state, _) in zip(snaps, alone):
        forced = _forced_for(state, 5)
        with _NoSolo(mset):
            many = mset.score_lp_ensemble_many(keys, [snap], rank=True)[0]
            many_sel = mset.select_cuts_lp_ensemble_many(keys, [snap], [forced], p_max=0.2, p_max_ub=0.6, max_selected=4)[0]
        one = mset.score_lp_ensemble(keys, snap, rank="device")
        one_sel = mset.select_cuts_lp_ensemble(keys, snap, forced, p_max=0.2, p_max_ub=0.6, max_selected=4)
        assert same(np.asarray(many), np.asarray(one)) and same(many.members, one.members) and same(many.cut_index, one.cut_index)
        assert same(many.rankings, one.rankings)
        assert same(np.asarray(many_sel.scores), np.asarray(one_sel.scores)) and same(many_sel.members, one_sel.members)
        assert same(many_sel.order, one_sel.order) and (many_sel.n_kept, many_sel.n_selected) == (one_sel.n_kept, one_sel.n_selected)
        assert same(many_sel.cut_index, one_sel.cut_index)


def test_a_flagged_snapshot_gets_its_own_error_and_its_neighbours_are_unchanged(farm, monkeypatch):
    """The upload of the middle snapshot is corrupted behind the host check (a column far out of range): the device sets its LP
    flag, its slot holds the ValueError, and its neighbours have the bits of a clean run of the same union."""
    mset, keys = farm["mset"], KEYS[:5]
    snaps, _ = _snaps(farm, 3)
    clean = mset.score_lp_ensemble_many(keys, snaps, rank=True)
    clean_sel = mset.select_cuts_lp_ensemble_many(keys, snaps, max_selected=4)
    index = [n for n, _ in lpstate.FIELDS].index("cut_col") + 1
    pack, calls = lpstate.pack_snapshot, []

    def wrapper(buf, snap_off, arrays):
        pack(buf, snap_off, arrays)
        calls.append(1)
        if len(calls) % 3 == 2:
            buf[snap_off[index]:].view(np.int32)[0] = 10 ** 6
    with monkeypatch.context() as mp, _NoSolo(mset):
        mp.setattr(lpstate, "pack_snapshot", wrapper)
        got = mset.score_lp_ensemble_many(keys, snaps, rank=True, return_exceptions=True)
        sel = mset.select_cuts_lp_ensemble_many(keys, snaps, max_selected=4, return_exceptions=True)
        with pytest.raises(ValueError, match="outside"):
            mset.score_lp_ensemble_many(keys, snaps)
    assert len(calls) == 9
    for res in (got, sel):
        assert isinstance(res[1], ValueError) and "outside" in str(res[1])
    for at in (0, 2):
        assert same(np.asarray(got[at]), np.asarray(clean[at])) and same(got[at].rankings, clean[at].rankings)
        assert same(got[at].members, clean[at].members) and same(got[at].cut_index, clean[at].cut_index)
        assert same(sel[at].order, clean_sel[at].order) and sel[at].n_kept == clean_sel[at].n_kept


def test_a_snapshot_of_32769_columns_is_admitted(farm):
    mset, keys = farm["mset"], KEYS[:3]
    snaps, _ = _snaps(farm, 2)
    narrow = int(np.asarray(synthetic.make_lp_snapshot("indset", 3, scale=0.3).col_type).shape[0])
    wide = synthetic.make_lp_snapshot("indset", 3, scale=0.3, extra_cols=32769 - narrow)
    assert int(np.asarray(wide.col_type).shape[0]) == 32769
    trio = [snaps[0], wide, snaps[1]]
    sess = mset.ensemble_batch_session(lp=True)
    calls = sess.calls
    with _NoSolo(mset):
        got = mset.score_lp_ensemble_many(keys, trio, rank=True)
        sel = mset.select_cuts_lp_ensemble_many(keys, trio)
    assert sess.calls == calls + 2
    state, index = farm["models"][keys[0]].state_from_lp(wide)
    assert state[8] == 32769 and np.array_equal(got[1].cut_index, index)
    ref = [[np.asarray(r) for r in farm["models"][k].score_lps(trio)] for k in keys]
    for i, q in enumerate(got):
        want = mean_loop([ref[m][i] for m in range(3)])
        assert all(same(q.members[m], ref[m][i]) for m in range(3)) and same(np.asarray(q), want) and q.rankings.tolist() == _ranking(want)
        assert same(np.asarray(sel[i].scores), want)


# ---- isolation, fallbacks, refusals ------------------------------------------------------------------------------------------------------
def test_isolation_and_fallbacks(farm, dev):  # noqa: F811
    mset, keys = farm["mset"], KEYS[:5]
    rng = np.random.default_rng(7)
    bad_index, unsorted, huge, _ = _bad_states(rng)
    clean = farm["all"][:3]
    empty = clean[1][:4] + (np.zeros((0, 6), f32), np.zeros((2, 0), i32), np.zeros((0, 1), f32)) + clean[1][7:9] + (0,)
    tensors = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in clean[0][:7]) + tuple(clean[0][7:])
    inputs = [clean[0], bad_index, clean[1], unsorted, huge, clean[2], empty, tensors]
    in_union = [0, 1, 2, 3, 5]                  # the out-of-range state stays in the union, confined to its own ranges
    solo_ids = [4, 6, 7]
    sess = mset.ensemble_batch_session()
    with _NoSolo(mset, allow=True) as spy:
        calls = sess.calls
        scored = mset.score_ensemble_many(keys, inputs, rank=True, return_exceptions=True)
        assert sess.calls == calls + 1
        assert [(n, s is inputs[i]) for (n, s), i in zip(spy.seen, solo_ids)] == [("score_ensemble", True)] * 3 and len(spy.seen) == 3
        selected = mset.select_cuts_ensemble_many(keys, inputs, return_exceptions=True)
        assert [n for n, _ in spy.seen[3:]] == ["select_cuts_ensemble"] * 3
    # each gets what `GCNN.score_states` documents for it
    assert isinstance(scored[1], ValueError) and "out of range" in str(scored[1]) and isinstance(selected[1], ValueError)
    assert isinstance(selected[4], _lib.GcnnError) and "4097" in str(selected[4])
    alone = mset.score_ensemble(keys, huge, rank=True)
    assert same(np.asarray(scored[4]), np.asarray(alone)) and same(scored[4].rankings, alone.rankings) and same(scored[4].members, alone.members)
    assert scored[6].shape == (0,) and scored[6].members.shape == (5, 0) and scored[6].rankings.shape == (0,)
    assert selected[6].n_kept == 0 and selected[6].order.shape == (0,)
    general = mset.score_ensemble(keys, tensors, rank=True)
    assert same(np.asarray(scored[7]), np.asarray(general)) and same(scored[7].members, general.members)
    np.testing.assert_allclose(np.asarray(scored[7]), _oracle_mean(farm, 0, 5), rtol=1e-4, atol=1e-4)
    # the others: the same union as the call without the solo states' slots
    same_union = [inputs[i] for i in in_union]
    with _NoSolo(mset):
        want = mset.score_ensemble_many(keys, same_union, rank=True, return_exceptions=True)
        want_sel = mset.select_cuts_ensemble_many(keys, same_union, return_exceptions=True)
    for j, i in enumerate(in_union):
        if i == 1:
            assert isinstance(want[j], ValueError)
            continue
        assert same(np.asarray(scored[i]), np.asarray(want[j])) and same(scored[i].members, want[j].members), i
        assert same(scored[i].rankings, want[j].rankings) and same(selected[i].order, want_sel[j].order), i
        assert selected[i].n_kept == want_sel[j].n_kept and same(np.asarray(selected[i].scores), np.asarray(scored[i])), i
    for i, at in ((0, 0), (2, 1), (5, 2)):       # (inputs[i] is the farm's state `at`)
        np.testing.assert_allclose(np.asarray(scored[i]), _oracle_mean(farm, at, 5), rtol=1e-4, atol=1e-4)
    # without return_exceptions the first error is raised, after every state was served
    calls = sess.calls
    with pytest.raises(ValueError, match="out of range"):
        mset.score_ensemble_many(keys, inputs[:3])
    assert sess.calls == calls + 1


def test_refusals_empty_lists_and_more_than_64_states(farm):
    mset = farm["mset"]
    state = farm["all"][0]
    snaps, _ = _snaps(farm, 1)
    sessions = (mset.ensemble_batch_session(), mset.ensemble_batch_session(lp=True))
    calls = [s.calls for s in sessions]
    methods = ((mset.score_ensemble_many, [state]), (mset.select_cuts_ensemble_many, [state]), (mset.score_lp_ensemble_many, snaps),
               (mset.select_cuts_lp_ensemble_many, snaps))
    for keys in ([], KEYS[:9], [KEYS[0], KEYS[1], KEYS[0]], [KEYS[0], "nobody"]):
        for call, arg in methods:
            with pytest.raises(ValueError):
                call(keys, arg)
            with pytest.raises(ValueError):
                call(keys, [])                   # before any other work, also for an empty list
    with pytest.raises(ValueError):
        mset.select_cuts_ensemble_many(KEYS[:2], [state], p_max=float("nan"))
    with pytest.raises(ValueError):
        mset.select_cuts_ensemble_many(KEYS[:2], [state, state], [None])
    for call, _ in methods:
        assert call(KEYS[:3], []) == []
    assert [s.calls for s in sessions] == calls
    # 65 states: ceil(65 / 64) calls; the first 64 ride in the union they ride in alone
    keys, inputs = KEYS[:2], farm["all"] + [farm["all"][0]]
    sess = sessions[0]
    with _NoSolo(mset):
        calls = sess.calls
        got = mset.score_ensemble_many(keys, inputs, rank=True)
        assert sess.calls == calls + 2 and sess.max_states_per_call == 64
        first = mset.score_ensemble_many(keys, inputs[:64], rank=True)
        last = mset.score_ensemble_many(keys, inputs[64:], rank=True)
    for a, b in zip(got, first + last):
        assert same(np.asarray(a), np.asarray(b)) and same(a.members, b.members) and same(a.rankings, b.rankings)
