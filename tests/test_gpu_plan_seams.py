"""The graph plans of gcnn_infer and gcnn_infer_batch, entry by entry, at every seam of their launches (GPU).

Cases, restatement and their proof are in tests/plancases.py and tests/test_plancases.py.  Per case: a throw-away call of the same
sizes and other contents makes the session's arena hold another state's plan, the arena is filled with a byte pattern, the product
call runs (`score_state`, `select_cuts`, `score_states`, `select_cuts_many`), and the plan is read out of the arena at the layout's offsets
(`last_plan` of the sessions).  Every integer array must equal the restatement, the copied coefficients in bits, `v_pos` per segment
as a set, the flags; the launch record must name the form the case is about.  Scores are compared with the fp64 oracle at the
project's 1e-4 and, where the general path runs the same edge and row kernels, with `m(state, False)` bit for bit; rankings with
Python's stable sort.

Bits against the general path are not compared where a receiver set has more than 16,384 rows: there the edge passes are picked by
`edge_slots` and may run a long-segment pass, which the plan path (longest segment unknown) and a prepared batch (longest segment
known once its copy has landed) need not agree on.  That is every case with 16,385 constraints or 32,767 / 32,768 variables.

One process, the product library, no retry.  Measured on an MI355X: the module takes 9 s, every test under 0.6 s with its
restatement."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import plancases as P  # noqa: E402
from gcnn_cut_selector_amd import _lib, ops  # noqa: E402
from gcnn_cut_selector_amd.graph import BipartiteGraph  # noqa: E402
from gcnn_cut_selector_amd.infer import _BatchSession, _InferenceSession  # noqa: E402

from gpucommon import dev, general_batch, make_model, oracle_scores  # noqa: E402,F401

RTOL = ATOL = 1e-4
SINGLE_KEYS = ("l_ptr0", "l_ptr1", "inds0", "inds1", "vcount", "cursor", "flags", "v_ptr", "v_oth", "v_coef")
UNION_KEYS = ("flags", "l_ptr0", "l_ptr1", "left", "var0", "var1", "iota", "f_col", "v_ptr", "v_oth", "v_coef")
FORWARD = ("k_infer_s", "k_iplan_", "k_embed_fwd", "k_edge_fwd", "k_conv_fwd")
PLAIN = tuple(c for c in P.SINGLE_IDS if not c.startswith(("bad/", "twins/", "deg/2049")))


@pytest.fixture(scope="module")
def model(dev):
    return make_model(77, dev)


def _poison(sess):
    sess.arena.fill_(0xA5)
    torch.cuda.synchronize()


def _same(got, want, alt=None):
    """Exact, floats in bits; `alt`: entries several positions of a list out of order write -- any of their values."""
    got, want = (a.view(np.int32) if a.dtype == np.float32 else a for a in (got, want.reshape(got.shape)))
    if alt:
        free = np.array(sorted(alt), np.int64)
        if not all(int(got[k]) in alt[k] for k in free):
            return False
        got, want = got.copy(), want.copy()
        got[free] = want[free] = 0
    return np.array_equal(got, want)


def _check_plan(cid, got, want, keys):
    for k in keys:
        assert got[k].shape == want[k].reshape(got[k].shape).shape and _same(got[k], want[k], want["alt"].get(k)), \
            (cid, k, np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))[:8].tolist())
    if "v_pos" in got:                                # arrival order: the set of every segment
        seg = np.repeat(np.arange(want["v_ptr"].size - 1), np.diff(want["v_ptr"]))
        assert np.array_equal(got["v_pos"][np.lexsort((got["v_pos"], seg))], want["v_pos"][np.lexsort((want["v_pos"], seg))]), (cid, "v_pos")


def _forward_names(prof):
    return [n for n, _ in prof.launches if n.startswith(FORWARD)]


def _run_single(m, st, rank=True):
    """(scores or the exception, the plan in the arena, the forward's launch names) of `score_state` through a poisoned arena."""
    sess = m._sess("_session", _InferenceSession)
    m.score_state(P.other_contents(st))
    _poison(sess)
    with _lib.launch_profile() as prof:
        try:
            q = m.score_state(st, rank=rank)
        except ValueError as exc:
            q = exc
        torch.cuda.synchronize()
    return q, sess.last_plan(), _forward_names(prof)


def _general(m, st):
    with _lib.launch_profile() as prof, torch.no_grad():
        scores = m(st, False).numpy()
    return scores, _forward_names(prof)


def _as_general(names, st):
    """The plan path's launch names as the general path would name the same kernels: the fused launches carry the embedding, the
    conv v->c edge pass (a block per segment for few, long rows: launch_edge_fwd) and the conv v->c row program."""
    C, E1 = st[7], st[1].shape[1]
    out = []
    for n in names:
        if n.startswith("k_infer_s1"):
            out.append("embed")
        elif n.startswith("k_infer_s2"):
            out.append("k_edge_fwd_block" if C <= 1024 and E1 >= 48 * C else "k_edge_fwd")
        elif n.startswith("k_infer_s3"):
            out.append("k_conv_fwd<proj>")
        elif not n.startswith("k_iplan_"):
            out.append("embed" if n.startswith("k_embed_fwd") else n)
    return out


def _check_scores(cid, m, params, st, q, names):
    np.testing.assert_allclose(q.numpy(), oracle_scores(params, st), rtol=RTOL, atol=ATOL, err_msg=cid)
    general, gnames = _general(m, st)
    if max(st[7], st[8]) <= P.FUSE_MAX_ROWS:          # (the module's docstring: beyond, the long-segment pass is a matter of timing)
        assert _as_general(names, st) == _as_general(gnames, st), (cid, names, gnames)
        assert np.array_equal(q.numpy(), general), (cid, int((q.numpy() != general).sum()))
    if q.rankings is not None:
        assert list(q.rankings) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), cid


@pytest.mark.parametrize("cid", PLAIN)
def test_single_state_plan_is_the_restatement(model, cid):
    m, params = model
    st, want = P.single(cid), P.expected_case(cid)
    q, got, names = _run_single(m, st)
    assert not isinstance(q, Exception), (cid, q)
    assert [n for n in names if n.startswith(("k_infer_s", "k_iplan_"))] == want["launch"]["names"], (cid, names)
    _check_plan(cid, got, want, SINGLE_KEYS)
    _check_scores(cid, m, params, st, q, names)


def test_over_long_segment_is_zero_filled_and_answered_by_the_general_path(model):
    m, params = model
    st, want = P.single("deg/2049"), P.expected_case("deg/2049")
    q, got, names = _run_single(m, st)
    assert want["flags"].tolist() == [0, 0, 0, 1] and names[:3] == want["launch"]["names"]
    _check_plan("deg/2049", got, want, SINGLE_KEYS)                       # that segment zero-filled, every other one exact
    assert "k_embed_fwd_split" in names or "k_embed_fwd" in names         # the answer is the general path's
    np.testing.assert_allclose(q.numpy(), oracle_scores(params, st), rtol=RTOL, atol=ATOL)
    assert np.array_equal(q.numpy(), _general(m, st)[0])
    assert list(q.rankings) == sorted(range(len(q)), key=lambda x: q[x], reverse=True)


@pytest.mark.parametrize("K", (1, 2, 257, 1025, 4096))
def test_twins_tie_and_rank_in_index_order(model, K):
    m, params = model
    cid = f"twins/K{K}"
    st, want = P.single(cid), P.expected_case(cid)
    q, got, names = _run_single(m, st, rank="device")
    _check_plan(cid, got, want, SINGLE_KEYS)
    assert "k_rank_scores" in [n for n, _ in _profile(lambda: m.score_state(st, rank="device"))]
    for a, b in P.twin_pairs(cid):
        assert q[a] == q[b], (cid, a, b)
    stable = sorted(range(K), key=lambda x: q[x], reverse=True)
    assert list(q.rankings) == stable
    default = m.score_state(st, rank=True)
    assert np.array_equal(default.numpy(), q.numpy()) and list(default.rankings) == stable
    _check_scores(cid, m, params, st, q, names)


@pytest.mark.parametrize("cid", ("count/E1/256", "scan/256/V513", "scan/1024/V1025", "place/trip/alone/65537"))
def test_selecting_call_builds_the_same_plan(model, dev, cid):
    """gcnn_infer_select: the forced rows close the upload, so every block of the arena lies elsewhere; the plan is the same."""
    m, params = model
    st, want = P.single(cid), P.expected_case(cid)
    K, V = st[9], st[8]
    fi, fv, F = P.forced_rows(np.random.default_rng(5), st, 2)
    sess = m._sess("_session", _InferenceSession)
    m.select_cuts(P.other_contents(st), (fi, fv, F))
    _poison(sess)
    with _lib.launch_profile() as prof:
        res = m.select_cuts(st, (fi, fv, F))
        torch.cuda.synchronize()
    names = [n for n, _ in prof.launches]
    assert [n for n in names if n.startswith(("k_infer_s", "k_iplan_"))] == want["launch"]["names"] and "k_sel_filter" in names, names
    _check_plan(cid, sess.last_plan(), want, SINGLE_KEYS)
    np.testing.assert_allclose(res.scores.numpy(), oracle_scores(params, st), rtol=RTOL, atol=ATOL)
    graph = BipartiteGraph(torch.from_numpy(st[5]).to(dev), torch.from_numpy(st[6]).to(dev), K, V)
    packed = tuple(torch.from_numpy(a).to(dev) for a in ops.pack_rows(fi, fv, F, V))
    order, n_kept = ops.select_cuts(torch.from_numpy(np.asarray(res.scores)).to(dev), graph, None, packed, max_cuts=K)
    assert np.array_equal(res.order, order.cpu().numpy()) and res.n_kept == int(n_kept.cpu()[0])
    kept = res.order[:res.n_kept].tolist()
    assert kept == sorted(kept, key=lambda x: res.scores[x], reverse=True) and sorted(res.order.tolist()) == list(range(K))


def _profile(call):
    with _lib.launch_profile() as prof:
        call()
        torch.cuda.synchronize()
    return prof.launches


@pytest.mark.parametrize("cid", [c for c in P.SINGLE_IDS if c.startswith("bad/")])
def test_bad_id_is_flagged_sanitised_and_leaves_the_session_exact(model, cid):
    m, params = model
    st, want = P.single(cid), P.expected_case(cid)
    q, got, names = _run_single(m, st)
    assert isinstance(q, ValueError) and "out of range" in str(q), (cid, q)
    assert want["flags"][0] == 1 and names[:3] == want["launch"]["names"]
    _check_plan(cid, got, want, SINGLE_KEYS)
    for k, hi in (("l_ptr0", P.BAD_E1), ("l_ptr1", P.BAD_E2), ("v_ptr", P.BAD_E1), ("v_pos", P.BAD_E1 - 1), ("v_oth", P.BAD_C - 1)):
        assert got[k].min() >= 0 and got[k].max() <= hi, (cid, k)
    assert got["inds0"][P.BAD_E1:].min() >= 0 and got["inds0"][P.BAD_E1:].max() < P.BAD_V
    assert got["inds1"][P.BAD_E2:].min() >= 0 and got["inds1"][P.BAD_E2:].max() < P.BAD_V
    # the next call on the same session: the same sizes, every id in range
    clean = P.random_state(60, P.BAD_C, P.BAD_V, P.BAD_K, P.BAD_E1, P.BAD_E2)
    sess = m._session
    _poison(sess)
    q = m.score_state(clean, rank=True)
    _check_plan(cid + " (next call)", sess.last_plan(), P.expected_single(clean), SINGLE_KEYS)
    np.testing.assert_allclose(q.numpy(), oracle_scores(params, clean), rtol=RTOL, atol=ATOL)
    assert np.array_equal(q.numpy(), _general(m, clean)[0])


@pytest.mark.parametrize("name", sorted(P.DEGENERATE))
def test_edges_without_nodes_are_refused_before_anything_is_enqueued(model, name):
    m, _ = model
    st = P.degenerate(name)
    for call in (lambda: m.score_state(st), lambda: m.score_state(st, rank="device"), lambda: m.select_cuts(st)):
        with _lib.launch_profile() as prof:
            with pytest.raises(ValueError, match="out of range"):
                call()
            torch.cuda.synchronize()
        assert prof.launches == [], (name, prof.launches)
    good = P.single("count/E1/1")
    got = m.score_states([good, st, good], return_exceptions=True)             # the batched call hands it to the same refusal
    assert isinstance(got[1], ValueError) and got[0].shape == got[2].shape == (good[9],)


# ---- the union plan ----------------------------------------------------------------------------------------------------------------
def _run_union(m, states, call):
    sess = m._sess("_batch_session", _BatchSession)
    others = [P.other_contents(s, 98) for s in states]
    call(others)
    _poison(sess)
    calls = sess.calls
    with _lib.launch_profile() as prof:
        out = call(states)
        torch.cuda.synchronize()
    assert sess.calls == calls + 1                    # one gcnn_infer_batch, no state went to the solo path
    return out, sess.last_plan(), [n for n, _ in prof.launches]


def _check_union_form(names, e1):
    assert names[0] == "k_ib_unpack" and names.count("k_ib_unpack") == 1 and (names[1] == "k_ib_by_variable") == (e1 > 0), names
    assert not [n for n in names if n.startswith(("k_infer_s", "k_iplan_", "k_check_edges"))], names


@pytest.mark.parametrize("cid", [c for c in P.UNION_IDS if c not in ("ib/forced", "ib/bad")])
def test_union_plan_is_the_restatement(model, cid):
    m, params = model
    states, _ = P.union(cid)
    want = P.expected_case(cid)
    scored, got, names = _run_union(m, states, lambda s: m.score_states(s, rank=True))
    _check_union_form(names, want["left"].size)
    _check_plan(cid, got, want, UNION_KEYS)
    batch, k_off = general_batch(m, states)
    with torch.no_grad():
        general = m(batch, False).as_subclass(torch.Tensor).cpu().numpy()
    for s, (st, q) in enumerate(zip(states, scored)):
        assert np.array_equal(q.numpy(), general[k_off[s]:k_off[s + 1]]), (cid, s)
        np.testing.assert_allclose(q.numpy(), oracle_scores(params, st), rtol=RTOL, atol=ATOL, err_msg=f"{cid} state {s}")
        assert list(q.rankings) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (cid, s)


def test_union_forced_rows(model, dev):
    m, params = model
    states, forced = P.union("ib/forced")
    want = P.expected_case("ib/forced")
    selected, got, names = _run_union(m, states, lambda s: m.select_cuts_many(s, forced))
    _check_union_form(names, want["left"].size)
    _check_plan("ib/forced", got, want, UNION_KEYS)
    batch, k_off = general_batch(m, states)
    with torch.no_grad():
        general = m(batch, False).as_subclass(torch.Tensor).cpu().numpy()
    for s, (st, (fi, fv, F), res) in enumerate(zip(states, forced, selected)):
        K, V = st[9], st[8]
        assert np.array_equal(res.scores.numpy(), general[k_off[s]:k_off[s + 1]]), s
        np.testing.assert_allclose(res.scores.numpy(), oracle_scores(params, st), rtol=RTOL, atol=ATOL)
        graph = BipartiteGraph(torch.from_numpy(st[5]).to(dev), torch.from_numpy(st[6]).to(dev), K, V)
        packed = tuple(torch.from_numpy(a).to(dev) for a in ops.pack_rows(fi, fv, F, V))
        order, n_kept = ops.select_cuts(torch.from_numpy(np.asarray(res.scores)).to(dev), graph, None, packed, max_cuts=K)
        assert np.array_equal(res.order, order.cpu().numpy()) and res.n_kept == int(n_kept.cpu()[0]), s
        kept = res.order[:res.n_kept].tolist()
        assert kept == sorted(kept, key=lambda x: res.scores[x], reverse=True) and sorted(res.order.tolist()) == list(range(K)), s
    # a forced column out of range (the host check of `select_cuts_many` would refuse it: the session is called directly) becomes -1
    sess = m._batch_session
    packed = P.packed_forced(states, forced)
    for s, at, bad in ((0, 1, -4), (3, 8, states[3][8])):
        packed[s][1][at] = bad
    checked = [m._admit_state(st, _lib.IBATCH_SELECT) for st in states]
    _poison(sess)
    res = sess.run(checked, packed, _lib.IBATCH_SELECT, 0.1, 0.5)
    assert all(r[0] == "ok" for r in res)
    want = P.expected_union(states, packed)
    got = sess.last_plan()
    assert want["f_col"][1] == -1 and want["f_col"][6 + 8] == -1 and (want["f_col"] == -1).sum() == 2
    _check_plan("ib/forced (bad column)", got, want, UNION_KEYS)


def test_union_bad_state_leaves_its_neighbours_exact(model):
    m, params = model
    states, _ = P.union("ib/bad")
    want = P.expected_case("ib/bad")
    solo = [m.score_state(states[s], rank=True) for s in (0, 2)]
    sess = m._sess("_batch_session", _BatchSession)
    m.score_states([P.other_contents(s, 98) for s in states], rank=True)
    _poison(sess)
    with _lib.launch_profile() as prof:
        got = m.score_states(states, rank=True, return_exceptions=True)
        torch.cuda.synchronize()
    names = [n for n, _ in prof.launches]
    _check_union_form(names, want["left"].size)
    plan = sess.last_plan()
    assert want["flags"].tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]] and want["alt"]["l_ptr0"]
    _check_plan("ib/bad", plan, want, UNION_KEYS)
    assert isinstance(got[1], ValueError) and "out of range" in str(got[1])
    # the neighbours' structures are those of the union without the bad ids ...
    clean = P.expected_union(P.union_bad_clean())
    e = [s[1].shape[1] for s in states]
    for k in ("left", "var0", "iota"):
        assert np.array_equal(plan[k][:e[0]], clean[k][:e[0]]) and np.array_equal(plan[k][e[0] + e[1]:], clean[k][e[0] + e[1]:]), k
    c = [s[7] for s in states]
    assert np.array_equal(plan["l_ptr0"][:c[0] + 1], clean["l_ptr0"][:c[0] + 1]) and np.array_equal(plan["l_ptr0"][c[0] + c[1]:], clean["l_ptr0"][c[0] + c[1]:])
    assert np.array_equal(plan["l_ptr1"], clean["l_ptr1"]) and np.array_equal(plan["var1"], clean["var1"])
    # ... and their scores the bits of their solo calls
    for s, q in zip((0, 2), solo):
        assert np.array_equal(got[s].numpy(), q.numpy()), s
        np.testing.assert_allclose(got[s].numpy(), oracle_scores(params, states[s]), rtol=RTOL, atol=ATOL)
        assert list(got[s].rankings) == sorted(range(len(q)), key=lambda x: got[s][x], reverse=True)
