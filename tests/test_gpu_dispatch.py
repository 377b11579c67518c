"""Dispatch boundaries (GPU, product library): deterministic states with controlled degrees and sizes, one just inside and one
just outside each threshold at which gcnn_capi.hip picks another kernel variant, each checked against the fp64 oracle with the
stress sweep's rules (test_gpu_stress.py): scores of the no-grad forward and of `score_state(rank=True)` within 1e-4, the
ranking exact, all 46 gradients within the bound with any ReLU flip proven (tests/gradparity.py), the fused training step
against the autograd path, and its loss.  Where the launch record (`_lib.launch_profile`) tells the two sides apart it is
asserted too:
  * long segments (> 32 * slots edges, k_edge.hpp edge_long_threshold): `+ long segments` with the longest segment known, on
    both sides when it is unknown;
  * a block per segment (n <= 4,096 and E >= 48 n): `k_edge_fwd_block<count>` against `k_edge_fwd<count>`;
  * the fused inference plan (n <= 16,384 and <= 4,096 variables): `k_infer_s2` / `k_infer_s3` against `k_iplan_place` /
    `k_iplan_order`;
  * split embeddings (<= 256 tiles over the three row sets): `k_embed_fwd_split` against `k_embed_fwd`;
  * ranking on the device for more than 1,024 cuts (`k_rank_scores`), the general path above 4,096.
Thresholds that rely on oracle parity alone, since both sides launch under the same name: lanes per segment (mean degree 12
and 40), 64 lanes for inference up to 16,384 receivers, the plan's block-per-segment form (n <= 1,024 and E >= 48 n), the
variable-degree limits of the plan (256: LDS-staged segments; 2,048: beyond it the general path) and 32,768 variables, four
waves per tile for one row set of 4,096 / 4,097 rows, 8 waves above 1,024 tiles, spreading below 2,048 tiles, and the
two-blocks-per-CU embedding launch from 8,192 tiles.
The last test requires every launch name gcnn_capi.hip can record (tests/launchnames.py) to appear in some recorded launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
import gradparity  # noqa: E402
import launchnames  # noqa: E402
from gpucommon import make_model  # noqa: E402

LONG = "k_edge_fwd<count> + long segments"


def _rows(n, E):
    """n row degrees summing to E, as even as possible."""
    d = np.full(n, E // n, np.int64)
    d[: E % n] += 1
    return d


def _with(d, idx, value):
    d = d.copy()
    d[idx] = value
    return d


# id -> (C, V, K, constraint-row degrees, cut-row degrees, variable 0's constraint degree or None, longest segment known)
def _cases():
    c = {}
    for tag, C, V, E in (("12n-1", 3000, 4000, 12 * 3000 - 1), ("12n", 3000, 4000, 12 * 3000),
                         ("40n-1", 5000, 6000, 40 * 5000 - 1), ("40n", 5000, 6000, 40 * 5000)):
        c[f"lanes/{tag}"] = (C, V, 200, _rows(C, E), _rows(200, 1000), None, True)
    for known in (True, False):
        k = "known" if known else "unknown"
        for L in (32, 33):     # 16 lanes (mean degree ~4)
            c[f"long16/{L}/{k}"] = (5000, 3000, 100, _with(_rows(5000, 20000), slice(0, 10), L), _rows(100, 500), None, known)
        for L in (64, 65):     # 32 lanes (mean degree ~14)
            c[f"long32/{L}/{k}"] = (5000, 12000, 100, _with(_rows(5000, 70000), slice(0, 10), L), _rows(100, 500), None, known)
    c["block/4096/48n"] = (500, 3000, 4096, _rows(500, 2500), _rows(4096, 48 * 4096), None, True)
    c["block/4096/48n-1"] = (500, 3000, 4096, _rows(500, 2500), _rows(4096, 48 * 4096 - 1), None, True)
    c["block/4097/48n"] = (500, 3000, 4097, _rows(500, 2500), _rows(4097, 48 * 4097), None, True)
    c["infer/16384"] = (16384, 3000, 100, _rows(16384, 3 * 16384), _rows(100, 500), None, True)
    c["infer/16385"] = (16385, 3000, 100, _rows(16385, 3 * 16385), _rows(100, 500), None, True)
    c["fuse/4096"] = (1000, 4096, 100, _rows(1000, 6000), _rows(100, 500), None, True)
    c["fuse/4097"] = (1000, 4097, 100, _rows(1000, 6000), _rows(100, 500), None, True)
    c["blockseg/1024"] = (1024, 3000, 100, _rows(1024, 48 * 1024), _rows(100, 500), None, True)
    c["blockseg/1025"] = (1025, 3000, 100, _rows(1025, 48 * 1025), _rows(100, 500), None, True)
    for D in (256, 257, 2048, 2049):
        c[f"vdeg/{D}"] = (2100, 400, 50, _rows(2100, 6300), _rows(50, 250), D, True)
    for V in (16 * 1024, 16 * 1024 + 1, 16 * 2047, 16 * 2048, 16 * 2048 + 1):   # row tiles of conv c->v: 1024 / 1025, 2047 / 2048; 32,768 / 32,769 variables
        c[f"vars/{V}"] = (1000, V, 50, _rows(1000, 4000), _rows(50, 250), None, True)
    c["split3/256"] = (1600, 1600, 896, _rows(1600, 8000), _rows(896, 4480), None, True)
    c["split3/257"] = (1600, 1600, 897, _rows(1600, 8000), _rows(897, 4485), None, True)
    c["embcap/8191"] = (160, 16 * 8171, 160, _rows(160, 3200), _rows(160, 800), None, True)
    c["embcap/8192"] = (160, 16 * 8172, 160, _rows(160, 3200), _rows(160, 800), None, True)
    return c


CASES = _cases()


def _edges(rng, deg, V, hub=None):
    """(row, col)-sorted COO with `deg[i]` distinct columns in row i; with `hub`, column 0 sits in exactly the first `hub` rows
    and no other."""
    n = len(deg)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    rows = np.repeat(np.arange(n), deg)
    k = np.arange(ptr[-1]) - np.repeat(ptr[:-1], deg)
    lo = 0 if hub is None else 1
    cols = lo + (np.repeat(rng.integers(0, V - lo, n), deg) + k) % (V - lo)
    if hub is not None:
        rows = np.concatenate([rows, np.arange(hub)])
        cols = np.concatenate([cols, np.zeros(hub, np.int64)])
    order = np.lexsort((cols, rows))
    return np.stack([rows[order], cols[order]]).astype(np.int32)


def make_state(cid):
    C, V, K, cdeg, kdeg, hub, _ = CASES[cid]
    rng = np.random.default_rng(sum(map(ord, cid)))
    cei, kei = _edges(rng, cdeg, V, hub), _edges(rng, kdeg, V)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    state = (f(C, 4), cei, f(cei.shape[1], 1), f(V, 14), f(K, 6), kei, f(kei.shape[1], 1), C, V, K)
    return state, rng.uniform(0, 0.2, K)


def _names(prof):
    return [n for n, _ in prof.launches]


@pytest.fixture(scope="module")
def results():
    """Every case run once on the GPU, with its launch record per phase; and the extra calls that reach the remaining
    launch names (PreNorm statistics with the two-layer forward, the stand-alone MSE and Adam, a fused Adam step)."""
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.trainer import Adam, TrainState, mse_loss, train_step
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda", 0)
    m, params = make_model(11, dev)
    out, seen = {}, set()
    for cid in CASES:
        state, y = make_state(cid)
        r = {}
        yt = torch.as_tensor(y, dtype=torch.float32).to(dev)
        batch = m.prepare(state)
        torch.cuda.synchronize()
        for g in (batch.cons_graph, batch.cut_graph):
            g.c   # adopt the longest segments (their copy has landed)
            if not CASES[cid][6]:
                g._md_ticket = None
                g.l_max_deg = g.v_max_deg = 0
                g._bind()
        with torch.no_grad(), _lib.launch_profile() as p:
            r["nograd"] = m(batch, False).numpy()
        r["nograd_launches"] = _names(p)
        with _lib.launch_profile() as p:
            q = m.score_state(state, rank=True)
        r["infer"], r["rank"], r["infer_launches"] = np.asarray(q).copy(), np.asarray(q.rankings).copy(), _names(p)
        with _lib.launch_profile() as p:
            pred = m(batch, True)
            loss = ((pred - yt) ** 2).mean()
            m.flat_parameters.grad = None
            loss.backward()
            torch.cuda.synchronize()
        r["autograd_launches"] = _names(p)
        r["loss"] = float(loss.detach())
        r["grads"] = {n: g.cpu().numpy() for n, g in zip(gradparity.NAMES, m.gradients())}
        r["flat_grad"] = m.flat_parameters.grad.cpu().numpy()
        ts = TrainState(m)
        with _lib.launch_profile() as p:
            loss2, _ = train_step(m, batch, yt, None, ts)
            torch.cuda.synchronize()
        r["train_launches"] = _names(p)
        r["train_grad"], r["train_loss"] = ts.grads.cpu().numpy(), float(loss2)
        for k in ("nograd_launches", "infer_launches", "autograd_launches", "train_launches"):
            seen.update(r[k])
        out[cid] = (state, y, r)
    # the rest of the library's launches, on the smallest case of the list above
    m2, _ = make_model(12, dev)
    state, y = make_state("vdeg/256")
    yt = torch.as_tensor(y, dtype=torch.float32).to(dev)
    with _lib.launch_profile() as p:
        m2.pretrain_init()
        while m2.pretrain(state):   # one PreNorm layer per pass, layers 5-10 after the two-layer forward
            m2.pretrain_next()
        scores = m2(state, False)
        mse_loss(scores.detach(), yt)
        ts, opt = TrainState(m2), Adam(1e-4)
        train_step(m2, m2.prepare(state), yt, opt, ts)
        opt.apply_flat(m2, ts.grads)
        torch.cuda.synchronize()
    seen.update(_names(p))
    return params, out, seen


@pytest.mark.parametrize("cid", list(CASES))
def test_boundary_case_matches_the_fp64_oracle(results, cid):
    params, out, _ = results
    state, y, r = out[cid]
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    want = O.scores(p64, state, torch.float64)
    np.testing.assert_allclose(r["nograd"], want, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(r["infer"], want, rtol=1e-4, atol=1e-4)
    assert list(r["rank"]) == sorted(range(len(want)), key=lambda i: r["infer"][i], reverse=True)
    _, want_loss, want_grads = O.loss_and_grads(p64, state, y, torch.float64)
    assert abs(r["loss"] - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    flips = gradparity.check(r["grads"], params, state, y, lambda ref, gap: max(1e-4 * ref, 3 * gap) + 1e-7 * ref, want64=want_grads)
    if flips:
        print(f"\ndispatch case {cid}: gradients match the fp64 oracle with ReLU units {flips} flipped")
    ga, gf = r["flat_grad"], r["train_grad"]
    np.testing.assert_allclose(gf, ga, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ga).max())))
    assert abs(r["train_loss"] - want_loss) <= 1e-4 * max(1.0, abs(want_loss))


def _has(results, cid, phase, name):
    return name in results[1][cid][2][phase + "_launches"]


def test_long_segment_pass_runs_exactly_where_a_segment_is_long(results):
    for lanes, short, long_ in (("long16", 32, 33), ("long32", 64, 65)):
        assert not _has(results, f"{lanes}/{short}/known", "train", LONG), lanes
        assert _has(results, f"{lanes}/{long_}/known", "train", LONG), lanes
        for L in (short, long_):    # longest segment unknown: the finder always runs
            assert _has(results, f"{lanes}/{L}/unknown", "train", LONG), (lanes, L)
            assert _has(results, f"{lanes}/{L}/unknown", "train", "k_edge_bwd_send + long segments"), (lanes, L)


def test_block_per_segment_boundary(results):
    assert _has(results, "block/4096/48n", "train", "k_edge_fwd_block<count>")
    assert _has(results, "block/4096/48n", "nograd", "k_edge_fwd_block")
    for cid in ("block/4096/48n-1", "block/4097/48n"):
        assert not _has(results, cid, "train", "k_edge_fwd_block<count>"), cid
        assert not _has(results, cid, "nograd", "k_edge_fwd_block"), cid
    assert _has(results, "block/4096/48n", "infer", "k_rank_scores")        # > 1,024 cuts: ranked on the device
    assert not _has(results, "block/4097/48n", "infer", "k_infer_s1 (embeddings + plan: count)")   # > 4,096: general path


def test_fused_inference_plan_boundary(results):
    s2, s3 = "k_infer_s2 (conv v->c edge pass + plan: place)", "k_infer_s3 (conv row program + plan: order)"
    for cid in ("fuse/4096", "infer/16384"):
        assert _has(results, cid, "infer", s2) and not _has(results, cid, "infer", "k_iplan_place"), cid
    assert _has(results, "fuse/4096", "infer", s3) and not _has(results, "fuse/4096", "infer", "k_iplan_order")
    for cid in ("fuse/4097", "infer/16385"):
        assert _has(results, cid, "infer", "k_iplan_place") and not _has(results, cid, "infer", s2), cid
    assert _has(results, "fuse/4097", "infer", "k_iplan_order") and not _has(results, "fuse/4097", "infer", s3)


def test_split_embedding_boundary(results):
    assert _has(results, "split3/256", "nograd", "k_embed_fwd_split") and not _has(results, "split3/256", "nograd", "k_embed_fwd")
    assert _has(results, "split3/257", "nograd", "k_embed_fwd") and not _has(results, "split3/257", "nograd", "k_embed_fwd_split")


def test_every_launch_name_is_recorded(results):
    names = launchnames.launch_names()
    missing = sorted(names - results[2])
    assert not missing, f"launch names of gcnn_capi.hip no case reached: {missing}"
