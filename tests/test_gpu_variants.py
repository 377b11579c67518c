"""Forced dispatch variants (GPU): every tuning knob of tools/README.md that picks another kernel or partition, set on the
non-default side in a child process that loads the experiment build (libgcnn_hip_tuning.so, -DGCNN_TUNING) -- the product
library has the knobs compiled in as constants, so only that build can run the other side.

Each child runs the same inputs (a setcov x 6 batch, a combauc sample, the 70,000-row and 66,000-variable stress states and a
state whose hub rows make the default edge pass give segments 64 lanes) through the fused training step, the autograd
backward, a no-grad forward and `score_state(rank=True)`, and writes the results and the library's launch record to an .npz.
Proof that a variant ran: the child's stderr carries the library's `gcnn knob NAME=value` line for every forced knob, and
where the launch record tells the variants apart it is asserted (`k_embed_fwd_split`; `+ long segments`).

What must be equal to the last bit, and why:
  * GCNN_SPLIT_MAX_TILES 0 / 1,000,000 against 256: everything.  The four-waves-per-tile programs keep the MFMA order per output
    element of the one-wave programs (k_rows_split.hpp header), and the loss head's partials are per tile in both (HEAD_SLAB).
  * GCNN_ROWS_WAVES 4 / 8, GCNN_EMB_CAP 256 / 509: everything.  A tile is walked by one wave (or one block, split) whichever
    block it is dealt to; no row program reduces over a block (the head partials are per tile, k_rows.hpp loss_head_tile).
  * GCNN_WG_SHARE 0 against 1: everything.  place_wg only reorders the weight-gradient jobs; a job's block count and rows per
    wave depend on the job and the chunk size alone, and its slabs are reduced in their own fixed order.
What goes to the fp64 oracle only (tests/gradparity.py's rule, the stress sweep's bound):
  * GCNN_SLOTS4_DEG / GCNN_SLOTS2_DEG forcing 16, 32 and 64 lanes per segment: the lanes of a segment split its edges
    differently, so the scatter-sum's order changes;
  * GCNN_WG_ROWS 16, 64 and the largest multiple of 16: the chunk size moves the weight-gradient slab boundaries.
    Their forward scores must still be the default's bits wherever only the weight gradients move (WG_ROWS)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
import gradparity  # noqa: E402
from gpucommon import make_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_LIB = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc", "libgcnn_hip_tuning.so")
INPUTS = ("setcov6", "combauc", "rows70k", "vars66k", "hubs")
BIG = 1_000_000_000
# (id, knobs, outputs bit-equal to the baseline: "all" | "scores" (forward only) | None (oracle only))
CONFIGS = [
    ("split256", {"GCNN_SPLIT_MAX_TILES": 256}, "all"),          # the baseline: the product's default
    ("split0", {"GCNN_SPLIT_MAX_TILES": 0}, "all"),
    ("splitall", {"GCNN_SPLIT_MAX_TILES": 1_000_000}, "all"),
    ("waves4", {"GCNN_ROWS_WAVES": 4}, "all"),
    ("waves8", {"GCNN_ROWS_WAVES": 8}, "all"),
    ("emb256", {"GCNN_EMB_CAP": 256}, "all"),
    ("emb509", {"GCNN_EMB_CAP": 509}, "all"),
    ("share0", {"GCNN_WG_SHARE": 0}, "all"),
    ("lanes16", {"GCNN_SLOTS4_DEG": BIG, "GCNN_SLOTS2_DEG": BIG}, None),
    ("lanes32", {"GCNN_SLOTS4_DEG": BIG, "GCNN_SLOTS2_DEG": 0}, None),
    ("lanes64", {"GCNN_SLOTS4_DEG": 0}, None),     # (GCNN_SLOTS2_DEG is then never read: no knob line for it)
    ("wg16", {"GCNN_WG_ROWS": 16}, "scores"),
    ("wg64", {"GCNN_WG_ROWS": 64}, "scores"),
    ("wgmax", {"GCNN_WG_ROWS": (2 ** 31 - 1) & ~15}, "scores"),
]
PHASES = ("train", "autograd", "nograd", "infer")

CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
from gcnn_cut_selector_amd import _lib
from gcnn_cut_selector_amd.trainer import TrainState, train_step
import test_gpu_variants as T
assert _lib.LIB_PATH == {lib!r}, _lib.LIB_PATH
dev = torch.device("cuda", 0)
m, _ = T.model(dev)
out = {{}}
for name in T.INPUTS:
    state, y = T.make_input(name)
    yt = torch.as_tensor(y, dtype=torch.float32).to(dev)
    batch = m.prepare(state)
    ts = TrainState(m)
    with _lib.launch_profile() as p:
        loss, scores = train_step(m, batch, yt, None, ts)
        torch.cuda.synchronize()
    out[name + "/train_grads"] = ts.grads.cpu().numpy(); out[name + "/train_scores"] = scores.cpu().numpy()
    out[name + "/train_loss"] = np.float32(float(loss)); out[name + "/train_launches"] = "\n".join(n for n, _ in p.launches)
    with _lib.launch_profile() as p:
        pred = m(batch, True)
        l2 = ((pred - yt) ** 2).mean()
        m.flat_parameters.grad = None
        l2.backward()
        torch.cuda.synchronize()
    out[name + "/autograd_grads"] = m.flat_parameters.grad.cpu().numpy(); out[name + "/autograd_scores"] = pred.detach().cpu().numpy()
    out[name + "/autograd_launches"] = "\n".join(n for n, _ in p.launches)
    with _lib.launch_profile() as p, torch.no_grad():
        out[name + "/nograd_scores"] = m(batch, False).cpu().numpy()
        torch.cuda.synchronize()
    out[name + "/nograd_launches"] = "\n".join(n for n, _ in p.launches)
    with _lib.launch_profile() as p:
        q = m.score_state(state, rank=True)
    out[name + "/infer_scores"] = np.asarray(q, np.float32).copy(); out[name + "/infer_rank"] = np.asarray(q.rankings)
    out[name + "/infer_launches"] = "\n".join(n for n, _ in p.launches)
np.savez({out!r}, **out)
print("CHILD OK")
"""


def model(dev):
    return make_model(11, dev)


def _hub_state():
    """5,000 constraint rows of mean degree ~44 (the default gives each segment 64 lanes; blocks per segment need n <= 4,096),
    a few hub rows of 300-900 entries among rows of ~40: forced to 16 or 32 lanes those are long segments."""
    rng = np.random.default_rng(77)
    C, V, K = 5000, 3000, 300
    deg = rng.integers(36, 45, C)
    deg[rng.choice(C, 12, replace=False)] = rng.integers(300, 900, 12)
    rows = np.repeat(np.arange(C), deg)
    cols = np.concatenate([np.sort(rng.choice(V, d, replace=False)) for d in deg])
    cei = np.stack([rows, cols]).astype(np.int32)
    kdeg = rng.integers(5, 20, K)
    kei = np.stack([np.repeat(np.arange(K), kdeg), np.concatenate([np.sort(rng.choice(V, d, replace=False)) for d in kdeg])]).astype(np.int32)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (f(C, 4), cei, f(cei.shape[1], 1), f(V, 14), f(K, 6), kei, f(kei.shape[1], 1), C, V, K), rng.uniform(0, 0.2, K)


def make_input(name):
    """(state 10-tuple, targets) of one named input -- deterministic, the same in every child."""
    from gcnn_cut_selector_amd import synthetic, utils
    if name == "setcov6":
        state, y, _ = synthetic.make_batch("setcov", 6)
        return state, np.asarray(y, np.float64)
    if name == "combauc":
        s, imp = synthetic.make_sample("combauc", 2)
        state = utils.state_to_inputs(s)
        return state, np.random.default_rng(5).uniform(0, 0.2, state[9])
    if name in ("rows70k", "vars66k"):
        import test_gpu_stress as S
        idx = 24 if name == "rows70k" else 25
        rng = np.random.default_rng(1000 + idx)
        state = S._state(S.CASES[idx], rng)
        return state, rng.uniform(0, 0.2, state[9])
    if name == "hubs":
        return _hub_state()
    raise KeyError(name)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One child per configuration, one at a time; the first failure ends the module (fixture errors are cached: no retry)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert os.path.exists(TUNING_LIB), "build() makes libgcnn_hip_tuning.so"
    tmp = tmp_path_factory.mktemp("variants")
    tests = os.path.dirname(os.path.abspath(__file__))
    out = {}
    for cid, knobs, _ in CONFIGS:
        path = str(tmp / f"{cid}.npz")
        env = dict(os.environ, GCNN_LIB=TUNING_LIB, **{k: str(v) for k, v in knobs.items()})
        for k in ("GCNN_SPLIT_MAX_TILES", "GCNN_ROWS_WAVES", "GCNN_EMB_CAP", "GCNN_WG_SHARE", "GCNN_SLOTS4_DEG", "GCNN_SLOTS2_DEG",
                  "GCNN_WG_ROWS", "GCNN_WG_COST2", "GCNN_WG_COST3", "GCNN_WG_COST3K"):
            if k not in knobs:
                env.pop(k, None)
        script = CHILD.format(root=ROOT, tests=tests, lib=TUNING_LIB, out=path)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, f"{cid}: exit {r.returncode}\n{r.stderr[-3000:]}"
        for k, v in knobs.items():   # the library's own word that it took the value
            assert f"gcnn knob {k}={v}" in r.stderr.splitlines(), f"{cid}: no knob line for {k}={v}\n{r.stderr[-2000:]}"
        with np.load(path) as z:
            out[cid] = {k: z[k] for k in z.files}
    return out


@pytest.fixture(scope="module")
def oracle():
    """fp64 scores and gradients of every input, and the fp32 weights they ran with."""
    params = O.randomize_params(O.init_params(11, np.float32), 12)   # gpucommon.make_model(11)'s weights
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    res = {}
    for name in INPUTS:
        state, y = make_input(name)
        _, loss, grads = O.loss_and_grads(p64, state, y, torch.float64)
        res[name] = (state, y, O.scores(p64, state, torch.float64), loss, grads)
    return params, res


def _launches(run, name, phase):
    return run[f"{name}/{phase}_launches"].item().split("\n")


def _grads(flat):
    from gcnn_cut_selector_amd import _lib
    layout, _ = _lib.param_layout()
    return {n: flat[off:off + r * c].reshape(shape) for (n, shape, t), (off, r, c, _) in zip(O.PARAM_SPEC, layout) if t}


def _check_oracle(run, cid, oracle):
    params, res = oracle
    for name in INPUTS:
        state, y, want, want_loss, want_grads = res[name]
        for key in ("train_scores", "autograd_scores", "nograd_scores", "infer_scores"):
            np.testing.assert_allclose(run[f"{name}/{key}"], want, rtol=1e-4, atol=1e-4, err_msg=f"{cid} {name} {key}")
        q = run[f"{name}/infer_scores"]
        assert list(run[f"{name}/infer_rank"]) == sorted(range(len(q)), key=lambda i: q[i], reverse=True), (cid, name)
        assert abs(float(run[f"{name}/train_loss"]) - want_loss) <= 1e-4 * max(1.0, abs(want_loss)), (cid, name)
        for key in ("autograd_grads", "train_grads"):
            flips = gradparity.check(_grads(run[f"{name}/{key}"]), params, state, y,
                                     lambda ref, gap: max(1e-4 * ref, 3 * gap) + 1e-7 * ref, want64=want_grads)
            if flips:
                print(f"\nvariant {cid} {name} {key}: gradients match the fp64 oracle with ReLU units {flips} flipped")


def test_baseline_matches_the_fp64_oracle(runs, oracle):
    _check_oracle(runs["split256"], "split256", oracle)


@pytest.mark.parametrize("cid", [c for c, _, eq in CONFIGS if eq == "all" and c != "split256"])
def test_forced_variant_gives_the_same_bits(runs, cid):
    base, run = runs["split256"], runs[cid]
    diff = [k for k in base if not k.endswith("_launches") and not np.array_equal(base[k], run[k])]
    assert not diff, f"{cid}: outputs that differ in bits from the default variants: {diff}"


def test_split_knob_switches_the_row_programs(runs):
    """The proof the split test needs: with 256 the small row sets take k_rows_split.hpp (the combauc sample's embeddings,
    inference and training alike), with 0 nothing does, with 1,000,000 every embedding launch does."""
    for name in INPUTS:
        for phase in PHASES:
            assert "k_embed_fwd_split" not in _launches(runs["split0"], name, phase), (name, phase)
    assert "k_embed_fwd_split" in _launches(runs["split256"], "combauc", "train")
    assert "k_embed_fwd" in _launches(runs["split0"], "combauc", "train")
    for name in INPUTS:
        for phase in ("train", "autograd", "nograd"):
            got = _launches(runs["splitall"], name, phase)
            assert "k_embed_fwd_split" in got and "k_embed_fwd" not in got, (name, phase)
    assert "k_embed_fwd" in _launches(runs["split256"], "rows70k", "train")


def test_forced_lanes_reach_the_long_segment_pass(runs):
    """The hub rows are long segments for 16 and 32 lanes (> 32 * slots edges) and not for 64 lanes (no long-segment pass)."""
    for cid in ("lanes16", "lanes32"):
        assert "k_edge_fwd<count> + long segments" in _launches(runs[cid], "hubs", "train"), cid
    for cid in ("lanes64", "split256"):
        assert "k_edge_fwd<count> + long segments" not in _launches(runs[cid], "hubs", "train"), cid


@pytest.mark.parametrize("cid", [c for c, _, eq in CONFIGS if eq != "all"])
def test_forced_variant_matches_the_fp64_oracle(runs, oracle, cid):
    _check_oracle(runs[cid], cid, oracle)
    if [eq for c, _, eq in CONFIGS if c == cid][0] == "scores":   # only the weight gradients' partition moved
        base, run = runs["split256"], runs[cid]
        for name in INPUTS:
            for key in ("train_scores", "train_loss", "autograd_scores", "nograd_scores", "infer_scores"):
                assert np.array_equal(base[f"{name}/{key}"], run[f"{name}/{key}"]), (cid, name, key)
