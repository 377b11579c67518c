"""The weight-gradient tail of a training step (k_wgrad with its four job bodies and the d w_edge pre-reduction, k_reduce,
fold_block / fold_chain, place_wg) at every chunk seam, with planted rows (GPU).

Cases and their proof are in tests/wgradcases.py and tests/test_wgradcases.py: every case puts up to eight isolated components
(cut k* - variable v* - constraint c*, target Y_STAR) on the rows where the restated index arithmetic has a seam, and a row that is
dropped, counted twice or replaced by its clamped neighbour moves every targeted tensor by at least ten times the bound used
here.  Per case: the fused training step and the autograd backward on `make_model(11)`, all 46 gradients against the fp64 oracle
through `gradparity.check` under the project's bound max(1e-4 ref, 3 gap) + 1e-7 ref, the loss within 1e-4, fused against
autograd as tests/test_gpu_dispatch.py requires, and `k_wgrad`, `k_reduce` and (where the restatement says a long-segment pass
runs) `k_edge_bwd_send + long segments` in the launch record.

Without a tolerance: the same case twice; GCNN_WG_SHARE=0 against 1 (children on the tuning build); the longest segment unknown
against known; a group of two members against the solo steps (the seam case second: its blocks at a non-zero offset); and the
cases of 1 / 17 / 65 / 1,000 rows from the NaN-filled, guarded workspace of tests/test_gpu_write_through.py (an all-empty block
must store its zero slab: at 1,000 rows the fifth block of the variables' recomputing job has no row).

The tuning-library cases (GCNN_WG_ROWS=16: 64 rows per slab, so that a reduced tensor has 1 .. 33 and a folded convolution
32 / 33 / 128 / 129 slabs) run in one child per knob setting, one at a time, each under a timeout; the first failing child ends
the module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
import gradparity  # noqa: E402
import wgradcases as W  # noqa: E402
import gpucommon as WT  # noqa: E402
from gpucommon import make_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_LIB = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc", "libgcnn_hip_tuning.so")
LONG = "k_edge_bwd_send + long segments"
PRODUCT = [c["id"] for c in W.cases() if c["lib"] == "product"]
TUNING = [c["id"] for c in W.cases() if c["lib"] == "wg16"]
GUARDED = [cid for cid in PRODUCT if cid.split("/")[0] in ("n1", "n17", "n65", "n1000")]
GROUPED = ["n65/0", "n1000/15", "aloneV/n1000/0", "dw/257/long"]
BOUND = lambda ref, gap: max(1e-4 * ref, 3 * gap) + 1e-7 * ref
# (id, knobs, the cases the child runs)
CHILDREN = [("wg16", {"GCNN_WG_ROWS": 16}, TUNING), ("share1", {"GCNN_WG_SHARE": 1}, PRODUCT), ("share0", {"GCNN_WG_SHARE": 0}, PRODUCT)]
KNOBS = ("GCNN_SPLIT_MAX_TILES", "GCNN_ROWS_WAVES", "GCNN_EMB_CAP", "GCNN_WG_SHARE", "GCNN_SLOTS4_DEG", "GCNN_SLOTS2_DEG",
         "GCNN_WG_ROWS", "GCNN_WG_COST2", "GCNN_WG_COST3", "GCNN_WG_COST3K")


def prepare(m, cid):
    """(state, targets, the prepared batch) of a case, the longest segments adopted or forgotten as the case says."""
    case = W.case(cid)
    state, y, _ = W.build(case)
    batch = m.prepare(state)
    torch.cuda.synchronize()
    for g in (batch.cons_graph, batch.cut_graph):
        g.c   # adopt the longest segments (their copy has landed)
        if not case["known"]:
            g._md_ticket = None
            g.l_max_deg = g.v_max_deg = 0
            g._bind()
    return state, y, batch


def run_case(m, cid, autograd=True):
    """The fused step (and the autograd backward) of one case: flat gradients, loss and the fused step's launch names."""
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.trainer import TrainState, train_step
    _, y, batch = prepare(m, cid)
    yt = torch.as_tensor(y, dtype=torch.float32).to(m.device)
    ts = TrainState(m)
    with _lib.launch_profile() as p:
        loss, _ = train_step(m, batch, yt, None, ts)
        torch.cuda.synchronize()
    r = {"train_grad": ts.grads.cpu().numpy(), "train_loss": np.float32(float(loss)), "launches": "\n".join(n for n, _ in p.launches)}
    if autograd:
        pred = m(batch, True)
        l2 = ((pred - yt) ** 2).mean()
        m.flat_parameters.grad = None
        l2.backward()
        torch.cuda.synchronize()
        r["flat_grad"], r["loss"] = m.flat_parameters.grad.cpu().numpy(), np.float32(float(l2.detach()))
    return r


CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
from gcnn_cut_selector_amd import _lib
import test_gpu_wgrad_seams as T
from gpucommon import make_model
assert _lib.LIB_PATH == {lib!r}, _lib.LIB_PATH
m, _ = make_model(11, torch.device("cuda", 0))
out = {{}}
for cid in {ids!r}:
    for k, v in T.run_case(m, cid, autograd={autograd!r}).items():
        out[cid + "|" + k] = v
np.savez({out!r}, **out)
print("CHILD OK")
"""


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """One child per knob setting on the tuning build, one at a time; the first failure ends the module."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert os.path.exists(TUNING_LIB), "build() makes libgcnn_hip_tuning.so"
    tmp = tmp_path_factory.mktemp("wgrad_seams")
    out = {}
    for tag, knobs, ids in CHILDREN:
        path = str(tmp / f"{tag}.npz")
        env = dict(os.environ, GCNN_LIB=TUNING_LIB, **{k: str(v) for k, v in knobs.items()})
        for k in KNOBS:
            if k not in knobs:
                env.pop(k, None)
        script = CHILD.format(root=ROOT, tests=os.path.dirname(os.path.abspath(__file__)), lib=TUNING_LIB, out=path, ids=ids, autograd=tag == "wg16")
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, f"{tag}: exit {r.returncode}\n{r.stderr[-3000:]}"
        for k, v in knobs.items():
            assert f"gcnn knob {k}={v}" in r.stderr.splitlines(), f"{tag}: no knob line for {k}={v}\n{r.stderr[-2000:]}"
        with np.load(path) as z:
            out[tag] = {k: z[k] for k in z.files}
    return out


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return make_model(11, torch.device("cuda", 0))


@pytest.fixture(scope="module")
def product(model):
    """Every product-library case, run twice."""
    m, _ = model
    return {cid: (run_case(m, cid), run_case(m, cid)) for cid in PRODUCT}


def _grads(flat):
    from gcnn_cut_selector_amd import _lib
    layout, _ = _lib.param_layout()
    return {n: flat[off:off + r * c].reshape(shape) for (n, shape, t), (off, r, c, _) in zip(O.PARAM_SPEC, layout) if t}


def _klass(name):
    return "d w_edge" if "feat_edge" in name else "folded" if ("feat_final" in name or "conv_out_1" in name) else \
        "embedding" if "_emb_" in name else "other"


def _check(cid, r, params):
    """Oracle parity of one run; prints the distance per tensor class (largest error over largest entry)."""
    case = W.case(cid)
    state, y, _ = W.build(case)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    _, want_loss, want = O.loss_and_grads(p64, state, y, torch.float64)
    names = r["launches"].item().split("\n") if isinstance(r["launches"], np.ndarray) else r["launches"].split("\n")
    assert "k_wgrad" in names and "k_reduce" in names, names
    expect_long = any(p["nlong"] > 0 for p in W.send_plans(case, state).values())
    assert (LONG in names) == expect_long, (cid, expect_long, names)
    dist = {}
    for key in ("train_grad", "flat_grad"):
        got = _grads(r[key])
        for n in gradparity.NAMES:
            d = float(np.abs(got[n].astype(np.float64) - want[n]).max()) / max(float(np.abs(want[n]).max()), 1e-6)
            dist[_klass(n)] = max(dist.get(_klass(n), 0.0), d)
    print(f"\n{cid}: distance / largest entry per class: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(dist.items())))
    for key in ("train_grad", "flat_grad"):
        flips = gradparity.check(_grads(r[key]), params, state, y, BOUND, want64=want)
        if flips:
            print(f"{cid} {key}: gradients match the fp64 oracle with ReLU units {flips} flipped")
    assert abs(float(r["loss"]) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    assert abs(float(r["train_loss"]) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    ga, gf = r["flat_grad"], r["train_grad"]
    np.testing.assert_allclose(gf, ga, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ga).max())))


@pytest.mark.parametrize("cid", PRODUCT)
def test_seam_case_matches_the_fp64_oracle(product, model, cid):
    _check(cid, product[cid][0], model[1])


@pytest.mark.parametrize("cid", TUNING)
def test_sixteen_row_chunks_match_the_fp64_oracle(children, model, cid):
    r = {k.split("|", 1)[1]: v for k, v in children["wg16"].items() if k.startswith(cid + "|")}
    _check(cid, r, model[1])


def _same(a, b, keys=("train_grad", "train_loss")):
    return [k for k in keys if not np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32))]


def test_the_same_case_twice_gives_the_same_bytes(product):
    diff = {cid: _same(a, b, ("train_grad", "train_loss", "flat_grad", "loss")) for cid, (a, b) in product.items()}
    assert not any(diff.values()), {k: v for k, v in diff.items() if v}


def test_job_order_without_sharing_gives_the_same_bytes(children):
    a, b = children["share1"], children["share0"]
    diff = [k for k in a if not k.endswith("launches") and not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]
    assert not diff, diff


def test_unknown_longest_segment_gives_the_bytes_of_the_known_one(product):
    pairs = [(cid, cid.replace("unknown", "known")) for cid in PRODUCT if cid.endswith("/unknown")]
    assert len(pairs) == 5
    for u, k in pairs:
        assert LONG in product[u][0]["launches"].split("\n") and LONG not in product[k][0]["launches"].split("\n"), u
        assert not _same(product[u][0], product[k][0], ("train_grad", "train_loss", "flat_grad", "loss")), u


@pytest.mark.parametrize("cid", GROUPED)
def test_group_member_gives_the_bytes_of_the_solo_step(product, cid):
    """The seam case as the second of two members: wgrad_body / reduce_body get their share of the grid at a block offset."""
    from gcnn_cut_selector_amd.trainer import TrainState, train_step, train_step_group
    dev = torch.device("cuda", 0)
    ms = [make_model(11, dev)[0] for _ in range(2)]
    small, ys = WT.make_state(50, 60, 20, seed=7)
    _, y, batch = prepare(ms[1], cid)
    batches = [ms[0].prepare(small), batch]
    yt = [torch.as_tensor(v, dtype=torch.float32).to(dev) for v in (ys, y)]
    solo = TrainState(ms[0])
    loss0, _ = train_step(ms[0], batches[0], yt[0], None, solo)
    torch.cuda.synchronize()
    want0 = (solo.grads.cpu().numpy().copy(), float(loss0))
    ts = [TrainState(m) for m in ms]
    out = train_step_group(ms, batches, yt, [None, None], ts)
    torch.cuda.synchronize()
    assert np.array_equal(ts[0].grads.cpu().numpy().view(np.uint32), want0[0].view(np.uint32)) and float(out[0][0]) == want0[1]
    got = {"train_grad": ts[1].grads.cpu().numpy(), "train_loss": np.float32(float(out[1][0]))}
    assert not _same(got, product[cid][0]), cid


@pytest.mark.parametrize("cid", GUARDED)
def test_step_from_a_nan_filled_guarded_workspace(product, cid):
    """No guard word changes, no NaN reaches a result, and the gradients are those of the step through an ordinary workspace."""
    m, _ = make_model(11, torch.device("cuda", 0))
    state, y, _ = W.build(W.case(cid))
    res, words, need, _ = WT.run_step(m, state, y)
    assert (words[need:need + WT.GUARD] == WT.PATTERN).all(), "the guard rows behind the workspace were written"
    for name in ("loss", "scores", "grads"):
        assert not np.isnan(res[name]).any() and not (res[name].view(np.uint32) == WT.PATTERN).any(), name
    got = {"train_grad": res["grads"], "train_loss": np.float32(res["loss"].reshape(-1)[0])}
    assert not _same(got, product[cid][0]), cid
