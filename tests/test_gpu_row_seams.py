"""The row programs (k_embed_fwd, k_conv_fwd, k_conv_turn, k_conv_bwd, k_tail_bwd with their _wt and _split forms, k_infer_s1/s3 and
the group twins) at every tile, wave, block and form seam, with planted rows (GPU).

Cases and their proof are in tests/rowcases.py and tests/test_rowcases.py: every case puts up to eight isolated components (cut k* -
variable v* - constraint c*, the target y* on k*, every other cut's target at its own score) on the rows at which the restated index arithmetic of the launch under test has a
seam, and a planted row that is lost, doubled or swapped moves every gradient tensor by at least ten times the bound used here and
its cut's score by at least ten times 1e-4.

ANCHOR, per case, on the product library with `make_model(11)`: the fused step and the autograd step, all 46 gradients against the
fp64 oracle through `gradparity.check` under the project's bound max(1e-4 ref, 3 gap) + 1e-7 ref, the loss within 1e-4, the scores
of the no-grad forward and of `score_state(rank=True)` within 1e-4 with the ranking exact, the fused step against the autograd step
as tests/test_gpu_dispatch.py requires; within the fused-inference limits `score_state` gives the no-grad forward's bits.

EVERY ROW, ACROSS FORMS, WITHOUT A TOLERANCE.  Each case runs from a workspace filled with `gpucommon.PATTERN` with guard rows behind
it (`gpucommon.run_step`, `gpucommon.run_autograd`) in nine child processes, one at a time, each under its own timeout, the first
failing child ending the module: the tuning build with default knobs, GCNN_ROWS_WAVES = 4 and 8, GCNN_SPLIT_MAX_TILES = 0 and
1,000,000, GCNN_EMB_CAP = 256 and 509, the product library and libgcnn_hip_plain.so.  Each child proves its setting by the library's
`gcnn knob ...` lines (the product and plain libraries: by their path and by printing none) and, where launch names differ, by the
launch record.  Between children: loss, scores, gradients of both steps, the scores of the no-grad forward and of `score_state`, and
the whole workspace after either step, word for word through one fingerprint per 64 words made on the device
(`gpucommon.fingerprint`); the guard rows intact; no pattern word in any result.  The comparison sees every row of every stored
tensor, forward and backward, independently of the restatement; what it cannot see is an error all nine forms share -- that is what
the anchor with its planted rows is for.  EXCLUDED lists the regions that legitimately differ between forms (none is known).

GROUP TWINS: a two-member `gcnn_group_train_step` with a seam case as its second member (its blocks at a non-zero offset) gives the
bits of the member's solo step, for one split case, one two-program case and one of 2,049 tiles.  THE SAME CASE TWICE, in two
processes: same bits."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
import gradparity  # noqa: E402
import rowcases as R  # noqa: E402
import gpucommon as G  # noqa: E402
from gpucommon import make_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
TUNING_LIB, PRODUCT_LIB, PLAIN_LIB = (os.path.join(CSRC, f"libgcnn_hip{s}.so") for s in ("_tuning", "", "_plain"))
IDS = [c["id"] for c in R.cases()]
GROUPED = ["K/4096", "pair/trim", "V/32769"]      # split (the cut rows' turnaround), two programs with the trim, 2,049 tiles
BOUND = lambda ref, gap: max(1e-4 * ref, 3 * gap) + 1e-7 * ref
KNOBS = ("GCNN_SPLIT_MAX_TILES", "GCNN_ROWS_WAVES", "GCNN_EMB_CAP", "GCNN_WG_SHARE", "GCNN_SLOTS4_DEG", "GCNN_SLOTS2_DEG",
         "GCNN_WG_ROWS", "GCNN_WG_COST2", "GCNN_WG_COST3", "GCNN_WG_COST3K")
DEFAULTS = {"GCNN_SPLIT_MAX_TILES": 256, "GCNN_ROWS_WAVES": 0, "GCNN_EMB_CAP": 0}
# (id, library, knobs)
CHILDREN = [("default", TUNING_LIB, {}), ("waves4", TUNING_LIB, {"GCNN_ROWS_WAVES": 4}), ("waves8", TUNING_LIB, {"GCNN_ROWS_WAVES": 8}),
            ("split0", TUNING_LIB, {"GCNN_SPLIT_MAX_TILES": 0}), ("splitall", TUNING_LIB, {"GCNN_SPLIT_MAX_TILES": 1_000_000}),
            ("emb256", TUNING_LIB, {"GCNN_EMB_CAP": 256}), ("emb509", TUNING_LIB, {"GCNN_EMB_CAP": 509}),
            ("product", PRODUCT_LIB, {}), ("plain", PLAIN_LIB, {})]
# Regions of the workspace that legitimately differ between forms: (child, case, [first word, last word)), the tensor and the source
# line that says no launch reads it.  None is known: every form stores the same tensors.
EXCLUDED = []
# the limits of the fused inference plan (tests/test_gpu_dispatch.py: n <= 16,384 receivers and <= 4,096 variables)
FUSED_INFER = lambda c: max(c["C"], c["K"]) <= 16384 and c["V"] <= 4096
RESULTS = ("fused/loss", "fused/scores", "fused/grads", "auto/loss", "auto/scores", "auto/grads", "nograd/scores", "infer/scores", "infer/rank")
COMPARED = RESULTS + ("fused/need", "fused/fp", "fused/pat", "auto/fp", "auto/pat")


def _guard_intact(ws, need):
    return np.bool_(bool((ws.view(torch.int32)[need:need + G.GUARD] == G.PATTERN).all()))


def settle(params):
    """{case: targets}: the planted targets, and every ordinary cut's own fp64 score (rowcases.settled), computed once per run."""
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    return {cid: R.settled(R.case(cid), lambda st: O.scores(p64, st, torch.float64))[1] for cid in IDS}


def run_case(m, cid, y):
    """Every path of one case on the loaded library: {name: array}."""
    from gcnn_cut_selector_amd import _lib
    state, _, _ = R.build(R.case(cid))
    out = {}
    with _lib.launch_profile() as p:
        res, _, need, ws = G.run_step(m, state, y, download=False)
    out["fused/launches"] = "\n".join(n for n, _ in p.launches)
    words = need + G.GUARD
    for k, v in res.items():
        out["fused/" + k] = v
    out["fused/need"] = np.int64(need)
    out["fused/fp"], out["fused/pat"] = G.fingerprint(ws, words)
    out["fused/guard"] = _guard_intact(ws, need)
    del ws
    with _lib.launch_profile() as p:
        res, need2, ws = G.run_autograd(m, state, y)
    assert need2 == need
    out["auto/launches"] = "\n".join(n for n, _ in p.launches)
    for k, v in res.items():
        out["auto/" + k] = v
    out["auto/fp"], out["auto/pat"] = G.fingerprint(ws, words)
    out["auto/guard"] = _guard_intact(ws, need)
    del ws
    m._ws_pool.clear()
    batch = m.prepare(state)
    with torch.no_grad(), _lib.launch_profile() as p:
        out["nograd/scores"] = m(batch, False).cpu().numpy()
        torch.cuda.synchronize()
    out["nograd/launches"] = "\n".join(n for n, _ in p.launches)
    with _lib.launch_profile() as p:
        q = m.score_state(state, rank=True)
    out["infer/scores"], out["infer/rank"] = np.asarray(q, np.float32).copy(), np.asarray(q.rankings).copy()
    out["infer/launches"] = "\n".join(n for n, _ in p.launches)
    m._ws_pool.clear()
    return out


CHILD = r"""
import sys, time
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
from gcnn_cut_selector_amd import _lib
import test_gpu_row_seams as T
from gpucommon import make_model
assert _lib.LIB_PATH == {lib!r}, _lib.LIB_PATH
m, _ = make_model(11, torch.device("cuda", 0))
out = {{}}
targets = np.load({targets!r})
t0 = time.perf_counter()
for cid in T.IDS:
    for k, v in T.run_case(m, cid, targets[cid]).items():
        out[cid + "|" + k] = v
out["seconds"] = np.float64(time.perf_counter() - t0)
np.savez({out!r}, **out)
print("CHILD OK")
"""


@pytest.fixture(scope="module")
def targets():
    return settle(O.randomize_params(O.init_params(11, np.float32), 12))     # gpucommon.make_model(11)'s weights


@pytest.fixture(scope="module")
def children(tmp_path_factory, targets):
    """One child per form, one at a time, each under its own timeout; the first failure ends the module."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    for lib in (TUNING_LIB, PRODUCT_LIB, PLAIN_LIB):
        assert os.path.exists(lib), f"build() makes {os.path.basename(lib)}"
    tmp = tmp_path_factory.mktemp("row_seams")
    tests = os.path.dirname(os.path.abspath(__file__))
    out, took = {}, {}
    np.savez(str(tmp / "targets.npz"), **targets)
    t_all = time.perf_counter()
    for tag, lib, knobs in CHILDREN:
        path = str(tmp / f"{tag}.npz")
        env = dict(os.environ, GCNN_LIB=lib, **{k: str(v) for k, v in knobs.items()})
        for k in KNOBS:
            if k not in knobs:
                env.pop(k, None)
        script = CHILD.format(root=ROOT, tests=tests, lib=lib, out=path, targets=str(tmp / "targets.npz"))
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=240)
        took[tag] = time.perf_counter() - t0
        assert r.returncode == 0 and "CHILD OK" in r.stdout, f"{tag}: exit {r.returncode}\n{r.stderr[-3000:]}"
        lines = r.stderr.splitlines()
        if lib == TUNING_LIB:      # the library's own word for the value it took, forced or default
            want = dict(DEFAULTS, **knobs)
            if tag == "splitall":      # every launch splits: the embedding launch never asks for its cap
                del want["GCNN_EMB_CAP"]
            for k, v in want.items():
                assert f"gcnn knob {k}={v}" in lines, f"{tag}: no knob line for {k}={v}\n{r.stderr[-2000:]}"
        else:                      # the product and the plain library read no knob
            assert not any(line.startswith("gcnn knob") for line in lines), tag
        with np.load(path) as z:
            out[tag] = {k: z[k] for k in z.files}
    total = time.perf_counter() - t_all
    slow = max(took, key=took.get)
    for tag in out:       # (the whole picture at once, before the per-form tests assert it)
        bad = {cid: d for cid in IDS for d in [_diff(tag, cid, _case(out["default"], cid), _case(out[tag], cid))] if d}
        if bad:
            print(f"\n{tag} differs from the default forms:\n" + "\n".join(f"  {c}: {d}" for c, d in bad.items()))
    print(f"\nrow seams: {len(CHILDREN)} children in {total:.1f} s; the longest, {slow}, {took[slow]:.1f} s "
          f"({float(out[slow]['seconds']):.1f} s of it in the cases)")
    return out


@pytest.fixture(scope="module")
def model(children):
    """(After the children: a child that failed ends the module before this process touches the GPU.)"""
    return make_model(11, torch.device("cuda", 0))


@pytest.fixture(scope="module")
def oracle(model, targets):
    """The fp64 oracle per case, computed once."""
    p64 = {k: v.astype(np.float64) for k, v in model[1].items()}
    cache = {}

    def get(cid):
        if cid not in cache:
            state, y = R.build(R.case(cid))[0], targets[cid]
            _, loss, grads = O.loss_and_grads(p64, state, y, torch.float64)
            cache[cid] = (state, y, O.scores(p64, state, torch.float64), loss, grads)
        return cache[cid]
    return get


def _grads(flat):
    from gcnn_cut_selector_amd import _lib
    layout, _ = _lib.param_layout()
    return {n: flat[off:off + r * c].reshape(shape) for (n, shape, t), (off, r, c, _) in zip(O.PARAM_SPEC, layout) if t}


def _case(run, cid):
    return {k.split("|", 1)[1]: v for k, v in run.items() if k.startswith(cid + "|")}


def _launches(r, path):
    return r[path + "/launches"].item().split("\n")


# ---- every row, across forms -----------------------------------------------------------------------------------------------------------------
def _runs(idx):
    """[first, last) runs of consecutive indices."""
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) > 1)
    return [(int(a), int(b) + 1) for a, b in zip(np.r_[idx[0], idx[cut + 1]], np.r_[idx[cut], idx[-1]])]


def _diff(tag, cid, a, b):
    """How one case's arrays of child `tag` differ from the default's: a list of strings."""
    bad = []
    for k in COMPARED:
        x, y = a[k], b[k]
        if x.shape != y.shape:
            bad.append(f"{k}: shape {y.shape} against {x.shape}")
            continue
        if k.endswith(("/fp", "/pat")):
            keep = np.ones(x.shape, bool)
            for t, c, (lo, hi), _ in EXCLUDED:
                if t == tag and c == cid:
                    keep[lo // G.FP_WORDS:-(-hi // G.FP_WORDS)] = False
            rows = np.flatnonzero((x != y) & keep)
            if rows.size:
                bad.append(f"{k}: {rows.size} of {x.size} 64-word rows differ, first at word {64 * rows[0]}; runs of rows {_runs(rows)[:6]}")
        elif not np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)):
            bad.append(f"{k}: differs in bits ({int((x != y).sum())} of {x.size} entries)")
    return bad


@pytest.mark.parametrize("tag", [t for t, _, _ in CHILDREN if t != "default"])
def test_form_gives_the_default_forms_bits_in_every_row(children, tag):
    base, run = children["default"], children[tag]
    bad = {}
    for cid in IDS:
        d = _diff(tag, cid, _case(base, cid), _case(run, cid))
        if d:
            bad[cid] = d
    assert not bad, f"{tag} differs from the default forms:\n" + "\n".join(f"  {c}: {d}" for c, d in bad.items())


@pytest.mark.parametrize("tag", [t for t, _, _ in CHILDREN])
def test_guards_are_intact_and_no_pattern_reaches_a_result(children, tag):
    run = children[tag]
    for cid in IDS:
        r = _case(run, cid)
        need = int(r["fused/need"])
        for path in ("fused", "auto"):
            assert bool(r[path + "/guard"]), f"{tag} {cid} {path}: the guard rows behind the workspace were written"
            assert (r[path + "/pat"][:need // G.FP_WORDS] < G.FP_WORDS).any(), f"{tag} {cid} {path}: nothing was written"
        for k in RESULTS:
            if k != "infer/rank":
                v = np.ascontiguousarray(r[k])
                assert not np.isnan(v).any() and not (v.view(np.uint32) == G.PATTERN).any(), (tag, cid, k)


def test_children_ran_the_forms_they_are_named_for(children):
    """Where the launch names tell the forms apart: the split embeddings."""
    for cid in IDS:
        c = R.case(cid)
        l = R.launches(c["C"], c["V"], c["K"], "fused")[0]
        for path in ("fused", "auto", "nograd"):
            want = "k_embed_fwd_split" if R.form_of(l)["split"] else "k_embed_fwd"
            for tag in ("default", "product", "plain", "waves4", "waves8", "emb256", "emb509"):
                got = _launches(_case(children[tag], cid), path)
                assert want in got and ({"k_embed_fwd_split", "k_embed_fwd"} - {want}).isdisjoint(got), (tag, cid, path)
            got = _launches(_case(children["split0"], cid), path)
            assert "k_embed_fwd" in got and "k_embed_fwd_split" not in got, (cid, path)
            got = _launches(_case(children["splitall"], cid), path)
            assert "k_embed_fwd_split" in got and "k_embed_fwd" not in got, (cid, path)
        names = _launches(_case(children["product"], cid), "fused")
        assert "k_conv_bwd" in names and "k_tail_bwd" in names and any(n.startswith("k_conv_turn") for n in names), (cid, names)


# ---- the anchor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_seam_case_matches_the_fp64_oracle(children, model, oracle, cid):
    r = _case(children["product"], cid)
    state, y, want, want_loss, want_grads = oracle(cid)
    for key in ("nograd/scores", "infer/scores", "fused/scores", "auto/scores"):
        err = float(np.abs(r[key] - want).max()) if want.size else 0.0
        print(f"\n{cid} {key}: largest error {err:.2e}")
        np.testing.assert_allclose(r[key], want, rtol=1e-4, atol=1e-4, err_msg=f"{cid} {key}")
    q = r["infer/scores"]
    assert list(r["infer/rank"]) == sorted(range(len(q)), key=lambda i: q[i], reverse=True)
    if FUSED_INFER(R.case(cid)):
        assert np.array_equal(q.view(np.uint32), r["nograd/scores"].view(np.uint32)), "score_state differs from the no-grad forward in bits"
    for key in ("fused/loss", "auto/loss"):
        got = float(np.asarray(r[key]).reshape(-1)[0])
        print(f"{cid} {key}: {got!r} against {want_loss!r}")
        assert abs(got - want_loss) <= 1e-4 * max(1.0, abs(want_loss)), (cid, key)
    for key in ("fused/grads", "auto/grads"):
        got = _grads(r[key])
        worst = max(float(np.abs(got[n].astype(np.float64) - want_grads[n]).max()) / max(float(np.abs(want_grads[n]).max()), 1e-6) for n in gradparity.NAMES)
        print(f"{cid} {key}: largest distance / largest entry over the 46 tensors {worst:.2e}")
        flips = gradparity.check(got, model[1], state, y, BOUND, want64=want_grads)
        if flips:
            print(f"{cid} {key}: gradients match the fp64 oracle with ReLU units {flips} flipped")
    ga, gf = r["auto/grads"], r["fused/grads"]
    np.testing.assert_allclose(gf, ga, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ga).max())))


# ---- the same case twice; group twins -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def again(model, targets):
    """The fused step of every case once more, in this process (product library)."""
    m, _ = model
    out = {}
    for cid in IDS:
        state, y = R.build(R.case(cid))[0], targets[cid]
        res, _, need, ws = G.run_step(m, state, y, download=False)
        res["fp"], res["pat"] = G.fingerprint(ws, need + G.GUARD)
        assert _guard_intact(ws, need), cid
        del ws
        m._ws_pool.clear()
        out[cid] = res
    return out


@pytest.mark.parametrize("cid", IDS)
def test_the_same_case_twice_gives_the_same_bytes(children, again, cid):
    r, a = _case(children["product"], cid), again[cid]
    for k in ("loss", "scores", "grads", "fp", "pat"):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(r["fused/" + k]).view(np.uint8)), (cid, k)


_TROUBLE = []      # a group test that raised: the ones after it do not touch the GPU


@pytest.mark.parametrize("cid", GROUPED)
def test_group_member_gives_the_bytes_of_the_solo_step(again, targets, cid):
    """The seam case as the second of two members: the group twins of the row programs get their share of the grid at a block offset."""
    assert not _TROUBLE, f"not run: {_TROUBLE[0]} failed before"
    try:
        _group_member(again, targets, cid)
    except BaseException:
        _TROUBLE.append(cid)
        raise


def _group_member(again, targets, cid):
    from gcnn_cut_selector_amd.trainer import TrainState, train_step, train_step_group
    dev = torch.device("cuda", 0)
    ms = [make_model(11, dev)[0] for _ in range(2)]
    small, ys = G.make_state(50, 60, 20, seed=7)
    state, y = R.build(R.case(cid))[0], targets[cid]
    batches = [ms[0].prepare(small), ms[1].prepare(state)]
    yt = [torch.as_tensor(v, dtype=torch.float32).to(dev) for v in (ys, y)]
    solo = TrainState(ms[0])
    loss0, scores0 = train_step(ms[0], batches[0], yt[0], None, solo)
    torch.cuda.synchronize()
    want0 = (solo.grads.cpu().numpy().copy(), float(loss0), scores0.cpu().numpy().copy())
    ts = [TrainState(m) for m in ms]
    out = train_step_group(ms, batches, yt, [None, None], ts)
    torch.cuda.synchronize()
    assert np.array_equal(ts[0].grads.cpu().numpy().view(np.uint32), want0[0].view(np.uint32)) and float(out[0][0]) == want0[1]
    assert np.array_equal(out[0][1].cpu().numpy().view(np.uint32), want0[2].view(np.uint32))
    a = again[cid]
    assert np.array_equal(ts[1].grads.cpu().numpy().view(np.uint32), a["grads"].view(np.uint32)), cid
    assert np.float32(float(out[1][0])).view(np.uint32) == np.float32(a["loss"].reshape(-1)[0]).view(np.uint32), cid
    assert np.array_equal(out[1][1].cpu().numpy().view(np.uint32), a["scores"].view(np.uint32)), cid
