"""The register-lean forms of the edge passes (k_edge_fwd / k_edge_bwd_send without the long-row body, csrc/k_edge.hpp) on the smallest
graphs at which a rework of the full-step / masked-step split can go wrong (GPU, bit for bit).

One graph per lane-group width SLOTS in {1, 2, 4}.  Its crafted (left) rows have 0, 1, STEP - 1, STEP, STEP + 1, 16 SLOTS and
16 SLOTS + 1 edges for both steps (STEP = EDGE_U SLOTS in the forward, EDGE_UB SLOTS in the sender pass) and filler rows that bring
the mean degree into the class of SLOTS; at most 64 left rows, 40 rows on the gathered side.  The counting forward walks the left
rows with recv_is_left=True, the sender pass with recv_is_left=False.  Values lie on the dyadic grid of tests/edgecases.py (coef k/4,
w k/4, tables and dS small integers, s1 = +-0.5), so every sum is exact in fp32 in any order and the expectation is integer
arithmetic: S, N, dP_send and the summed partial rows of d w_edge must be `torch.equal` to it.  Which edge is added how often comes
from the restatement of the walk in tests/edgecases.py (`multiplicity` under the restated launch plan): once each."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edgecases as X  # noqa: E402
from gpucommon import dev  # noqa: E402,F401

N_VAR = 40
FILL = {1: (), 2: (24,) * 4, 4: (60,) * 12}      # filler rows: mean degree 6 / 14.1 / 41.9, below the block-per-segment rule (48)


def _graph(S):
    F, B, G = X.EDGE_U * S, X.EDGE_UB * S, 16 * S
    lens = np.asarray(sorted({0, 1, F - 1, F, F + 1, B - 1, B, B + 1, G, G + 1}) + list(FILL[S]), np.int64)
    rng = np.random.default_rng(100 + S)
    lens = lens[rng.permutation(lens.size)]
    n_left, E = lens.size, int(lens.sum())
    assert n_left <= 64 and X.edge_slots(n_left, E) == S and lens.max() <= X.long_threshold(S)
    l_ptr = np.zeros(n_left + 1, np.int64)
    np.cumsum(lens, out=l_ptr[1:])
    el, ev = np.repeat(np.arange(n_left), lens), rng.integers(0, N_VAR, E)
    pv = np.argsort(ev, kind="stable")
    v_ptr = np.zeros(N_VAR + 1, np.int64)
    np.cumsum(np.bincount(ev, minlength=N_VAR), out=v_ptr[1:])
    q = rng.integers(-6, 3, E)                      # coef = q / 4, c = (coef + 0.5) * 2 = (q + 2) / 2
    w4 = rng.integers(-8, 9, X.EMB)
    ints = lambda lo, hi, n: rng.integers(lo, hi + 1, (n, X.EMB))
    return dict(S=S, n_left=n_left, E=E, lens=lens, l_ptr=l_ptr, el=el, ev=ev, pv=pv, v_ptr=v_ptr, q=q, w4=w4, PL=ints(-4, 4, n_left),
                PR=ints(-4, 4, N_VAR), dS_l=ints(-2, 2, n_left), dS_v=ints(-2, 2, N_VAR))


def _expected(g, s1):
    """Integer arithmetic: the forward over the left rows (S, N) and the sender pass over the left rows (dP_send, d w_edge), every
    edge weighted by how often the restated walk adds it."""
    md = int(g["lens"].max())
    fplan, splan = X.fwd_plan(g["n_left"], g["E"], md, True), X.send_plan(g["n_left"], g["E"], md)
    for plan in (fplan, splan):
        assert plan["kind"] == "main" and plan["slots"] == g["S"] and plan["lb"] == 0, plan
    mf, mb = X.multiplicity(g["l_ptr"], fplan, X.EDGE_U), X.multiplicity(g["l_ptr"], splan, X.EDGE_UB)
    assert (mf == 1).all() and (mb == 1).all()
    c2 = (g["q"] + 2)[:, None]
    J8 = c2 * g["w4"][None, :] + 8 * g["PL"][g["el"]] + 8 * g["PR"][g["ev"]]
    act = (J8 > 0) if s1 > 0 else (J8 < 0)
    A, N, T = (np.zeros((g["n_left"], X.EMB), np.int64) for _ in range(3))
    X._seg_add(A, g["el"], J8 * act * mf[:, None])
    X._seg_add(N, g["el"], act * mf[:, None])
    t = g["dS_v"][g["ev"]] * act * mb[:, None]      # left rows send: dS is the variable side's
    X._seg_add(T, g["el"], t)
    f32 = np.float32
    return dict(S=A.astype(f32) * f32(s1 / 8), N=N.astype(f32), d_send=T.astype(f32) * f32(s1),
                d_w=(c2 * t).sum(0).astype(f32) * f32(s1 / 2), names=[fplan["name"], splan["name"]])


def _up(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


@pytest.mark.parametrize("S", (1, 2, 4))
def test_lean_edge_forms_at_the_step_seams(dev, S):
    from gcnn_cut_selector_amd import _lib, ops
    from gcnn_cut_selector_amd.graph import BipartiteGraph
    g = _graph(S)
    coef = (g["q"] / 4).astype(np.float32)
    assert np.array_equal((coef + np.float32(X.E_SHIFT)) * np.float32(X.E_SCALE) * 2, g["q"] + 2)
    i32 = lambda a: _up(a, dev, np.int32)
    graph = BipartiteGraph.from_plan(g["n_left"], N_VAR, i32(g["l_ptr"]), i32(g["ev"]), _up(coef, dev), i32(g["v_ptr"]), i32(g["el"][g["pv"]]),
                                     _up(coef[g["pv"]], dev), int(g["lens"].max()), int(np.diff(g["v_ptr"]).max()))
    PL, PR, w = _up(g["PL"], dev), _up(g["PR"], dev), _up(g["w4"] / 4, dev)
    esh, esc = _up([X.E_SHIFT], dev), _up([X.E_SCALE], dev)
    for s1 in X.S1:
        want = _expected(g, s1)
        args = (PL, PR, w, esh, esc, _up([s1], dev))
        _, N_v = ops.conv_edge_fwd(graph, False, *args, save=True)     # the variable rows' counts: conv_edge_bwd wants them, nothing here reads its d_PR
        with _lib.launch_profile() as p:
            S_l, N_l = ops.conv_edge_fwd(graph, True, *args, save=True)                  # the left rows receive
            d_pl, _, d_w = ops.conv_edge_bwd(graph, False, N_v, *args, _up(g["dS_v"], dev))   # the left rows send
            torch.cuda.synchronize()
        names = [n for n, _ in p.launches if n.startswith(("k_edge_fwd", "k_edge_bwd_send"))]
        assert names == want["names"], names
        for key, got in (("S", S_l), ("N", N_l), ("d_send", d_pl), ("d_w", d_w)):
            got, ref = got.cpu(), torch.from_numpy(want[key])
            assert torch.equal(got, ref), (S, s1, key, torch.nonzero((got != ref).reshape(-1, X.EMB).any(-1)).flatten().tolist(),
                                           g["lens"].tolist())
