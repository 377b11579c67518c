"""The edge passes (k_edge_fwd, k_edge_fwd_block, the long-row blocks, k_edge_bwd_send) at every lane-group, step and long-row seam,
and the standalone scatter-sum pass (GPU).

Cases, fills and their proof are in tests/edgecases.py and tests/test_edgecases.py.  Per case, both signs of s1 and both
orientations (the forward with recv_is_left=True and the backward with recv_is_left=False walk the crafted left rows; the other
two walk the variable side):

grid fill -- every value on a dyadic grid, every sum exact in fp32 in any order: S (with and without counts), N, d_PL, d_PR and
d w_edge must be `torch.equal` to the integer expectation, forced and natural ties J == 0 inactive everywhere, and the recorded
launch names must be the restated ones.  With the longest segment unknown the sender pass is also called directly: n_parts is main
blocks + long blocks, the long blocks' partial rows of d w_edge are s1 * (+0) where no row is long, and otherwise the main rows and
the tail rows sum to the expected shares of the short and the long senders.

float fill -- standard normal values: on the 256 matched pairs, where the kernels' expression is exactly 0, dP_recv and dP_send
agree bit for bit (both inactive); per channel the active edges the sender pass saw are as many as the forward counted, over every
edge of the case; S is within 3e-5 of the fp64 reference (the bound of tests/test_gpu_ops.py::test_conv_edge_fwd_bwd).

Outputs are compared on the host and their device blocks overwritten with NaN afterwards; no expected value is ever uploaded.  So the
blocks the wrappers' `torch.empty` recycles never hold a right answer, and a row that a pass skips cannot pass by what was there.

Measured on an MI355X, host expectation included (grid / float test): trip/S1 1.2 / 1.5 s, trip/S2 1.9 / 2.5 s, trip/S4 2.7 / 3.2 s,
finder2/S1 3.4 s (grid only); every other case under 0.8 s; DESIGN.md, section 4.z."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edgecases as X  # noqa: E402
from gpucommon import dev  # noqa: E402,F401

RTOL, ATOL = 3e-5, 3e-5       # tests/test_gpu_ops.py
ORIENTATIONS = (True, False)


def _up(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def upload(cid, fill, dev):
    """(graph, tables) of a case under a fill; the longest segments are the case's (0, 0 = unknown)."""
    from gcnn_cut_selector_amd.graph import BipartiteGraph
    c = X.case(cid)
    ml, mv = X.max_degs(c)
    coef = fill["coef"]
    g = BipartiteGraph.from_plan(c["n_left"], c["n_var"], _up(c["l_ptr"], dev, np.int32), _up(c["ev"], dev, np.int32), _up(coef, dev),
                                 _up(c["v_ptr"], dev, np.int32), _up(c["el"][c["pv"]], dev, np.int32), _up(coef[c["pv"]], dev), ml, mv)
    t = {k: _up(fill[k], dev) for k in ("PL", "PR", "w", "dS_l", "dS_v")}
    t["esh"], t["esc"] = _up(np.float32([X.E_SHIFT]), dev), _up(np.float32([X.E_SCALE]), dev)
    return g, t


def send_rows(g, recv_is_left, t, s1, d_s):
    """gcnn_conv_edge_bwd_send as ops.conv_edge_bwd calls it: (dP_send, the partial rows of d w_edge, n_parts)."""
    from gcnn_cut_selector_amd import _lib, ops
    from gcnn_cut_selector_amd.graph import _ptr, _stream
    sptr, soth, scoef, n_send = ops._edge_side(g, not recv_is_left)
    p_send, p_recv = (t["PR"], t["PL"]) if recv_is_left else (t["PL"], t["PR"])
    d_send = torch.empty((n_send, 64), dtype=torch.float32, device=d_s.device)
    rows = torch.full((16384, 64), float("nan"), dtype=torch.float32, device=d_s.device)
    n_parts = C.c_int32(0)
    with torch.cuda.device(d_s.device):
        _lib.check(_lib.lib().gcnn_conv_edge_bwd_send(_ptr(sptr), _ptr(soth), _ptr(scoef), n_send, g.n_edges, _ptr(p_send), _ptr(p_recv),
                                                      _ptr(t["w"]), _ptr(t["esh"]), _ptr(t["esc"]), _ptr(s1), _ptr(d_s), _ptr(d_send), _ptr(rows),
                                                      C.byref(n_parts), g.v_max_deg if recv_is_left else g.l_max_deg, _stream(d_s.device)),
                   "gcnn_conv_edge_bwd_send")
    return d_send, rows, n_parts.value


def run(g, t, s1, recv_is_left):
    """Forward with counts, forward without, backward: the outputs by name and the recorded edge-pass launch names."""
    from gcnn_cut_selector_amd import _lib, ops
    args = (t["PL"], t["PR"], t["w"], t["esh"], t["esc"], s1)
    d_s = t["dS_l"] if recv_is_left else t["dS_v"]
    with _lib.launch_profile() as p:
        S, N = ops.conv_edge_fwd(g, recv_is_left, *args, save=True)
        S_infer = ops.conv_edge_fwd(g, recv_is_left, *args)
        d_pl, d_pr, d_w = ops.conv_edge_bwd(g, recv_is_left, N, *args, d_s)
        torch.cuda.synchronize()
    d_recv, d_send = (d_pl, d_pr) if recv_is_left else (d_pr, d_pl)
    names = [n for n, _ in p.launches if n.startswith(("k_edge_fwd", "k_edge_bwd_send"))]
    return dict(S=S, S_infer=S_infer, N=N, d_recv=d_recv, d_send=d_send, d_w=d_w), names


def _restated_names(cid, recv_is_left):
    p = X.plans(X.case(cid), recv_is_left)
    return [p["fwd"]["name"], p["infer"]["name"], p["send"]["name"]]


def _download(got):
    """The outputs as host tensors; their device blocks are left holding NaN.  No expected value is ever uploaded, so what a later
    `torch.empty` of the library wrappers recycles is NaN, never a correct answer: a row that a pass leaves unwritten shows."""
    host = {k: v.detach().cpu() for k, v in got.items()}
    for v in got.values():
        v.detach().fill_(float("nan"))
    return host


def _differing(got, want, lens):
    """Where two [rows, 64] tensors differ: for the failure message."""
    if got.dim() != 2:
        return f"channels {torch.nonzero(got != want).flatten().tolist()} differ"
    rows = torch.nonzero((got != want).any(-1) | torch.isnan(got).any(-1)).flatten().numpy()
    return f"{rows.size} rows differ, first {rows[:8].tolist()} of lengths {lens[rows[:8]].tolist()}"


@pytest.mark.parametrize("cid", X.IDS)
def test_grid_fill_is_exact_to_the_bit(dev, cid):
    c = X.case(cid)
    g, t = upload(cid, X.grid_fill(cid), dev)
    for s1 in X.S1:
        s1_dev = _up(np.float32([s1]), dev)
        for recv_is_left in ORIENTATIONS:
            want = X.expected(cid, s1, recv_is_left)
            got, names = run(g, t, s1_dev, recv_is_left)
            got = _download(got)
            assert names == _restated_names(cid, recv_is_left), (cid, s1, recv_is_left, names)
            rlens, slens = np.diff(X.csr(c, recv_is_left)[0]), np.diff(X.csr(c, not recv_is_left)[0])
            for key, ref, lens in (("S", "S", rlens), ("S_infer", "S", rlens), ("N", "N", rlens), ("d_recv", "d_recv", rlens),
                                   ("d_send", "d_send", slens), ("d_w", "d_w", slens)):
                w = torch.from_numpy(want[ref])
                assert torch.equal(got[key], w), (cid, s1, recv_is_left, key, _differing(got[key], w, lens))


@pytest.mark.parametrize("cid", [i for i in X.IDS if i.startswith("unknown")])
def test_unknown_longest_segment_partial_rows(dev, cid):
    c = X.case(cid)
    g, t = upload(cid, X.grid_fill(cid), dev)
    assert g.l_max_deg == 0 and g.v_max_deg == 0
    for s1 in X.S1:
        s1_dev = _up(np.float32([s1]), dev)
        for recv_is_left in ORIENTATIONS:
            plan = X.plans(c, recv_is_left)["send"]
            want = X.expected(cid, s1, recv_is_left)
            d_send, rows, n_parts = send_rows(g, recv_is_left, t, s1_dev, t["dS_l"] if recv_is_left else t["dS_v"])
            torch.cuda.synchronize()
            host = _download(dict(d_send=d_send, rows=rows))
            d_send, rows = host["d_send"], host["rows"]
            assert plan["lb"] > 0 and n_parts == plan["grid"] + plan["lb"], (n_parts, plan)
            assert torch.isnan(rows[n_parts:]).all() and not torch.isnan(rows[:n_parts]).any()       # one row per block, none behind
            assert torch.equal(d_send, torch.from_numpy(want["d_send"]))
            main, tail = rows[:plan["grid"]].sum(0), rows[plan["grid"]:n_parts].sum(0)
            assert torch.equal(main, torch.from_numpy(want["dw_main"])) and torch.equal(tail, torch.from_numpy(want["dw_tail"])), (cid, s1, recv_is_left)
            assert torch.equal(main + tail, torch.from_numpy(want["d_w"]))
            slens = np.diff(X.csr(c, not recv_is_left)[0])
            if not (X.row_paths(slens, plan)[0] == X.LONG).any():
                # no row for the finder: every long block stores s1 * (+0), which added to the main rows' sum leaves its bits
                zero = int((np.float32(s1) * np.float32(0.0)).view(np.int32))
                assert (rows[plan["grid"]:n_parts].view(torch.int32) == zero).all(), (cid, s1, recv_is_left)
        if "seams" in cid:        # the crafted side has no long row
            assert not (X.row_paths(np.diff(c["l_ptr"]), X.plans(c, False)["send"])[0] == X.LONG).any()


@pytest.mark.parametrize("cid", X.FLOAT_IDS)
def test_float_fill_backward_sees_the_forward_relu_bits(dev, cid):
    c = X.case(cid)
    for recv_is_left in ORIENTATIONS:
        g, t = upload(cid, X.float_fill(cid, recv_is_left), dev)
        pr, pu = (c["pair_l"], c["pair_v"]) if recv_is_left else (c["pair_v"], c["pair_l"])       # receivers, their senders
        pr, pu = torch.from_numpy(pr), torch.from_numpy(pu)
        for s1 in X.S1:
            got = _download(run(g, t, _up(np.float32([s1]), dev), recv_is_left)[0])
            # 1. the planted elements: J is exactly 0 in both passes, so both gradients are s1 * 0, the same bits
            a, b = got["d_recv"][pr].view(torch.int32), got["d_send"][pu].view(torch.int32)
            assert torch.equal(a, b), (cid, s1, recv_is_left, int((a != b).sum()))
            assert (got["N"][pr] == 0).all() and (got["d_send"][pu] == 0).all()
            # 2. every edge of the case: what the sender pass treated as active is what the forward counted (dS = 1)
            per_s1 = got["d_send"].numpy().astype(np.float64) / s1
            assert np.array_equal(per_s1, np.rint(per_s1))
            seen, counted = per_s1.astype(np.int64).sum(0), got["N"].numpy().astype(np.int64).sum(0)
            assert np.array_equal(seen, counted), (cid, s1, recv_is_left, (seen - counted).tolist())
            # 3. the forward against fp64
            ref = X.reference_S(cid, s1, recv_is_left)
            scale = max(1.0, float(np.abs(ref).max()))
            for key in ("S", "S_infer"):
                np.testing.assert_allclose(got[key].numpy().astype(np.float64), ref, rtol=RTOL, atol=ATOL * scale, err_msg=f"{cid} {s1} {recv_is_left} {key}")


# ---- scatter-sum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", X.SCATTER_IDS)
@pytest.mark.parametrize("sorted_index", (True, False))
def test_scatter_sum_of_integer_messages_is_exact(dev, sid, sorted_index):
    from gcnn_cut_selector_amd import ops
    lens, idx, msg, d_out = X.scatter_case(sid)
    if not sorted_index:
        order = np.random.default_rng(1).permutation(idx.size)
        idx, msg = idx[order], msg[order]
    m = _up(msg, dev).requires_grad_()
    plan = ops.SegmentPlan(_up(idx, dev, np.int32), lens.size)
    assert plan.sorted == sorted_index
    out = ops.scatter_sum(m, plan, lens.size)
    assert torch.equal(out.detach().cpu(), torch.from_numpy(X.scatter_expected(sid)))
    out.backward(_up(d_out, dev))
    assert torch.equal(m.grad.cpu(), torch.from_numpy(d_out[idx]))        # a row gather
    out.detach().fill_(float("nan"))
    m.grad.fill_(float("nan"))
