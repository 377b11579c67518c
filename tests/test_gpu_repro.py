"""Same inputs => same bits, whether or not the longest segment of each CSR order is known (GPU).

`BipartiteGraph` learns the longest segment of each order through a pinned mailbox that is not waited on (graph.py): until the
copy has landed, and for good if its slot is reused first, the plan says 0 = "unknown".  An edge pass that does not know the
degree runs its long-segment blocks in front of the main grid (gcnn_capi.hip, launch_edge_fwd / launch_edge_bwd_send); one that
knows no segment is long leaves them out.  Neither choice may change a bit of what a training step computes: the same batch is
built three ways -- degree known (`sync_max_degree=True`), the same plan with both degrees 0 (`from_plan(..., 0, 0)`) and the
plain `GCNN.prepare` path -- and one fused training step with Adam from the same start must give identical scores, loss, all 46
gradients and updated parameters.

States: setcov x 32 (one, two and four lane groups per segment, no long segments; thousands of d w_edge partial rows, so the
DW_CHUNK = 128 grouping of their pre-reduction matters), capfac (hub rows beyond the long-segment threshold: long blocks run either way), a
sparse random state whose mean degrees are below 12 (one lane group per segment) with more than 128 partial rows, and a state
without edges."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gcnn_cut_selector_amd import synthetic  # noqa: E402
from oracle import gcnn_oracle as O  # noqa: E402  (checker only)
from gpucommon import dev  # noqa: E402

# mirror of the host rules in gcnn_capi.hip (edge_slots, edge_long_threshold, the send pass's grid): used only to prove that
# each state exercises what it is here for
EDGE_MAX_GRID = 8192


def _slots(n_own, n_edges):
    avg = n_edges / max(n_own, 1)
    return 4 if avg >= 40 else (2 if avg >= 12 else 1)


def _send_grid(n_own, n_edges):
    cdiv = lambda a, b: -(-a // b)
    slots = _slots(n_own, n_edges)
    return min(cdiv(cdiv(n_own, 4 // slots), 4), EDGE_MAX_GRID), slots


def _sparse_state(rng, C, V, K, e1, e2):
    def edges(n_left, n_e):
        if n_e == 0:
            return np.zeros((2, 0), np.int32)
        ei = np.unique(np.stack([rng.integers(0, n_left, n_e), rng.integers(0, V, n_e)]), axis=1).astype(np.int32)
        return ei[:, np.lexsort((ei[1], ei[0]))]
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    cei, kei = edges(C, e1), edges(K, e2)
    return (f(C, 4), cei, f(cei.shape[1], 1), f(V, 14), f(K, 6), kei, f(kei.shape[1], 1), C, V, K)


def _states():
    rng = np.random.default_rng(77)
    st, _, _ = synthetic.make_batch("setcov", 32)
    yield "setcov32", st
    st, _, _ = synthetic.make_batch("capfac", 2)
    yield "capfac2_hubs", st
    yield "slots1", _sparse_state(rng, 6000, 4000, 3000, 40000, 20000)
    yield "no_edges", _sparse_state(rng, 16, 16, 16, 0, 0)


STATES = dict(_states())


def _three_batches(m, state):
    from gcnn_cut_selector_amd.graph import BipartiteGraph
    from gcnn_cut_selector_amd.model import Batch
    plain = m.prepare(state)
    torch.cuda.synchronize()
    graphs = []
    for g in (plain.cons_graph, plain.cut_graph):
        # rebuild from the same device COO lists, this time waiting for the degrees
        ei = torch.stack([torch.repeat_interleave(torch.arange(g.n_left, device=g.device, dtype=torch.int32),
                                                  (g.l_ptr[1:] - g.l_ptr[:-1]).long()), g.l_oth]).to(torch.int32)
        known = BipartiteGraph(ei.contiguous(), g.l_coef.clone(), g.n_left, g.n_var, sync_max_degree=True)
        unknown = BipartiteGraph.from_plan(known.n_left, known.n_var, known.l_ptr, known.l_oth, known.l_coef, known.v_ptr,
                                           known.v_oth, known.v_coef, 0, 0)
        graphs.append((known, unknown))
    mk = lambda i: Batch(plain.cons_feats, plain.var_feats, plain.cut_feats, graphs[0][i], graphs[1][i])
    return {"known": mk(0), "unknown": mk(1), "prepare": plain}


def _step(m, params, batch, y, dev):
    from gcnn_cut_selector_amd.trainer import Adam, TrainState, train_step
    m.set_weights([params[n] for n in O.PARAM_NAMES])
    ts = TrainState(m)
    opt = Adam(learning_rate=1e-3)
    loss, scores = train_step(m, batch, torch.as_tensor(y, dtype=torch.float32).to(dev), opt, ts)
    torch.cuda.synchronize()
    return dict(scores=scores.clone(), loss=loss.clone(), grads=ts.grads.clone(), params=m.flat_parameters.detach().clone())


@pytest.mark.parametrize("name", list(STATES))
def test_step_bits_do_not_depend_on_known_max_degree(dev, name):
    from gcnn_cut_selector_amd.model import GCNN
    state = STATES[name]
    params = O.randomize_params(O.init_params(31, np.float32), 32)
    m = GCNN(device=dev)
    batches = _three_batches(m, state)
    known = batches["known"]
    # the state exercises what it is listed for
    C, V, K, E1, E2 = (known.dims.n_cons, known.dims.n_vars, known.dims.n_cuts, known.dims.n_cons_edges,
                       known.dims.n_cut_edges)
    sends = [(V, E1, known.cons_graph.v_max_deg), (C, E1, known.cons_graph.l_max_deg), (V, E2, known.cut_graph.v_max_deg)]
    info = [(_send_grid(n, e), md) for n, e, md in sends if n > 0 and e > 0]
    if name == "setcov32":
        assert all(s == 4 or md <= 32 * s for (_, s), md in info), info    # no long segment once the degree is known ...
        assert any(s < 4 and gr > 128 for (gr, s), _ in info), info         # ... but long blocks when it is not
    elif name == "capfac2_hubs":
        assert any(s < 4 and md > 32 * s for (_, s), md in info), info       # long blocks run, known or not
    elif name == "slots1":
        assert all(s == 1 for (_, s), _ in info) and max(gr for (gr, _), _ in info) > 128, info
    else:
        assert E1 == E2 == 0
    y = np.random.default_rng(5).uniform(0, 0.2, K)
    got = {k: _step(m, params, b, y, dev) for k, b in batches.items()}
    names = [n for n, _, t in O.PARAM_SPEC if t]
    for way in ("unknown", "prepare"):
        diff = []
        for key in ("scores", "loss", "params"):
            if not torch.equal(got[way][key], got["known"][key]):
                diff.append(key)
        ga, gb = m.gradients(got["known"]["grads"]), m.gradients(got[way]["grads"])
        diff += [f"grad {n}" for n, a, b in zip(names, ga, gb) if not torch.equal(a, b)]
        assert not diff, f"{name}: degree {way} vs known differs in {diff}"
