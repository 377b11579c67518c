"""The index pass of the two unions is one body (ib_unpack_body, k_ibatch.hpp) in two instantiations: k_ib_unpack without models,
k_mb_unpack with them.  With ONE model whose first state is 0 they must write the same plan and the calls the same download
(GPU): `_ModelsSession.last_plan()[0]` of a one-model call against `_BatchSession.last_plan()` of the same states array by array,
and scores, order, n_kept and flags bit for bit -- at the smallest shapes where the two can disagree: a state boundary, a closing
entry, an order flag (a cut-edge list that travels unsorted because a row id in its middle is out of range)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import plancases as P  # noqa: E402
from gcnn_cut_selector_amd import _lib  # noqa: E402
from gcnn_cut_selector_amd.infer import _BatchSession, _ModelsSession  # noqa: E402
from gpucommon import dev, make_model  # noqa: E402,F401

PLAN = ("l_ptr0", "l_ptr1", "left", "var0", "var1", "v_ptr", "v_oth", "v_coef")


def _states(S, unsorted):
    states = [P.random_state(70 + s, 5, 6, 3, 7, 4) for s in range(S)]
    if unsorted:
        c, cei, cef, v, k, kei, kef, nc, nv, nk = states[-1]
        kei = kei.copy()
        # a row id past the state's 3 cuts in the middle: the list is not sorted (2 follows 7) and is packed as it is.  These
        # rows give every by-left entry exactly one writer (positions 1 and 2 write entries 1 and 2, the others none), so the
        # flagged state's plan does not depend on which of two racing stores lands last.
        kei[0] = [0, 1, 7, 2]
        states[-1] = (c, cei, cef, v, k, kei, kef, nc, nv, nk)
    return states


def _download(sess, L, S, mode):
    """The written parts of the download as bytes: scores | order | n_kept (selection) | flags."""
    out, off, K = sess.out_np, list(L.out_off), L.total.n_cuts
    parts = [out[off[0]:off[0] + 4 * K], out[off[1]:off[1] + 4 * K], out[off[3]:off[3] + 16 * S]]
    if mode == _lib.IBATCH_SELECT:
        parts.append(out[off[2]:off[2] + 4 * S])
    return [p.tobytes() for p in parts]


@pytest.mark.parametrize("S,unsorted", [(1, False), (1, True), (3, True)])
def test_one_model_union_is_the_batch_union(dev, S, unsorted):
    m, _ = make_model(311, dev)
    states = _states(S, unsorted)
    sess = m._sess("_batch_session", _BatchSession)
    models = _ModelsSession(sess)
    for mode in (_lib.IBATCH_RANK, _lib.IBATCH_SELECT):
        checked = [m._admit_state(st, mode) for st in states]
        want = sess.run(checked, None, mode, 0.1, 0.5)
        want_plan, want_out = sess.last_plan(), _download(sess, sess.last[0], S, mode)
        got = models.run(checked, None, mode, [0] * S, [m], 0.1, 0.5)
        got_plan, got_out = models.last_plan(), _download(sess, models.last[0].u, S, mode)
        assert len(got_plan) == 1 and [r[0] for r in got] == [r[0] for r in want] == ["ok"] * (S - unsorted) + ["bad_index"] * unsorted
        for name in PLAN:
            assert want_plan[name].size and want_plan[name].tobytes() == got_plan[0][name].tobytes(), (mode, name)
        assert got_out == want_out, mode
        flags = np.frombuffer(want_out[2], np.int32).reshape(S, 4)
        assert flags.tolist() == [[0, 0, 0, 0]] * (S - unsorted) + [[1, 0, 1, 0]] * unsorted
        for a, b in zip(want, got):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
