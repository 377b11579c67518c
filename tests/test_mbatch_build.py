"""CPU checks of the call that scores states of several models at once (gcnn_infer_models) and of the server that uses it:
declared, exported and bound at ABI 13; launch names of its own file only; two kernels that cross-compile for gfx950 as wave64
without scratch or float atomics; limits returned without a device; a layout aligned as gcnn_infer_batch's; a table that equals
its NumPy restatement; a server that groups host-state requests across models."""
import ctypes as C
import os
import re
import tempfile

import numpy as np

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
MBATCH = os.path.join(CSRC, "gcnn_mbatch.hpp")
SYMBOLS = ("gcnn_infer_models_layout_for", "gcnn_infer_models_fill_table", "gcnn_infer_models")
NAMES = {"k_mb_unpack", "k_mb_by_variable", "k_mb_vptr", "k_mb_rank"}     # k_mb_rank: the record of k_ib_rank over all states
KERNELS = {"k_mb_unpack", "k_mb_vptr"}


def test_symbols_in_header_binding_and_library_abi_13():
    header = buildsupport.declared_everywhere(SYMBOLS)
    from gcnn_cut_selector_amd import _lib
    assert "gcnn_mbatch_layout" in header
    assert "#define GCNN_MBATCH_TABLE_WORDS (GCNN_IBATCH_TABLE_COLS * GCNN_IBATCH_TABLE_STRIDE + 16 + GCNN_IBATCH_MAX)\n" in header
    assert _lib.MBATCH_TABLE_WORDS == 7 * 72 + 16 + 64 and _lib.MBATCH_HEAD == 16


def test_launch_names_are_its_own():
    names = launchnames.launch_names(MBATCH)
    assert names == NAMES
    assert len(launchnames.launch_names()) == 28 and not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_mbatch.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_mbatch.hpp", "gcnn_select.hpp", "gcnn_group.hpp", "gcnn_ibatch.hpp")
    # the forward passes go out under the group kernels' names: this file spells none of them
    assert "k_group_" not in re.sub(r"//[^\n]*", "", open(MBATCH).read())


def test_kernels_compile_wave64_without_scratch_or_float_atomics():
    build = buildsupport.device_build()
    new = {k: v for k, v in build.rows.items() if "k_mb_" in k}
    assert len(new) == 2 and all(any(n in k for k in new) for n in KERNELS), sorted(new)
    for name, v in new.items():
        assert v["scratch"] == 0 and v["lds"] <= 64 * 1024, (name, v)
        assert not re.search(r"atomic_(add|pk_add)_f(16|32|64)", build.body(name)), name
        assert build.wavefront_size(name) == 64, name
    # the families the other build tests count are as they were
    rows = list(build.rows)
    assert sum("k_ib_" in r for r in rows) == 2 and sum("k_sel_" in r for r in rows) == 2 and sum("k_group_" in r for r in rows) == 35


ONE = (5, 6, 3, 7, 4)


def _layout(shapes, model_of, n_models=None, forced=None, mode=0):
    from gcnn_cut_selector_amd import _lib
    n = len(shapes)
    dims = (_lib.Dims * max(n, 1))(*(_lib.Dims(*s) for s in shapes))
    nf = (C.c_int32 * max(n, 1))(*(f[0] for f in forced)) if forced else None
    nfe = (C.c_int32 * max(n, 1))(*(f[1] for f in forced)) if forced else None
    mos = (C.c_int32 * max(len(model_of), 1))(*model_of)
    M = (max(model_of) + 1 if model_of else 1) if n_models is None else n_models
    L = _lib.MbatchLayout()
    rc = _lib.lib().gcnn_infer_models_layout_for(n, dims, nf, nfe, mode, M, mos, C.byref(L))
    return rc, L, (dims, nf, nfe, mos, M)


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    # n_states outside 1..64, n_models outside 1..8
    assert _layout([], [])[0] == -1 and _layout([ONE] * 65, [0] * 65)[0] == -1 and _layout([ONE] * 64, [0] * 64)[0] == 0
    assert _layout([ONE], [0], n_models=0)[0] == -1 and _layout([ONE] * 9, list(range(9)))[0] == -1
    assert _layout([ONE] * 8, list(range(8)))[0] == 0
    assert _layout([ONE], [0], mode=3)[0] == -1 and _layout([ONE, (5, 5, -1, 5, 5)], [0, 0])[0] == -1
    # a decreasing model_of_state, an index >= n_models, a negative one
    assert _layout([ONE] * 3, [0, 1, 0])[0] == -1
    assert _layout([ONE] * 2, [0, 2], n_models=2)[0] == -1 and _layout([ONE] * 2, [-1, 0], n_models=2)[0] == -1
    # a model without any state is REFUSED: in front, in the middle, at the end
    assert _layout([ONE] * 2, [1, 1], n_models=2)[0] == -1
    assert _layout([ONE] * 2, [0, 2], n_models=3)[0] == -1
    assert _layout([ONE] * 2, [0, 0], n_models=2)[0] == -1
    d, nf, nfe, mos, M = _layout([ONE], [0])[2]
    assert lib.gcnn_infer_models_layout_for(1, d, None, None, 0, 1, None, C.byref(_lib.MbatchLayout())) == -1
    assert lib.gcnn_infer_models_layout_for(1, d, None, None, 0, 1, mos, None) == -1
    # unions past 2^24 rows or 2^30 edges; edges with nothing to point at; forced entries without a row
    assert _layout([((1 << 23) + 1, 5, 5, 5, 5)] * 2, [0, 1])[0] == -4
    assert _layout([(5, 5, 5, 1 << 29, 5)] * 3, [0, 0, 1])[0] == -4
    assert _layout([ONE, (0, 5, 5, 3, 5)], [0, 1])[0] == -4 and _layout([ONE, (5, 0, 5, 0, 2)], [0, 1])[0] == -4
    assert _layout([ONE, ONE], [0, 1], forced=[(0, 0), (0, 3)], mode=2)[0] == -1
    assert _layout([ONE, (0, 0, 0, 0, 0), (5, 5, 4097, 5, 5)], [0, 0, 1], mode=1)[0] == 0   # riders as in gcnn_infer_batch
    # the call itself: thresholds that are not finite, a short or misaligned arena, missing buffers -- before anything is enqueued
    rc, L, (d, nf, nfe, mos, M) = _layout([ONE, ONE], [0, 1], mode=2)
    assert rc == 0
    fake = 1 << 20
    params = (C.c_void_p * 2)(fake, fake)

    def call(p_max=0.1, arena=fake * 256, size=L.u.arena_bytes, par=params, host_in=fake, host_out=fake, staging=fake, mos=mos, M=2):
        return lib.gcnn_infer_models(2, d, None, None, 2, M, mos, par, host_in, host_out, arena, size, staging, p_max, 0.5, None)

    assert call(p_max=float("nan")) == -1 and call(p_max=float("inf")) == -1
    assert call(size=L.u.arena_bytes - 1) == -1 and call(arena=fake * 256 + 16) == -1
    assert call(par=None) == -1 and call(par=(C.c_void_p * 2)(fake, None)) == -1
    assert call(host_in=None) == -1 and call(host_out=None) == -1 and call(staging=None) == -1
    assert call(mos=(C.c_int32 * 2)(1, 0)) == -1 and call(M=9) == -1
    assert lib.gcnn_infer_models_fill_table(2, d, None, None, 2, mos, None) == -1
    assert lib.gcnn_infer_models_fill_table(2, d, None, None, 2, (C.c_int32 * 2)(1, 0), (C.c_int32 * _lib.MBATCH_TABLE_WORDS)()) == -1


def _batch_layout(shapes, forced, mode):
    from gcnn_cut_selector_amd import _lib
    n = len(shapes)
    dims = (_lib.Dims * n)(*(_lib.Dims(*s) for s in shapes))
    nf, nfe = (C.c_int32 * n)(*(f[0] for f in forced)), (C.c_int32 * n)(*(f[1] for f in forced))
    L = _lib.IbatchLayout()
    return _lib.lib().gcnn_infer_batch_layout_for(n, dims, nf, nfe, mode, C.byref(L)), L


SHAPES = [(50, 100, 10, 400, 90), (7, 9, 1, 0, 3), (20, 30, 4, 0, 11), (500, 1000, 100, 25000, 9000), (3, 4, 2, 5, 6), (9, 8, 7, 6, 5)]
MODEL_OF = [0, 1, 1, 1, 2, 2]            # models of 1, 3 and 2 states; states 1 and 2 have no constraint edges
FORCED = [(0, 0), (1, 5), (0, 0), (40, 800), (2, 2), (0, 0)]


def test_layout_is_aligned_as_the_batch_layout_and_holds_every_block():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    al16 = lambda x: (x + 15) & ~15  # noqa: E731
    for mode in (0, 1, 2):
        rc, ML, (dims, nf, nfe, mos, M) = _layout(SHAPES, MODEL_OF, forced=FORCED, mode=mode)
        assert rc == 0 and M == 3
        L = ML.u
        in_off, out_off, dev_off = list(L.in_off), list(L.out_off), list(L.dev_off)
        assert all(o % 16 == 0 for o in in_off + out_off) and all(o % 256 == 0 for o in dev_off + [ML.table_off, L.arena_bytes])
        assert in_off == sorted(in_off) and in_off[0] == 0 and L.in_bytes >= in_off[-1] and L.in_bytes % 16 == 0
        assert out_off == sorted(out_off) and L.out_bytes == out_off[3] + 16 * len(SHAPES)
        assert dev_off == sorted(dev_off) and dev_off[0] >= L.in_bytes
        tot = L.total
        sums = tuple(sum(s[i] for s in SHAPES) for i in range(5))
        assert (tot.n_cons, tot.n_vars, tot.n_cuts, tot.n_cons_edges, tot.n_cut_edges) == sums
        assert (L.n_forced, L.n_forced_entries) == ((43, 807) if mode == 2 else (0, 0)) and L.max_cuts == 100 and L.n_states == 6
        C_, V, K, E1, E2 = sums
        # the table with its model words; the zero block with one closing by-left offset per model (+ the union's cut offsets)
        assert in_off[1] - in_off[0] >= 4 * _lib.MBATCH_TABLE_WORDS
        zero = al16(16 * 6) + al16(4 * (C_ + M)) + al16(4 * (K + M)) + (al16(4 * (K + 1)) if mode == 2 else 0)
        assert in_off[2] - in_off[1] == zero
        # the seven arrays lie where gcnn_infer_batch keeps them relative to in_off[2]
        rc, IL = _batch_layout(SHAPES, FORCED, mode)
        assert rc == 0 and [o - in_off[2] for o in in_off[2:]] == [o - IL.in_off[2] for o in list(IL.in_off)[2:]]
        assert list(IL.out_off) == out_off and IL.out_bytes == L.out_bytes
        # the per-model v_ptr, the sort keys and the union's v_ptr; the models' workspaces and the launch tables inside the arena
        assert dev_off[7] - dev_off[6] >= 4 * (V + M) and dev_off[15] - dev_off[14] >= 4 * E1
        assert ML.n_models == 3 and list(ML.first_state)[:4] == [0, 1, 4, 6]
        end = dev_off[12]
        for m in range(3):
            mine = [s for s, k in zip(SHAPES, MODEL_OF) if k == m]
            dm = ML.model[m]
            assert (dm.n_cons, dm.n_vars, dm.n_cuts, dm.n_cons_edges, dm.n_cut_edges) == tuple(sum(s[i] for s in mine) for i in range(5))
            assert ML.ws_off[m] % 256 == 0 and ML.ws_off[m] >= end
            end = ML.ws_off[m] + 4 * lib.gcnn_workspace_floats(C.byref(dm))
        assert end <= dev_off[13]
        size = C.c_size_t()
        assert lib.gcnn_group_table_bytes(3, C.byref(size)) == 0 and ML.table_bytes == size.value
        assert ML.table_off >= dev_off[15] + 4 * (V + 1) and ML.table_off + ML.table_bytes <= L.arena_bytes


def test_table_equals_its_restatement():
    from gcnn_cut_selector_amd import _lib
    rc, ML, (dims, nf, nfe, mos, M) = _layout(SHAPES, MODEL_OF, forced=FORCED, mode=2)
    assert rc == 0
    table = np.full(_lib.MBATCH_TABLE_WORDS, -1, np.int32)
    assert _lib.lib().gcnn_infer_models_fill_table(6, dims, nf, nfe, 3, mos, table.ctypes.data) == 0
    cols, stride, head = _lib.IBATCH_TABLE_COLS, _lib.IBATCH_TABLE_STRIDE, _lib.MBATCH_HEAD
    t = table[:cols * stride].reshape(cols, stride)
    want = np.cumsum([[0] * 7] + [list(s) + list(f) for s, f in zip(SHAPES, FORCED)], axis=0).T
    assert np.array_equal(t[:, :7], want)
    mod = table[cols * stride:]
    restated = np.zeros(head + _lib.IBATCH_MAX, np.int32)
    restated[0] = 3
    restated[1:5] = [0, 1, 4, 6]                      # np.searchsorted(MODEL_OF, m) for m = 0..3
    assert restated[1:5].tolist() == np.searchsorted(MODEL_OF, np.arange(4)).tolist()
    restated[head:head + 6] = MODEL_OF
    assert np.array_equal(mod, restated)


class _StubModel:
    device = "stub"

    def __init__(self, log, name):
        self.log, self.name = log, name

    def score_states(self, states, rank=False, return_exceptions=False):
        self.log.append(("model", self.name, len(states)))
        return [np.zeros(1, np.float32) for _ in states]

    def select_cuts_many(self, *args, **kwargs):                   # (the server looks a kind's pair of methods up together)
        raise AssertionError("not asked for")


class _StubSet:
    def __init__(self, log):
        self.log = log

    def score_states(self, keys, states, rank=False, return_exceptions=False):
        self.log.append(("set", tuple(keys), len(states)))
        return [np.zeros(1, np.float32) for _ in states]

    select_cuts_many = _StubModel.select_cuts_many


def _served(cross, keys, devices=None, model_set=True):
    """(calls made, stats) of one sweep over one KIND_SCORE request per key."""
    from gcnn_cut_selector_amd import serve, synthetic, utils
    state = utils.state_to_inputs(synthetic.make_sample("setcov", 1, scale=0.2)[0])
    log = []
    models = {k: _StubModel(log, k) for k in "abc"}
    for k, d in (devices or {}).items():
        models[k].device = d
    with tempfile.TemporaryDirectory() as tmp:
        server = serve.ScoringServer(models, os.path.join(tmp, "s.sock"), cross_model=cross, model_set=_StubSet(log) if model_set else None)
        try:
            pending = [(None, serve.decode_request(serve.encode_request(k, serve.KIND_SCORE, state))) for k in keys]
            server._serve(pending)          # (no connection is registered: the replies are dropped, the calls are what counts)
        finally:
            server.close()
    return log, server.stats


def test_server_groups_host_states_across_models():
    from gcnn_cut_selector_amd import serve
    log, stats = _served(True, "abc")
    assert log == [("set", ("a", "b", "c"), 3)] and stats["calls"] == 1 and stats["max_models_per_call"] == 3
    log, stats = _served(False, "abc")
    assert log == [("model", "a", 1), ("model", "b", 1), ("model", "c", 1)] and stats["calls"] == 3 and stats["max_models_per_call"] == 1
    # requests of ONE model take that model's own call (the faster one for them), whatever the grouping
    log, stats = _served(True, "bbb")
    assert log == [("model", "b", 3)] and stats["calls"] == 1 and stats["max_models_per_call"] == 1
    # the stat is what the set reports for its calls, not the number of keys in the group
    class Splitting(_StubSet):
        max_models_per_call = 2
    from gcnn_cut_selector_amd import synthetic, utils
    state = utils.state_to_inputs(synthetic.make_sample("setcov", 1, scale=0.2)[0])
    with tempfile.TemporaryDirectory() as tmp:
        log = []
        server = serve.ScoringServer({k: _StubModel(log, k) for k in "abc"}, os.path.join(tmp, "s.sock"), model_set=Splitting(log))
        try:
            server._serve([(None, serve.decode_request(serve.encode_request(k, serve.KIND_SCORE, state))) for k in "abc"])
        finally:
            server.close()
    assert server.stats["max_models_per_call"] == 2
    # models on more than one device cannot share a ModelSet: they are served per model, as before
    log, stats = _served(True, "abc", devices={"c": "elsewhere"}, model_set=False)
    assert log == [("model", "a", 1), ("model", "b", 1), ("model", "c", 1)] and stats["max_models_per_call"] == 1
    assert serve.ScoringServer.__init__.__defaults__[1] is True     # cross_model: (a) is 2.3x faster than (b) at M = 5


class _FallbackModel:
    """What `ModelSet` needs of a model when the grouped call declines: a device, `_many` and the solo entry point."""
    device = "stub"

    def __init__(self, name, log):
        self.name, self.log = name, log

    def _many(self, states, mode, solo, forced=None, p_max=0.0, p_max_ub=0.0):
        self.log.append((self.name, [int(st[9]) for st in states], None if forced is None else len(forced)))
        out = []
        for j, st in enumerate(states):
            if st[9] == 3:                                   # this model's own call declines it: its solo tail answers
                out.append(solo(j))
            elif st[9] == 4:
                out.append(ValueError("bad state"))
            else:
                out.append(("ok", np.full(st[9], ord(self.name), np.float32), None, None))
        return out

    def score_state(self, state, rank=False):
        return np.full(state[9], -1.0, np.float32)


def test_model_set_falls_back_to_one_call_per_model_when_the_group_declines():
    from gcnn_cut_selector_amd import synthetic, utils
    from gcnn_cut_selector_amd.infer import _ModelsSession
    from gcnn_cut_selector_amd.model import ModelSet
    base = utils.state_to_inputs(synthetic.make_sample("setcov", 1, scale=0.2)[0])
    assert base[9] > 6

    def with_cuts(n):                                        # the same state with its first n cuts: n tells the states apart
        c, cei, cef, v, k, kei, kef, nc, nv, nk = base
        keep = kei[0] < n
        return (c, cei, cef, v, k[:n], kei[:, keep], kef[keep], nc, nv, n)

    log, runs = [], []
    mset = ModelSet({"a": _FallbackModel("a", log), "b": _FallbackModel("b", log)})

    class Declines:
        MAX, UNSUPPORTED = _ModelsSession.MAX, _ModelsSession.UNSUPPORTED

        def run(self, checked, forced, mode, model_of, models, p_max=0.0, p_max_ub=0.0):
            runs.append((list(model_of), [m.name for m in models]))
            return self.UNSUPPORTED

    mset._session = Declines()
    keys = ["b", "a", "b", "a", "b"]
    got = mset.score_states(keys, [with_cuts(n) for n in (1, 2, 3, 4, 5)], return_exceptions=True)
    assert runs == [([0, 0, 1, 1, 1], ["a", "b"])]                                   # sorted by model for the one grouped attempt
    assert log == [("a", [2, 4], None), ("b", [1, 3, 5], None)]                      # then each model once, its states in their order
    assert mset.calls == 0 and mset.max_models_per_call == 0
    assert [None if isinstance(r, Exception) else (r.shape[0], float(r[0])) for r in got] == \
        [(1, float(ord("b"))), (2, float(ord("a"))), (3, -1.0), None, (5, float(ord("b")))]  # un-permuted, solo tail and error in place
    assert isinstance(got[3], ValueError)
