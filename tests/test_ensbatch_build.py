"""CPU checks of the many-state ensemble calls (gcnn_infer_ensemble_batch, gcnn_lp_ensemble_batch, csrc/gcnn_ensbatch.hpp) and of the
server that groups ensemble requests for them: the four symbols are declared, bound and exported at ABI 13; the host file is
included once behind gcnn_ensemble.hpp and spells one launch name, its own; gcnn_ensemble.hpp's names are what they were; the one
new kernel cross-compiles for gfx950 as wave64 without scratch or atomics; every limit and bad argument is returned without a
device; the layout uploads what gcnn_infer_batch uploads and keeps the members' rows behind the output block; with one state it is
the single-state call's layout; a server made with `ensemble_batching=True` answers the requests that wait together with one
`*_ensemble_many` call per (ensemble, kind, thresholds), with `_ensemble_one`'s reply bytes."""
import ctypes as C
import os
import re
import tempfile

import pytest

import buildsupport
import launchnames
from test_ensemble_build import NAMES as ENSEMBLE_NAMES
from test_ensemble_build import _FakeConn, _frame, _requests, _scores, _Selection, _StubModel, _StubSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
ENSBATCH = os.path.join(CSRC, "gcnn_ensbatch.hpp")
SYMBOLS = ("gcnn_infer_ensemble_batch_layout_for", "gcnn_infer_ensemble_batch", "gcnn_lp_ensemble_batch_layout_for",
           "gcnn_lp_ensemble_batch")
OTHER_FAMILIES = ("k_ens_", "k_ib_", "k_sel_", "k_group_", "k_lpset_", "k_lp_", "k_hyb_", "k_mb_")
ONE = (5, 6, 3, 7, 4)
FAKE = 1 << 20


def test_symbols_in_header_binding_and_library_abi_13():
    header = buildsupport.declared_everywhere(SYMBOLS)
    from gcnn_cut_selector_amd import _lib
    assert _lib.ABI_VERSION == 13 == _lib.lib().gcnn_abi_version()           # additive: the number does not move
    for sym in ("gcnn_infer_ensemble_batch (", "gcnn_lp_ensemble_batch ("):     # the farm and the seeds it deploys
        at = header.index(sym)
        text = header[at:at + 400]
        assert "model_evaluator.py:157-241" in text and "model_trainer.py:38-49" in text, sym
    # the calls reuse the single-state calls' layout structs
    assert _lib.SIGNATURES[SYMBOLS[0]][1][-1] is _lib.SIGNATURES["gcnn_infer_ensemble_layout_for"][1][-1]
    assert _lib.SIGNATURES[SYMBOLS[2]][1][-1] is _lib.SIGNATURES["gcnn_lp_ensemble_layout_for"][1][-1]


def test_host_file_is_included_once_and_its_launch_name_is_its_own():
    buildsupport.included_once_after("gcnn_ensbatch.hpp", "gcnn_group.hpp", "gcnn_ibatch.hpp", "gcnn_lpbatch.hpp", "gcnn_ensemble.hpp")
    names = launchnames.launch_names(ENSBATCH)
    assert names == {"k_eb_mean_rank"}
    assert not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_ensbatch.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    assert not [n for n in names if any(p in n for p in OTHER_FAMILIES)]
    # the single-state calls' file spells what it spelled
    assert launchnames.launch_names(os.path.join(CSRC, "gcnn_ensemble.hpp")) == ENSEMBLE_NAMES
    # the shared work goes out under gcnn_ensemble.hpp's names: this file calls that file's generalised halves
    text = re.sub(r"//[^\n]*", "", open(ENSBATCH).read())
    for used in ("ens_layout(", "ens_call(", "lpens_layout(", "lpens_call("):
        assert used in text, used
    assert set(re.findall(r'"(k_[a-z_0-9]*)"', text)) == names          # (the include of k_ensbatch.hpp is no name)


def test_kernel_compiles_wave64_without_scratch_or_atomics():
    build = buildsupport.device_build()
    new = {k: v for k, v in build.rows.items() if "k_eb_" in k}
    assert len(new) == 1 and "k_eb_mean_rank" in next(iter(new)), sorted(new)
    for name, v in new.items():
        assert not any(p in name for p in OTHER_FAMILIES), name
        assert v["scratch"] == 0, (name, v)
        assert not re.search(r"atomic", build.body(name)), name
        assert build.wavefront_size(name) == 64, name
        print(f"{name}: LDS {v['lds']} bytes/block, {v['vgpr']} VGPRs, occupancy {v['occ']} waves/SIMD")
        assert v["lds"] == 2 * 4 * 4096          # the keys and the indices of 4,096 cuts, as k_ib_rank
    # the families the other build tests count are as they state them
    rows = list(build.rows)
    counts = {p: sum(p in r for r in rows) for p in ("k_ens_", "k_ib_", "k_sel_", "k_group_")}
    assert counts == {"k_ens_": 1, "k_ib_": 2, "k_sel_": 2, "k_group_": 35}, counts


def _dims(shapes):
    from gcnn_cut_selector_amd import _lib
    return (_lib.Dims * len(shapes))(*(_lib.Dims(*s) for s in shapes))


def _counts(values):
    return None if values is None else (C.c_int32 * len(values))(*values)


def _layout(shapes=(ONE,), nf=None, nfe=None, mode=0, M=3, n=None):
    from gcnn_cut_selector_amd import _lib
    L = _lib.EnsembleLayout()
    rc = _lib.lib().gcnn_infer_ensemble_batch_layout_for(len(shapes) if n is None else n, _dims(shapes), _counts(nf), _counts(nfe), mode, M,
                                                         C.byref(L))
    return rc, L


def _lp_dims(n_cuts=3, n_cols=6):
    return dict(n_rows=4, n_cols=n_cols, n_cuts=n_cuts, row_nnz=8, cut_nnz=2 * n_cuts, has_incumbent=0, n_model_vars=n_cols,
                n_state_rows=4, n_state_edges=8, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=1.0)


def _lp_layout(dims, nf=None, nfe=None, mode=0, M=3, n=None):
    from gcnn_cut_selector_amd import _lib
    L = _lib.LpEnsembleLayout()
    d = (_lib.LpDims * len(dims))(*(_lib.LpDims(**x) for x in dims))
    rc = _lib.lib().gcnn_lp_ensemble_batch_layout_for(len(dims) if n is None else n, d, _counts(nf), _counts(nfe), mode, M, C.byref(L))
    return rc, L, d


def test_layout_refusals_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    assert _layout()[0] == 0 and _layout(M=1)[0] == 0 and _layout(M=8)[0] == 0 and _layout([ONE] * 64)[0] == 0
    assert _layout(n=0)[0] == -1 and _layout([ONE] * 65)[0] == -1
    assert _layout(M=0)[0] == -1 and _layout(M=9)[0] == -1
    assert _layout(mode=3)[0] == -1 and _layout(mode=-1)[0] == -1
    assert _layout([ONE, (5, 6, -1, 7, 4)])[0] == -1 and _layout([ONE, ONE], nf=[0, -1], nfe=[0, 0], mode=2)[0] == -1
    assert _layout([ONE, ONE], nf=[1, 0], nfe=[2, 3], mode=2)[0] == -1       # entries without rows
    assert lib.gcnn_infer_ensemble_batch_layout_for(1, _dims([ONE]), None, None, 0, 3, None) == -1
    assert lib.gcnn_infer_ensemble_batch_layout_for(1, None, None, None, 0, 3, C.byref(_lib.EnsembleLayout())) == -1
    # 4,097 cuts in any state: the two ordering modes decline, score mode answers; 4,096 are fine everywhere
    big, fine = (5, 6, 4097, 7, 4097), (5, 6, 4096, 7, 4096)
    assert _layout([ONE, big], mode=0)[0] == 0 and _layout([ONE, big], mode=1)[0] == -4 and _layout([big, ONE], mode=2)[0] == -4
    assert all(_layout([ONE, fine], mode=m)[0] == 0 for m in (0, 1, 2))
    # edges with nothing to point at; a union past 2^24 rows; no variable limit
    assert _layout([ONE, (0, 5, 5, 3, 5)])[0] == -4
    assert _layout([(1 << 23, 6, 3, 7, 4)] * 3)[0] == -4
    assert _layout([(5, 32769, 3, 7, 4)])[0] == 0 and _layout([ONE, (5, 100000, 3, 7, 4)], mode=2)[0] == 0
    # the LP form: the same for the built states' sizes
    one = _lp_dims()
    assert _lp_layout([one])[0] == 0 and _lp_layout([one] * 64)[0] == 0
    assert _lp_layout([one], n=0)[0] == -1 and _lp_layout([one] * 65)[0] == -1
    assert _lp_layout([one], M=0)[0] == -1 and _lp_layout([one], M=9)[0] == -1 and _lp_layout([one], mode=3)[0] == -1
    assert _lp_layout([one, _lp_dims(n_cuts=-1)])[0] == -1
    assert _lp_layout([one, _lp_dims(n_cuts=4097)], mode=0)[0] == 0
    assert _lp_layout([one, _lp_dims(n_cuts=4097)], mode=1)[0] == -4 and _lp_layout([_lp_dims(n_cuts=4097), one], mode=2)[0] == -4
    assert _lp_layout([one, _lp_dims(n_cols=32769)], mode=2)[0] == 0          # admitted: no variable limit
    assert lib.gcnn_lp_ensemble_batch_layout_for(1, _lp_layout([one])[2], None, None, 0, 3, None) == -1


def test_calls_refuse_bad_arguments_before_anything_is_enqueued():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    shapes = [ONE, (4, 5, 2, 6, 3)]
    rc, EL = _layout(shapes, nf=[0, 0], nfe=[0, 0], mode=2)
    assert rc == 0
    d, zero = _dims(shapes), _counts([0, 0])
    params = (C.c_void_p * 3)(FAKE, FAKE + 4096, FAKE + 8192)

    def call(p_max=0.1, p_max_ub=0.5, arena=FAKE * 256, size=EL.u.arena_bytes, par=params, host_in=FAKE, host_out=FAKE, staging=FAKE,
             M=3, mode=2, n=2, dims=d):
        return lib.gcnn_infer_ensemble_batch(n, dims, zero, zero, mode, M, par, host_in, host_out, arena, size, staging, p_max, p_max_ub,
                                             None)

    assert call(p_max=float("nan")) == -1 and call(p_max=float("inf")) == -1 and call(p_max_ub=float("nan")) == -1
    assert call(size=EL.u.arena_bytes - 1) == -1 and call(arena=FAKE * 256 + 16) == -1 and call(arena=None) == -1
    assert call(par=None) == -1 and call(par=(C.c_void_p * 3)(FAKE, None, FAKE)) == -1
    assert call(host_in=None) == -1 and call(host_out=None) == -1 and call(staging=None) == -1
    assert call(M=0) == -1 and call(M=9) == -1 and call(mode=3) == -1 and call(n=0) == -1 and call(n=65) == -1
    assert call(dims=_dims([ONE, (5, 6, 4097, 7, 4097)])) == -4 and call(dims=_dims([ONE, (0, 5, 5, 3, 5)])) == -4
    assert call(dims=_dims([ONE, (5, 6, -1, 7, 4)])) == -1
    rc, L, ld = _lp_layout([_lp_dims(), _lp_dims(n_cuts=2)], nf=[0, 0], nfe=[0, 0], mode=2)
    assert rc == 0

    def lp_call(p_max=0.1, size=L.lp.arena_bytes, par=params, host_in=FAKE, host_out=FAKE, staging=FAKE, M=3, n=2, arena=FAKE * 256):
        return lib.gcnn_lp_ensemble_batch(n, ld, zero, zero, 2, M, par, host_in, host_out, arena, size, staging, p_max, 0.5, None)

    assert lp_call(p_max=float("nan")) == -1 and lp_call(size=L.lp.arena_bytes - 1) == -1 and lp_call(arena=FAKE * 256 + 16) == -1
    assert lp_call(par=None) == -1 and lp_call(par=(C.c_void_p * 3)(FAKE, FAKE, None)) == -1
    assert lp_call(host_in=None) == -1 and lp_call(host_out=None) == -1 and lp_call(staging=None) == -1
    assert lp_call(M=0) == -1 and lp_call(M=9) == -1 and lp_call(n=0) == -1


def _shapes(n):
    return [(500 + 7 * s, 1000 + 3 * s, 100 + s % 5, 25000 + 11 * s, 9000 + 5 * s) for s in range(n)]


def test_layout_uploads_the_union_and_holds_every_member():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    for n in (1, 3, 64):
        shapes = _shapes(n)
        dims, nf, nfe = _dims(shapes), _counts([40 + s for s in range(n)]), _counts([800 + 2 * s for s in range(n)])
        total = _lib.Dims(*(sum(s[j] for s in shapes) for j in range(5)))
        ws = 4 * lib.gcnn_workspace_floats(C.byref(total))
        for mode in (0, 1, 2):
            IL = _lib.IbatchLayout()
            assert lib.gcnn_infer_batch_layout_for(n, dims, nf, nfe, mode, C.byref(IL)) == 0
            size = C.c_size_t()
            for M in (1, 5, 8):
                EL = _lib.EnsembleLayout()
                assert lib.gcnn_infer_ensemble_batch_layout_for(n, dims, nf, nfe, mode, M, C.byref(EL)) == 0
                L = EL.u
                assert EL.n_models == M and L.n_states == n and L.total.n_cuts == total.n_cuts
                # the upload and the output block are gcnn_infer_batch's for these states, whatever M is
                assert L.in_bytes == IL.in_bytes and list(L.in_off) == list(IL.in_off) and list(L.out_off) == list(IL.out_off)
                dev_off = list(L.dev_off)
                assert all(o % 256 == 0 for o in dev_off + [EL.table_off, L.arena_bytes]) and dev_off[:14] == sorted(dev_off[:14])
                # one member row over the whole union; the rows lie behind the output block, where the one download reaches them
                assert EL.member_stride == (4 * total.n_cuts + 15) & ~15
                assert EL.member_off >= IL.out_bytes and L.out_bytes == EL.member_off + M * EL.member_stride
                end = dev_off[11] + L.out_bytes
                for m in range(M):
                    assert EL.ws_off[m] % 256 == 0 and EL.ws_off[m] >= end
                    end = EL.ws_off[m] + ws
                assert end <= dev_off[13]
                assert lib.gcnn_group_table_bytes(M, C.byref(size)) == 0 and EL.table_bytes == size.value
                assert EL.table_off % 256 == 0 and EL.table_off >= dev_off[13] and EL.table_off + EL.table_bytes <= L.arena_bytes


def _fields(a, b, struct):
    for name, kind in struct._fields_:
        x, y = getattr(a, name), getattr(b, name)
        if isinstance(x, C.Structure):
            _fields(x, y, type(x))
        elif isinstance(x, C.Array):
            if len(x) and isinstance(x[0], C.Structure):
                for p, q in zip(x, y):
                    _fields(p, q, type(p))
            else:
                assert list(x) == list(y), name
        else:
            assert x == y, name


def test_one_state_is_the_single_state_layout_field_for_field():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    shape, forced = (500, 1000, 100, 25000, 9000), (40, 800)
    for mode in (0, 1, 2):
        for M in (1, 5, 8):
            one, many = _lib.EnsembleLayout(), _lib.EnsembleLayout()
            assert lib.gcnn_infer_ensemble_layout_for(C.byref(_lib.Dims(*shape)), *forced, mode, M, C.byref(one)) == 0
            assert lib.gcnn_infer_ensemble_batch_layout_for(1, _dims([shape]), _counts(forced[:1]), _counts(forced[1:]), mode, M,
                                                            C.byref(many)) == 0
            _fields(one, many, _lib.EnsembleLayout)
            lp_one, lp_many = _lib.LpEnsembleLayout(), _lib.LpEnsembleLayout()
            d = _lib.LpDims(**_lp_dims(n_cuts=40, n_cols=30))
            assert lib.gcnn_lp_ensemble_layout_for(C.byref(d), 7, 21, mode, M, C.byref(lp_one)) == 0
            assert lib.gcnn_lp_ensemble_batch_layout_for(1, (_lib.LpDims * 1)(d), _counts([7]), _counts([21]), mode, M, C.byref(lp_many)) == 0
            _fields(lp_one, lp_many, _lib.LpEnsembleLayout)


def test_lp_layout_appends_the_lp_flags_and_cut_index_behind_the_members():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    dims = [_lp_dims(n_cuts=3 + s, n_cols=6 + s) for s in range(5)]
    K = sum(d["n_cuts"] for d in dims)
    for mode in (0, 1, 2):
        BL = _lib.LpBatchLayout()
        rc, L, d = _lp_layout(dims, nf=[1] * 5, nfe=[2] * 5, mode=mode, M=5)
        assert rc == 0 and lib.gcnn_lp_batch_layout_for(5, d, _counts([1] * 5), _counts([2] * 5), mode, C.byref(BL)) == 0
        # one upload, byte for byte gcnn_lp_batch's
        assert L.lp.in_bytes == BL.in_bytes and list(L.lp.snap_base) == list(BL.snap_base) and list(L.lp.forced_off) == list(BL.forced_off)
        assert L.lp.table_bytes == BL.table_bytes and L.lp.n_snapshots == 5
        out_off = list(L.lp.out_off)
        assert out_off[:4] == list(L.ens.u.out_off) == list(BL.out_off)[:4]
        assert out_off[4] == L.ens.u.out_bytes == L.ens.member_off + 5 * L.ens.member_stride and out_off[5] == out_off[4] + 16 * 5
        assert L.lp.out_bytes == out_off[5] + ((4 * K + 15) & ~15)


# ---- the server's grouping, with stub models -------------------------------------------------------------------------------------------
class _StubManySet(_StubSet):
    """The single-state methods of test_ensemble_build's stub and the four `*_ensemble_many` methods: each logs its keys, how many
    states it got and its thresholds, and answers request i of a call with the value 10 * (call number) + i."""

    def __init__(self, log):
        super().__init__(log)
        self.n = 0

    def _values(self, count):
        self.n += 1
        return [10 * self.n + i for i in range(count)]

    def score_ensemble_many(self, keys, states, rank=False, return_exceptions=False):
        self.log.append(("many", "score_ensemble_many", tuple(keys), len(states), bool(rank), return_exceptions))
        return [_scores(v) for v in self._values(len(states))]

    def select_cuts_ensemble_many(self, keys, states, forced=None, *, p_max, p_max_ub, return_exceptions=False):
        self.log.append(("many", "select_cuts_ensemble_many", tuple(keys), len(states), (p_max, p_max_ub, len(forced)), return_exceptions))
        return [_Selection(v) for v in self._values(len(states))]

    def score_lp_ensemble_many(self, keys, snaps, rank=False, return_exceptions=False):
        self.log.append(("many", "score_lp_ensemble_many", tuple(keys), len(snaps), bool(rank), return_exceptions))
        return [_scores(v) for v in self._values(len(snaps))]

    def select_cuts_lp_ensemble_many(self, keys, snaps, forced=None, *, p_max, p_max_ub, return_exceptions=False):
        self.log.append(("many", "select_cuts_lp_ensemble_many", tuple(keys), len(snaps), (p_max, p_max_ub, len(forced)), return_exceptions))
        return [_Selection(v) for v in self._values(len(snaps))]


def _server(tmp, log, **kw):
    from gcnn_cut_selector_amd import serve
    return serve.ScoringServer({k: _StubModel(log, k) for k in "abc"}, os.path.join(tmp, "s.sock"), model_set=_StubManySet(log), **kw)


def _feed(server, conns, messages):
    """Every (connection index, message) read into one list of waiting requests."""
    pending = []
    for c, message in messages:
        conns[c].inbox.append(_frame(message))
        server._read(conns[c], pending)
    return pending


def test_the_keyword_is_appended_and_off_by_default():
    from gcnn_cut_selector_amd import serve
    import inspect
    params = list(inspect.signature(serve.ScoringServer.__init__).parameters)
    assert params[-2:] == ["ensemble_sessions", "ensemble_batching"]
    assert serve.ScoringServer.__init__.__defaults__[-1] is False and serve.ScoringServer.__init__.__defaults__[1] is True


def test_waiting_ensemble_requests_share_one_call_per_name_kind_and_thresholds():
    from gcnn_cut_selector_amd import serve
    make, state, snap = _requests()
    log = []
    with tempfile.TemporaryDirectory() as tmp:
        server = _server(tmp, log, ensembles={"ens": ["c", "a"], "two": ["b"]}, ensemble_batching=True)
        try:
            conns = [_FakeConn() for _ in range(4)]
            for c in conns:
                server._buffers[c] = bytearray()
            # three workers under "ens" and one under "two" send one request of every kind 0-5; worker 2's selections come with
            # other thresholds; a request under the plain model "b" waits with them
            messages = []
            for c, name in enumerate(("ens", "ens", "ens", "two")):
                for kind, message in make(name):
                    if c == 2 and serve._LP_BASE.get(kind, kind) == serve.KIND_SELECT:
                        encode = serve.encode_lp_request if kind in serve._LP_BASE else serve.encode_request
                        message = encode(name, kind, snap if kind in serve._LP_BASE else state, p_max=0.3, p_max_ub=0.6, max_selected=1)
                    messages.append((c, message))
            messages.append((3, serve.encode_request("b", serve.KIND_SCORE, state)))
            pending = _feed(server, conns, messages)
            assert len(pending) == 25 and not any(c.sent for c in conns)
            server._serve(pending)
            stats = dict(server.stats)
        finally:
            server.close()
    many = [e for e in log if e[0] == "many"]
    keys, two = ("c", "a"), ("b",)
    # one call per (ensemble, kind, thresholds), groups in arrival order of their first member, every call with return_exceptions
    assert many == [("many", "score_ensemble_many", keys, 3, False, True), ("many", "score_ensemble_many", keys, 3, True, True),
                    ("many", "select_cuts_ensemble_many", keys, 2, (0.2, 0.6, 2), True),
                    ("many", "score_lp_ensemble_many", keys, 3, False, True), ("many", "score_lp_ensemble_many", keys, 3, True, True),
                    ("many", "select_cuts_lp_ensemble_many", keys, 2, (0.2, 0.6, 2), True),
                    ("many", "select_cuts_ensemble_many", keys, 1, (0.3, 0.6, 1), True),
                    ("many", "select_cuts_lp_ensemble_many", keys, 1, (0.3, 0.6, 1), True),
                    ("many", "score_ensemble_many", two, 1, False, True), ("many", "score_ensemble_many", two, 1, True, True),
                    ("many", "select_cuts_ensemble_many", two, 1, (0.2, 0.6, 1), True),
                    ("many", "score_lp_ensemble_many", two, 1, False, True), ("many", "score_lp_ensemble_many", two, 1, True, True),
                    ("many", "select_cuts_lp_ensemble_many", two, 1, (0.2, 0.6, 1), True)]
    assert not [e for e in log if e[0] == "ensemble"], "no single-state ensemble call was made"
    assert [e for e in log if e[0] == "model"] == [("model", "b", "score_states", 1)]
    assert stats["ensemble_calls"] == 14 and stats["ensemble_batched_calls"] == 6 and stats["max_ensemble_batch"] == 3
    assert stats["calls"] == 15 and stats["errors"] == 0 and stats["requests"] == 25
    # the replies: byte for byte what `_ensemble_one` sends for a result of the same values, the members in arrival order
    kinds = [k for k, _ in make("ens")]
    value = {}          # (kind, thresholds group) -> the call's number, in the order of `many`
    for number, e in enumerate(many, 1):
        value[(e[1], e[2], e[4] if isinstance(e[4], tuple) else e[4])] = number
    for c, conn in enumerate(conns):
        assert len(conn.sent) == (7 if c == 3 else 6)
        # worker 2's selections wait in groups of their own, which were formed, and so are served, after the six shared ones
        served = [kinds[i] for i in (0, 1, 3, 4, 2, 5)] if c == 2 else kinds
        for kind, sent in zip(served, conn.sent):
            lp, base = kind in serve._LP_BASE, serve._LP_BASE.get(kind, kind)
            name = ("select_cuts_lp" if lp else "select_cuts") if base == serve.KIND_SELECT else ("score_lp" if lp else "score")
            call_keys = two if c == 3 else keys
            if base == serve.KIND_SELECT:
                other = c == 2
                group = [i for i in range(3) if (i == 2) == other] if c < 3 else [3]
                number = value[(name + "_ensemble_many", call_keys, ((0.3 if other else 0.2), 0.6, len(group)))]
                v = 10 * number + group.index(c)
                want = serve.encode_reply(*serve._selection_reply(_Selection(v), 1 if other else 4, lp))
            else:
                number = value[(name + "_ensemble_many", call_keys, base == serve.KIND_RANK)]
                v = 10 * number + (c if c < 3 else 0)
                want = serve.encode_reply(*serve._scores_reply(_scores(v), base == serve.KIND_RANK, lp))
            assert sent == _frame(want), (c, kind)


def test_an_exception_in_a_slot_is_that_request_s_error_reply():
    from gcnn_cut_selector_amd import serve
    _, state, _ = _requests()
    log = []

    class Failing(_StubManySet):
        def score_ensemble_many(self, keys, states, rank=False, return_exceptions=False):
            out = super().score_ensemble_many(keys, states, rank, return_exceptions)
            out[1] = ValueError("edge index out of range")
            return out

    with tempfile.TemporaryDirectory() as tmp:
        server = serve.ScoringServer({k: _StubModel(log, k) for k in "abc"}, os.path.join(tmp, "s.sock"), model_set=Failing(log),
                                     ensembles={"ens": ["a", "b"]}, ensemble_batching=True)
        try:
            conns = [_FakeConn() for _ in range(3)]
            for c in conns:
                server._buffers[c] = bytearray()
            server._serve(_feed(server, conns, [(c, serve.encode_request("ens", serve.KIND_SCORE, state)) for c in range(3)]))
            assert server.stats["errors"] == 1 and server.stats["ensemble_calls"] == 1 and server.stats["max_ensemble_batch"] == 3
        finally:
            server.close()
    assert serve.decode_reply(conns[0].sent[0][4:])[0][0].tolist() == [10.0, 10.0]
    assert serve.decode_reply(conns[2].sent[0][4:])[0][0].tolist() == [12.0, 12.0]
    with pytest.raises(ValueError, match="edge index out of range"):          # the slot's own error, as the wire reports a ValueError
        serve.decode_reply(conns[1].sent[0][4:])


def test_the_default_server_answers_every_ensemble_request_with_its_own_call():
    from gcnn_cut_selector_amd import serve
    make, _, _ = _requests()
    log = []
    with tempfile.TemporaryDirectory() as tmp:
        server = _server(tmp, log, ensembles={"ens": ["c", "a"]})
        try:
            assert server.ensemble_batching is False
            conns = [_FakeConn(), _FakeConn()]
            for c in conns:
                server._buffers[c] = bytearray()
            server._serve(_feed(server, conns, [(c, m) for c in (0, 1) for _, m in make("ens")]))
            stats = dict(server.stats)
        finally:
            server.close()
    one = [("ensemble", "score_ensemble", ("c", "a"), False), ("ensemble", "score_ensemble", ("c", "a"), True),
           ("ensemble", "select_cuts_ensemble", ("c", "a"), (0.2, 0.6, 4)),
           ("ensemble", "score_lp_ensemble", ("c", "a"), False), ("ensemble", "score_lp_ensemble", ("c", "a"), True),
           ("ensemble", "select_cuts_lp_ensemble", ("c", "a"), (0.2, 0.6, 4))]
    assert log == one + one                              # today's log: one single-state call per request, in arrival order
    assert stats["ensemble_calls"] == 12 and stats["ensemble_batched_calls"] == 0 and stats["max_ensemble_batch"] == 0
    assert all(len(c.sent) == 6 for c in conns)
