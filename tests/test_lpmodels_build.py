"""CPU checks of the call that scores LP snapshots of several models at once (gcnn_lp_models) and of the server that uses it:
declared, exported and bound at ABI 13; two launch names of its own and no kernel of its own; a layout that is gcnn_infer_models'
for the built states' sizes with gcnn_lp_batch's snapshot, output and scratch parts behind it; a table that is the two parents'
tables one behind the other, the descriptor's byte positions shifted by the new offsets and nothing else; limits returned without
a device; a server that groups LP requests across models."""
import ctypes as C
import os
import re
import tempfile

import numpy as np

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
LPMODELS = os.path.join(CSRC, "gcnn_lpmodels.hpp")
SYMBOLS = ("gcnn_lp_models_layout_for", "gcnn_lp_models_fill_table", "gcnn_lp_models")
NAMES = {"k_lpm_stats", "k_lpm_emit"}           # the records of k_lpset_stats / k_lpset_emit in this call
# kernels per family, as the other build tests count them (by substring of the symbol)
FAMILIES = {"k_lp_": 2, "k_lpset_": 2, "k_ib_": 2, "k_mb_": 2, "k_sel_": 2, "k_group_": 35, "k_pgroup_": 9, "k_rank": 3, "k_hyb_": 3,
            "k_lpm_": 0}


def test_symbols_in_header_binding_and_library_abi_13():
    header = buildsupport.declared_everywhere(SYMBOLS)
    from gcnn_cut_selector_amd import _lib
    assert "gcnn_lp_models_layout" in header
    assert C.sizeof(_lib.LpModelsLayout) == C.sizeof(_lib.MbatchLayout) + C.sizeof(_lib.LpBatchLayout)


def test_launch_names_are_its_own_and_it_has_no_kernel():
    names = launchnames.launch_names(LPMODELS)
    assert names == NAMES
    assert len(launchnames.launch_names()) == 28 and not names & launchnames.launch_names()
    code = re.sub(r"//[^\n]*", "", open(LPMODELS).read())
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_lpmodels.hpp":
            theirs = launchnames.launch_names(os.path.join(CSRC, other))
            assert not names & theirs, other
            assert not [n for n in theirs if f'"{n}"' in code], other        # it records no launch under another file's name
    buildsupport.included_once_after("gcnn_lpmodels.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp", "gcnn_group.hpp", "gcnn_ibatch.hpp",
                                     "gcnn_lpbatch.hpp", "gcnn_mbatch.hpp")
    assert "__global__" not in code and "#include" not in code
    # the builder launches and the run half are the parents', shared, not copied
    for shared in ("lpset_layout(", "lpset_fill(", "lpset_launch(", "lpset_at(", "mbatch_layout(", "mbatch_prepare(", "mbatch_run(",
                   "k_lpset_stats,", "k_lpset_emit,"):
        assert code.count(shared) == 1, shared


def test_kernel_families_keep_their_counts():
    rows = list(buildsupport.device_build().rows)
    assert {f: sum(f in r for r in rows) for f in FAMILIES} == FAMILIES


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=100, n_cols=50, n_cuts=7, row_nnz=400, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=130,
             n_state_edges=520, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.0)
    f.update(over)
    return _lib.LpDims(**f)


def _args(dims, model_of, forced=None, n_models=None):
    n = len(dims)
    from gcnn_cut_selector_amd import _lib
    d = (_lib.LpDims * max(n, 1))(*dims)
    nf = (C.c_int32 * max(n, 1))(*(f[0] for f in forced)) if forced else None
    nfe = (C.c_int32 * max(n, 1))(*(f[1] for f in forced)) if forced else None
    mos = (C.c_int32 * max(len(model_of), 1))(*model_of)
    M = (max(model_of) + 1 if model_of else 1) if n_models is None else n_models
    return d, nf, nfe, mos, M


def _layout(dims, model_of, forced=None, mode=0, n_models=None):
    from gcnn_cut_selector_amd import _lib
    d, nf, nfe, mos, M = _args(dims, model_of, forced, n_models)
    L = _lib.LpModelsLayout()
    rc = _lib.lib().gcnn_lp_models_layout_for(len(dims), d, nf, nfe, mode, M, mos, C.byref(L))
    return rc, L, (d, nf, nfe, mos, M)


def _fields(struct, skip=()):
    """A ctypes structure as nested lists, so that two of them compare with ==."""
    out = []
    for name, _ in struct._fields_:
        if name in skip:
            continue
        v = getattr(struct, name)
        out.append(_fields(v) if isinstance(v, C.Structure) else
                   [_fields(x) if isinstance(x, C.Structure) else x for x in v] if isinstance(v, C.Array) else v)
    return out


DIMS = dict(a=dict(), b=dict(n_rows=0, row_nnz=0, n_state_rows=0, n_state_edges=0), c=dict(has_incumbent=0, n_cols=300, n_model_vars=300),
            d=dict(n_cuts=600, cut_nnz=5000), e=dict(n_cuts=1, cut_nnz=3))
UNION = ("a", "b", "c", "d", "e", "a")
MODEL_OF = [0, 1, 1, 1, 2, 3]
FORCED = [(0, 0), (2, 9), (1, 1), (0, 0), (3, 4), (0, 0)]
ENTRY_WORDS, N_POS = 2 * (22 + 7 + 9), 22 + 7 + 9          # LpSetEntry: 38 byte positions in front of its scalars


def test_layout_is_the_models_union_with_the_lp_parts_behind_it():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    dims = [_dims(**DIMS[x]) for x in UNION]
    n = len(dims)
    sd = (_lib.Dims * n)(*(_lib.Dims(x.n_state_rows, x.n_cols, x.n_cuts, x.n_state_edges, x.cut_nnz) for x in dims))
    mb_words, ib_words = _lib.MBATCH_TABLE_WORDS, _lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE
    for mode in (0, 1, 2):
        rc, L, (d, nf, nfe, mos, M) = _layout(dims, MODEL_OF, FORCED, mode)
        assert rc == 0 and M == 4 and L.lp.n_snapshots == n
        # the state part: gcnn_infer_models' own layout for the built states' sizes, and the lp part's copy of its union
        ML = _lib.MbatchLayout()
        assert lib.gcnn_infer_models_layout_for(n, sd, nf, nfe, mode, M, mos, C.byref(ML)) == 0
        assert _fields(L.models) == _fields(ML) and _fields(L.lp.state) == _fields(ML.u)
        # the snapshot, output and scratch parts: gcnn_lp_batch's, behind a longer table and a larger union
        B = _lib.LpBatchLayout()
        assert lib.gcnn_lp_batch_layout_for(n, d, nf, nfe, mode, C.byref(B)) == 0
        grown = 4 * (mb_words - ib_words)
        assert grown % 16 == 0 and L.lp.table_bytes == B.table_bytes + grown and L.lp.in_bytes == B.in_bytes + grown
        assert [o - grown for o in list(L.lp.snap_base)[:n]] == list(B.snap_base)[:n]
        assert [o - grown for o in L.lp.forced_off] == list(B.forced_off)
        assert list(L.lp.out_off) == list(B.out_off) and L.lp.out_bytes == B.out_bytes
        assert list(L.lp.scratch_base) == list(B.scratch_base)
        # blocks of the arena: aligned, disjoint, in order: the union | the upload | the output block | the scratch
        lp = L.lp
        assert all(o % 256 == 0 for o in (lp.up_off, lp.out_dev_off, lp.scratch_off, lp.arena_bytes))
        assert all(o % 16 == 0 for o in list(lp.snap_base) + list(lp.forced_off) + list(lp.out_off) + [lp.table_bytes, lp.in_bytes])
        assert ML.u.arena_bytes <= lp.up_off and lp.up_off + lp.in_bytes <= lp.out_dev_off
        assert lp.out_dev_off + lp.out_bytes <= lp.scratch_off
        assert lp.arena_bytes - lp.scratch_off == B.arena_bytes - B.scratch_off
        assert lp.out_dev_off - lp.up_off >= lp.in_bytes and lp.scratch_off - lp.out_dev_off == B.scratch_off - B.out_dev_off
        # the table: gcnn_infer_models' words, then gcnn_lp_batch's descriptor part
        table = np.full(lp.table_bytes // 4, -1, np.int32)
        assert lib.gcnn_lp_models_fill_table(n, d, nf, nfe, mode, M, mos, table.ctypes.data) == 0
        mb = np.zeros(mb_words, np.int32)           # (both fillers of a whole upload table zero what they do not write)
        sel = mode == 2
        assert lib.gcnn_infer_models_fill_table(n, sd, nf if sel else None, nfe if sel else None, M, mos, mb.ctypes.data) == 0
        assert np.array_equal(table[:mb_words], mb)
        plain = np.full(B.table_bytes // 4, -1, np.int32)
        assert lib.gcnn_lp_batch_fill_table(n, d, nf, nfe, mode, plain.ctypes.data) == 0
        assert np.array_equal(plain[:ib_words], mb[:ib_words])                       # (the union's columns are the same ones)
        mine, theirs = table[mb_words:], plain[ib_words:]
        head = 4 + 2 * _lib.IBATCH_TABLE_STRIDE
        assert mine.size == theirs.size and np.array_equal(mine[:head], theirs[:head])
        entry = (mine.size - head) // n
        assert entry * n == mine.size - head and entry > ENTRY_WORDS
        # the descriptors: the scalars are the same; every byte position is shifted by where its block now lies, and nothing else
        cols = mb[:ib_words].reshape(_lib.IBATCH_TABLE_COLS, -1)
        shift = ([lp.up_off - B.up_off + grown] * 22 + [lp.scratch_off - B.scratch_off] * 7
                 + [L.models.u.in_off[2 + j] - B.state.in_off[2 + j] for j in range(7)] + [lp.out_dev_off - B.out_dev_off] * 2)
        for s in range(n):
            a, b = mine[head + s * entry:][:entry], theirs[head + s * entry:][:entry]
            assert np.array_equal(a[ENTRY_WORDS:], b[ENTRY_WORDS:]), s
            pa, pb = a[:ENTRY_WORDS].view(np.int64), b[:ENTRY_WORDS].view(np.int64)
            assert (pa - pb).tolist() == shift, s
            assert (pa[1:] >= 0).all() and (pa[1:] < lp.arena_bytes).all()
            assert pa[29] == L.models.u.in_off[2] + 16 * cols[0][s] and pa[36] == lp.out_dev_off + lp.out_off[5] + 4 * cols[2][s]


def test_limits_and_bad_arguments_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    one = _dims()
    # n outside 1..64, n_models outside 1..8
    assert _layout([], [])[0] == -1 and _layout([one] * 65, [0] * 65)[0] == -1 and _layout([one] * 64, [0] * 64)[0] == 0
    assert _layout([one], [0], n_models=0)[0] == -1 and _layout([one] * 9, list(range(9)))[0] == -1
    assert _layout([one] * 8, list(range(8)))[0] == 0
    assert _layout([one], [0], mode=3)[0] == -1
    # a decreasing or gapped model_of_snapshot, an index outside 0..n_models-1, a model without a snapshot
    assert _layout([one] * 3, [0, 1, 0])[0] == -1 and _layout([one] * 2, [0, 2], n_models=3)[0] == -1
    assert _layout([one] * 2, [0, 2], n_models=2)[0] == -1 and _layout([one] * 2, [-1, 0], n_models=2)[0] == -1
    assert _layout([one] * 2, [1, 1], n_models=2)[0] == -1 and _layout([one] * 2, [0, 0], n_models=2)[0] == -1
    d, nf, nfe, mos, M = _args([one], [0])
    assert lib.gcnn_lp_models_layout_for(1, d, None, None, 0, 1, None, C.byref(_lib.LpModelsLayout())) == -1
    assert lib.gcnn_lp_models_layout_for(1, d, None, None, 0, 1, mos, None) == -1
    assert lib.gcnn_lp_models_layout_for(1, None, None, None, 0, 1, mos, C.byref(_lib.LpModelsLayout())) == -1
    # what gcnn_lp_batch refuses: a gcnn_lp_dims gcnn_lp_layout_for refuses, forced entries without a row, unions that are too large
    for over in (dict(n_rows=-1), dict(n_model_vars=0), dict(obj_norm=float("nan")), dict(infinity=0.0), dict(n_state_rows=201)):
        assert _layout([one, _dims(**over)], [0, 1])[0] == -1, over
    assert _layout([one, one], [0, 1], [(0, 0), (0, 3)], 2)[0] == -1
    wide = _dims(n_rows=(1 << 23) + 1, row_nnz=0, n_state_rows=(1 << 23) + 1, n_state_edges=0)
    assert _layout([wide, wide], [0, 1])[0] == -4
    assert _layout([one, _dims(n_cuts=0)], [0, 0])[0] == -4                            # cut entries with no cut to point at
    assert _layout([one, _dims(n_cols=40000, n_model_vars=40000)], [0, 1])[0] == 0     # no variable limit
    assert _layout([one, _dims(n_cuts=0, cut_nnz=0), _dims(n_cuts=4097, cut_nnz=5000)], [0, 0, 1], mode=1)[0] == 0   # riders
    # the call itself: everything is returned before anything is enqueued
    rc, L, (d, nf, nfe, mos, M) = _layout([one, one], [0, 1], mode=2)
    assert rc == 0
    fake = 1 << 20
    params = (C.c_void_p * 2)(fake, fake)

    def call(n=2, p_max=0.1, arena=fake * 256, size=L.lp.arena_bytes, par=params, host_in=fake, host_out=fake, staging=fake, mos=mos, M=2):
        return lib.gcnn_lp_models(n, d, None, None, 2, M, mos, par, host_in, host_out, arena, size, staging, p_max, 0.5, None)

    assert call(p_max=float("nan")) == -1 and call(p_max=float("inf")) == -1
    assert call(size=L.lp.arena_bytes - 1) == -1 and call(arena=fake * 256 + 16) == -1
    assert call(par=None) == -1 and call(par=(C.c_void_p * 2)(fake, None)) == -1
    assert call(host_in=None) == -1 and call(host_out=None) == -1 and call(staging=None) == -1
    assert call(mos=(C.c_int32 * 2)(1, 0)) == -1 and call(M=9) == -1 and call(M=0) == -1 and call(mos=None) == -1
    assert call(n=0) == -1 and call(n=65) == -1
    table = (C.c_int32 * (L.lp.table_bytes // 4))()
    assert lib.gcnn_lp_models_fill_table(2, d, None, None, 2, 2, mos, None) == -1
    assert lib.gcnn_lp_models_fill_table(2, d, None, None, 2, 2, (C.c_int32 * 2)(1, 0), table) == -1
    assert lib.gcnn_lp_models_fill_table(2, d, None, None, 2, 3, mos, table) == -1
    assert lib.gcnn_lp_models_fill_table(2, d, None, None, 2, 2, mos, table) == 0


class _StubModel:
    device = "stub"

    def __init__(self, log, name):
        self.log, self.name = log, name

    def score_lps(self, snapshots, rank=False, return_exceptions=False):
        self.log.append(("model", self.name, "score", len(snapshots)))
        return [_scores() for _ in snapshots]

    def select_cuts_lp_many(self, snapshots, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        self.log.append(("model", self.name, "select", len(snapshots)))
        return [_selection() for _ in snapshots]

    def score_states(self, *args, **kwargs):
        raise AssertionError("not asked for")

    select_cuts_many = score_states


class _StubSet:
    def __init__(self, log):
        self.log = log

    def score_lps(self, keys, snapshots, rank=False, return_exceptions=False):
        self.log.append(("set", tuple(keys), "score", len(snapshots)))
        return [_scores() for _ in snapshots]

    def select_cuts_lp_many(self, keys, snapshots, forced=None, *, p_max=0.1, p_max_ub=0.5, max_selected=None, return_exceptions=False):
        self.log.append(("set", tuple(keys), "select", len(snapshots)))
        return [_selection() for _ in snapshots]

    score_states = select_cuts_many = _StubModel.score_states


class _Scores(np.ndarray):
    cut_index = rankings = np.zeros(1, np.int32)


def _scores():
    return np.zeros(1, np.float32).view(_Scores)


def _selection():
    from types import SimpleNamespace
    return SimpleNamespace(scores=np.zeros(1, np.float32), order=np.zeros(1, np.int32), cut_index=np.zeros(1, np.int32), n_kept=1)


def _served(keys, kind, devices=None, model_set=True, **options):
    """(calls made, stats) of one sweep over one LP request of `kind` per key."""
    from gcnn_cut_selector_amd import serve, synthetic
    snap = synthetic.make_lp_snapshot("setcov", 1, scale=0.2)
    log = []
    models = {k: _StubModel(log, k) for k in "abc"}
    for k, d in (devices or {}).items():
        models[k].device = d
    with tempfile.TemporaryDirectory() as tmp:
        server = serve.ScoringServer(models, os.path.join(tmp, "s.sock"), model_set=_StubSet(log) if model_set else None, **options)
        try:
            pending = [(None, serve.decode_request(serve.encode_lp_request(k, kind, snap))) for k in keys]
            server._serve(pending)          # (no connection is registered: the replies are dropped, the calls are what counts)
        finally:
            server.close()
    return log, server.stats


def test_server_groups_lp_requests_across_models():
    from gcnn_cut_selector_amd import serve
    for kind, what in ((serve.KIND_LP_SCORE, "score"), (serve.KIND_LP_RANK, "score"), (serve.KIND_LP_SELECT, "select")):
        log, stats = _served("abc", kind, cross_model_lp=True)
        assert log == [("set", ("a", "b", "c"), what, 3)] and stats["calls"] == 1 and stats["max_models_per_call"] == 3
        # requests of ONE model take that model's own call, whatever the grouping
        log, stats = _served("bbb", kind, cross_model_lp=True)
        assert log == [("model", "b", what, 3)] and stats["calls"] == 1 and stats["max_models_per_call"] == 1
        per_model = [("model", k, what, 1) for k in "abc"]
        for options in (dict(cross_model=False), dict(cross_model_lp=False), dict(cross_model=False, cross_model_lp=True)):
            log, stats = _served("abc", kind, **options)
            assert log == per_model and stats["calls"] == 3 and stats["max_models_per_call"] == 1, options
        # models on two devices cannot share a ModelSet
        log, stats = _served("abc", kind, devices={"c": "elsewhere"}, model_set=False, cross_model_lp=True)
        assert log == per_model and stats["max_models_per_call"] == 1
    # two thresholds: two groups, each across models
    from gcnn_cut_selector_amd import synthetic
    snap = synthetic.make_lp_snapshot("setcov", 1, scale=0.2)
    log = []
    with tempfile.TemporaryDirectory() as tmp:
        server = serve.ScoringServer({k: _StubModel(log, k) for k in "abc"}, os.path.join(tmp, "s.sock"), model_set=_StubSet(log),
                                     cross_model_lp=True)
        try:
            server._serve([(None, serve.decode_request(serve.encode_lp_request(k, serve.KIND_LP_SELECT, snap, None, p, 0.5)))
                           for k, p in (("a", 0.1), ("b", 0.2), ("c", 0.1), ("a", 0.2))])
        finally:
            server.close()
    assert log == [("set", ("a", "c"), "select", 2), ("set", ("b", "a"), "select", 2)]
    defaults = serve.ScoringServer.__init__.__defaults__
    assert defaults[1] is True and defaults[3] is True      # cross_model, cross_model_lp: profiles/lp_models.txt


class _FallbackModel:
    """What `ModelSet` needs of a model when the grouped LP call declines: a device, `_many` and the solo entry point."""
    device = "stub"

    def __init__(self, name, log):
        self.name, self.log = name, log

    def _many(self, snapshots, mode, solo, forced=None, p_max=0.0, p_max_ub=0.0, lp=False):
        self.log.append((self.name, lp, [int(s.cut_lhs.shape[0]) for s in snapshots]))
        out = []
        for j, s in enumerate(snapshots):
            n = int(s.cut_lhs.shape[0])
            if n == 3:                                       # this model's own call declines it: its solo tail answers
                out.append(solo(j))
            elif n == 4:
                out.append(ValueError("bad snapshot"))
            else:
                out.append(("ok", np.full(n, ord(self.name), np.float32).view(_Scores), None, None, np.arange(n, dtype=np.int32)))
        return out

    def score_lp(self, snapshot, rank=False):
        return np.full(int(snapshot.cut_lhs.shape[0]), -1.0, np.float32).view(_Scores)


def test_model_set_falls_back_to_one_lp_call_per_model_when_the_group_declines():
    from gcnn_cut_selector_amd import synthetic
    from gcnn_cut_selector_amd.infer import _LPBatchSession, _LPModelsSession
    from gcnn_cut_selector_amd.model import ModelSet
    log, runs = [], []
    mset = ModelSet({"a": _FallbackModel("a", log), "b": _FallbackModel("b", log)})

    class Declines:
        MAX, UNSUPPORTED = _LPModelsSession.MAX, _LPModelsSession.UNSUPPORTED
        base = _LPBatchSession(None)                         # its snapshot check needs no device

        def run(self, checked, forced, mode, model_of, models, p_max=0.0, p_max_ub=0.0):
            runs.append((list(model_of), [m.name for m in models], [d["n_cuts"] for _, d in checked]))
            return self.UNSUPPORTED

    mset._lp_session = Declines()
    keys = ["b", "a", "b", "a", "b"]
    snaps = [synthetic.make_lp_snapshot("setcov", 1, scale=0.2, n_cuts=n) for n in (1, 2, 3, 4, 5)]
    got = mset.score_lps(keys, snaps, return_exceptions=True)
    assert runs == [([0, 0, 1, 1, 1], ["a", "b"], [2, 4, 1, 3, 5])]                  # sorted by model for the one grouped attempt
    assert log == [("a", True, [2, 4]), ("b", True, [1, 3, 5])]                      # then each model once, its snapshots in their order
    assert mset.calls == 0 and mset.max_models_per_call == 0
    assert [None if isinstance(r, Exception) else (r.shape[0], float(r[0])) for r in got] == \
        [(1, float(ord("b"))), (2, float(ord("a"))), (3, -1.0), None, (5, float(ord("b")))]  # un-permuted, solo tail and error in place
    assert isinstance(got[3], ValueError) and np.array_equal(got[4].cut_index, np.arange(5))
    # an unknown key and a snapshot that breaks its contract on the host hold their own errors and reach no call
    runs.clear()
    bad = synthetic.make_lp_snapshot("setcov", 1, scale=0.2, n_cuts=2)
    bad.obj_norm = float("nan")
    got = mset.score_lps(["a", "nobody", "b", "b"], [snaps[0], snaps[1], bad, snaps[4]], return_exceptions=True)
    assert isinstance(got[1], KeyError) and isinstance(got[2], ValueError) and runs[0][2] == [1, 5]
