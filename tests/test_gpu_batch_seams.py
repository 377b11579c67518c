"""The general path's graph plan (gcnn_graph_check, gcnn_graph_build) and the store's collation (gcnn_collate) at every seam (GPU).

Cases, the restatement and their proof are in tests/batchcases.py and tests/test_batchcases.py.  Every comparison is exact: offsets,
ids and permutations as integers, coefficients and features as their 32 bits.

check -- through the C ABI the two flags of every check case equal the restatement's (the planted entry is written on the device
into a copy of the size's base list, and the copy is read back and compared with the host's case); through
`BipartiteGraph(validate=True)` a planted id raises ValueError and a descent takes the sort path and builds the right plan.  A list
with a planted bad id is never built on.

build -- every build case through `BipartiteGraph(validate=True, keep_perm=True)` (the copy path when the list is sorted),
`BipartiteGraph(validate=False, keep_perm=True)` (always the sort) and gcnn_graph_build itself, all seven arrays against the
restatement (hence bit for bit against each other).  The C-ABI call writes into pattern-filled buffers with guard words behind every
array and behind gcnn_graph_temp_bytes(E) bytes of temp; one byte of temp less is GCNN_E_WORKSPACE and writes nothing.

collate -- every batch through `SampleStore.batch` against the restatement, array for array, and against
`GCNN.prepare(utils.collate(...))`; one direct gcnn_collate call per seam family into a pattern-filled destination whose words
between and behind the arrays must keep the pattern.

One process, the product library, no retry.  Measured on an MI355X: DESIGN.md, section 4.ac."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import batchcases as B  # noqa: E402
from gpucommon import dev, make_model  # noqa: E402,F401

GUARD = 9                      # words behind every array of a direct call: more than a chunk split without its clamp overshoots (7), and odd
TEMP_GUARD = 256               # bytes behind the temp of a direct build
S_CHECK, S_BUILD = B.check_seam(), B.build_seam()


def _up(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _bits(t):
    t = t.detach().reshape(-1)
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy()


def _assert_plan(got, want, what):
    for f, g, w in zip(B.CSR_FIELDS, got, want):
        w = w.view(np.int32) if w.dtype == np.float32 else w
        assert g.dtype == np.int32 and g.shape == w.shape, (what, f, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {f} differs in {at.size} of {w.size} entries, first at {at[:6].tolist()}: "
                                 f"{g[at[:6]].tolist()} for {w[at[:6]].tolist()}")


# ---- gcnn_graph_check -------------------------------------------------------------------------------------------------------------------
def _flags(ei, n, n_left, n_var, dev):
    from gcnn_cut_selector_amd import _lib
    flags = torch.full((2 + GUARD,), B.PATTERN, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gcnn_graph_check(C.c_void_p(ei.data_ptr()), n, n_left, n_var, C.c_void_p(flags.data_ptr()), _stream(dev)),
                   "gcnn_graph_check")
    host = flags.cpu().numpy()
    assert (host[2:] == B.PATTERN).all()
    return int(host[0]), int(host[1])


@pytest.mark.parametrize("n", B.check_sizes())
def test_check_flags_equal_the_restatement(dev, n):
    base = _up(np.stack(B.check_base(n)), dev, np.int32)           # one upload per size: [2, n], row 1 behind row 0
    for kind, plants in B.check_plants(n).items():
        c = B.check_case(f"E{n}/{kind}")
        ei = base.clone()
        for row, pos, value in plants:
            if pos is None:
                ei[row].fill_(value)
            else:
                ei[row, pos] = value
        want = B.check_flags(c["left"], c["var"], c["n_left"], c["n_var"])
        got = _flags(ei, n, c["n_left"], c["n_var"], dev)
        assert np.array_equal(ei.cpu().numpy(), np.stack([c["left"], c["var"]])), (n, kind)    # the device saw the host's case
        assert got == want, (n, kind, got, want)


def test_validate_refuses_a_planted_id_before_it_builds(dev):
    from gcnn_cut_selector_amd.graph import BipartiteGraph
    for cid in (f"E{S_CHECK + 1}/left=n@{S_CHECK}", f"E{S_CHECK + 1}/var=-1@{S_CHECK}", f"E{2 * S_CHECK + 1}/var=n@{2 * S_CHECK}",
                "E256/left=-1@255", "E257/var=n@256", "E1/left=n@0"):
        assert cid in B.check_ids(), cid
        c = B.check_case(cid)
        ei = _up(np.stack([c["left"], c["var"]]), dev, np.int32)
        with pytest.raises(ValueError, match="out of range"):
            BipartiteGraph(ei, torch.zeros(ei.shape[1], device=dev), c["n_left"], c["n_var"], validate=True)


def test_validate_sends_a_descent_through_the_sort(dev):
    from gcnn_cut_selector_amd.graph import BipartiteGraph
    for cid in (f"E{2 * S_CHECK + 1}/descent@{S_CHECK}", f"E{S_CHECK + 1}/descent@{S_CHECK - 1}", "E257/descent@255", "E2/descent@0",
                f"E{S_CHECK + 1}/ok", "E257/ties"):
        assert cid in B.check_ids(), cid
        c = B.check_case(cid)
        n = c["left"].size
        coef = B.distinct_coef(n)
        g = BipartiteGraph(_up(np.stack([c["left"], c["var"]]), dev, np.int32), _up(coef, dev), c["n_left"], c["n_var"], validate=True,
                           keep_perm=True)
        _assert_plan([_bits(getattr(g, f)) for f in B.CSR_FIELDS], B.csr(c["left"], c["var"], coef, c["n_left"], c["n_var"], False), cid)
        took_the_sort = not np.array_equal(_bits(g.l_perm), np.arange(n))
        assert took_the_sort == ("descent" in cid), cid


# ---- gcnn_graph_build -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uploads(dev):
    """cid -> ([2, E] int32 ids, [E] fp32 coefficients) on the device: every case is uploaded once per module."""
    cache = {}

    def get(cid):
        if cid not in cache:
            c = B.build_case(cid)
            cache[cid] = (_up(np.stack([c["left"], c["var"]]), dev, np.int32), _up(c["coef"], dev, np.float32))
        return cache[cid]
    return get


def _abi_build(dev, ei, coef, n, n_left, n_var, left_sorted, short=0):
    """gcnn_graph_build into one pattern-filled buffer: (rc, the seven arrays by CSR_FIELDS, the words that must have kept the pattern,
    the temp's bytes behind gcnn_graph_temp_bytes(n) -- or all of the temp when `short` bytes fewer are offered)."""
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    sizes = dict(l_ptr=n_left + 1, l_oth=n, l_coef=n, l_perm=n, v_ptr=n_var + 1, v_oth=n, v_coef=n)
    off, total = {}, GUARD
    for f in B.CSR_FIELDS:
        off[f] = total
        total += sizes[f] + GUARD
    buf = torch.full((total,), B.PATTERN, dtype=torch.int32, device=dev)
    p = lambda f: C.c_void_p(buf.data_ptr() + 4 * off[f])
    temp_bytes = int(lib.gcnn_graph_temp_bytes(n))
    temp = torch.full((temp_bytes + TEMP_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gcnn_graph_build(C.c_void_p(ei.data_ptr() if n else 0), C.c_void_p(coef.data_ptr() if n else 0), n, n_left, n_var,
                                  int(left_sorted), p("l_ptr"), p("l_oth"), p("l_coef"), p("v_ptr"), p("v_oth"), p("v_coef"), p("l_perm"),
                                  C.c_void_p(temp.data_ptr()), temp_bytes - short, _stream(dev))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    keep = np.ones(total, bool)
    arrays = []
    for f in B.CSR_FIELDS:
        arrays.append(host[off[f]:off[f] + sizes[f]])
        keep[off[f]:off[f] + sizes[f]] = False
    behind = temp[0 if short else temp_bytes:].cpu().numpy()
    return rc, arrays, host[keep], behind, temp_bytes


@pytest.mark.parametrize("cid", B.BUILD_IDS)
def test_build_in_three_forms_equals_the_restatement(dev, uploads, cid):
    from gcnn_cut_selector_amd.graph import BipartiteGraph
    c = B.build_case(cid)
    n, n_left, n_var = c["left"].size, c["n_left"], c["n_var"]
    ei, coef = uploads(cid)
    want = B.expected_csr(cid, left_sorted=False)                  # (the copy path's arrays are the sort's: tests/test_batchcases.py)
    for validate in (True, False):
        g = BipartiteGraph(ei, coef, n_left, n_var, validate=validate, keep_perm=True, sync_max_degree=True)
        _assert_plan([_bits(getattr(g, f)) for f in B.CSR_FIELDS], want, f"{cid} validate={validate}")
        assert (g.l_max_deg, g.v_max_deg) == B.max_degrees(want), cid
        assert (g.n_edges, g.n_left, g.n_var) == (n, n_left, n_var)
    rc, arrays, kept, behind, temp_bytes = _abi_build(dev, ei, coef, n, n_left, n_var, c["left_sorted"])
    assert rc == 0
    _assert_plan(arrays, want, f"{cid} C ABI left_sorted={c['left_sorted']}")
    assert (kept == B.PATTERN).all(), (cid, int((kept != B.PATTERN).sum()))
    assert (behind == 0xA5).all() and temp_bytes >= 3 * 4 * n, cid


@pytest.mark.parametrize("cid", ["E/257/unsorted", "lead-trail/sorted", "E0/sorted"])
def test_one_byte_of_temp_short_is_refused_and_nothing_is_written(dev, uploads, cid):
    c = B.build_case(cid)
    ei, coef = uploads(cid)
    rc, arrays, kept, temp, _ = _abi_build(dev, ei, coef, c["left"].size, c["n_left"], c["n_var"], c["left_sorted"], short=1)
    assert rc == -2                                                # GCNN_E_WORKSPACE
    assert (kept == B.PATTERN).all() and all((a == B.PATTERN).all() for a in arrays) and (temp == 0xA5).all()


@pytest.mark.parametrize("cid", ["E/257/unsorted", "lead-trail/sorted", "ties/unsorted"])
def test_transposed_view_is_built_like_the_contiguous_list(dev, cid):
    from gcnn_cut_selector_amd.graph import BipartiteGraph
    c = B.build_case(cid)
    pairs = _up(np.stack([c["left"], c["var"]], axis=1), dev, np.int32)        # [E, 2]: the list as (left, variable) pairs
    view = pairs.T
    assert not view.is_contiguous() and tuple(view.shape) == (2, c["left"].size)
    g = BipartiteGraph(view, _up(c["coef"], dev).reshape(-1, 1), c["n_left"], c["n_var"], validate=True, keep_perm=True)
    _assert_plan([_bits(getattr(g, f)) for f in B.CSR_FIELDS], B.expected_csr(cid, left_sorted=False), cid)


@pytest.mark.parametrize("cid", ["lead-trail/sorted", "lead-trail/unsorted", "first-last/unsorted", "E/256/sorted"])
def test_segment_plan_of_a_sorted_and_an_unsorted_index(dev, cid):
    from gcnn_cut_selector_amd import ops
    c = B.build_case(cid)
    plan = ops.SegmentPlan(_up(c["left"], dev, np.int32), c["n_left"])
    zeros = np.zeros(c["left"].size, np.int32)
    want = B.csr(c["left"], zeros, zeros.astype(np.float32), c["n_left"], 1, False)
    assert plan.sorted == c["left_sorted"] and (plan.n_recv, plan.n_edges) == (c["n_left"], c["left"].size)
    assert np.array_equal(_bits(plan.seg_ptr), want[0]) and np.array_equal(_bits(plan.perm), want[3]), cid


# ---- gcnn_collate -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store(dev):
    from gcnn_cut_selector_amd.store import SampleStore
    return SampleStore.from_samples(B.pool(), dev, chunk=7)       # seven ingestion chunks, the last one short


@pytest.fixture(scope="module")
def model(dev):
    return make_model(3, dev)[0]


def _batch_words(sb):
    out = {"cons_feats": sb.batch.cons_feats, "var_feats": sb.batch.var_feats, "cut_feats": sb.batch.cut_feats, "improvements": sb.improvements}
    for slot, g in enumerate((sb.batch.cons_graph, sb.batch.cut_graph)):
        for f in ("l_ptr", "l_oth", "l_coef", "v_ptr", "v_oth", "v_coef"):
            out[f"{slot}.{f}"] = getattr(g, f)
    return {k: _bits(v) for k, v in out.items()}


@pytest.mark.parametrize("bid", B.BATCH_IDS)
def test_store_batch_equals_the_restatement_and_the_host_path(dev, store, model, bid):
    from gcnn_cut_selector_amd import utils
    ids = B.batches()[bid]
    assert len(store) == len(B.pool())
    sb = store.batch(ids)
    got, want = _batch_words(sb), B.collate(ids)
    for name in B.NAMES:
        assert got[name].shape == want[name].shape, (bid, name, got[name].shape, want[name].shape)
        if not np.array_equal(got[name], want[name]):
            at = np.flatnonzero(got[name] != want[name])
            raise AssertionError(f"{bid}: {name} differs in {at.size} of {want[name].size} words, first at {at[:6].tolist()}")
    host = utils.collate([B.pool()[i] for i in ids])
    prepared = model.prepare(tuple(host[:7]) + (int(host[7].sum()), int(host[8].sum()), int(host[9].sum())))
    for name in ("cons_feats", "var_feats", "cut_feats"):
        assert torch.equal(getattr(sb.batch, name), getattr(prepared, name)), name
    for gname in ("cons_graph", "cut_graph"):
        a, b = getattr(sb.batch, gname), getattr(prepared, gname)
        assert (a.n_edges, a.n_left, a.n_var) == (b.n_edges, b.n_left, b.n_var)
        for f in ("l_ptr", "l_oth", "l_coef", "v_ptr", "v_oth", "v_coef"):
            assert torch.equal(getattr(a, f), getattr(b, f)), f"{gname}.{f}"
    assert [getattr(sb.batch.dims, f) for f, _ in sb.batch.dims._fields_] == [getattr(prepared.dims, f) for f, _ in prepared.dims._fields_]
    for got_n, want_n in ((sb.n_cons, host[7]), (sb.n_vars, host[8]), (sb.n_cuts, host[9])):
        np.testing.assert_array_equal(got_n, want_n)
    np.testing.assert_array_equal(sb.improvements.cpu().numpy(), host[10])


@pytest.fixture(scope="module")
def store_words(dev):
    """The restatement's store on the device: the sources of the direct calls (GUARD words behind each, so that a copy which
    overshoots a sample's segment still reads the test's own memory)."""
    return {name: _up(np.concatenate([a, np.full(GUARD, B.PATTERN, np.int32)]), dev, np.int32) for name, a in B.store()[0].items()}


@pytest.mark.parametrize("bid", ["b1", "every-tiny", "b257", "large"])     # the last sample's tail, the chunk split, the item loop, the copy loop
def test_direct_collate_writes_its_arrays_and_nothing_else(dev, store_words, bid):
    from gcnn_cut_selector_amd import _lib
    ids = B.batches()[bid]
    b = len(ids)
    want = B.collate(ids, guard=GUARD)
    src_off, dst_off = B.tables(ids)
    tab = _up(np.concatenate([src_off.reshape(-1), dst_off.reshape(-1)]), dev, np.int64)
    off, total = {}, GUARD
    for name in B.NAMES:
        off[name] = total
        total += want[name].size
    buf = torch.full((total,), B.PATTERN, dtype=torch.int32, device=dev)
    jobs = (_lib.CollateJob * len(B.JOBS))()
    for i, (name, kind, width, add, is_ptr) in enumerate(B.JOBS):
        src = store_words[name]
        jobs[i] = _lib.CollateJob(src.data_ptr() if src.numel() else 0, buf.data_ptr() + 4 * off[name], kind, width, add, is_ptr)
    max_words = max(want[name].size for name in B.NAMES)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gcnn_collate(jobs, len(B.JOBS), C.c_void_p(tab.data_ptr()), C.c_void_p(tab.data_ptr() + 8 * 5 * b), b,
                                           max_words, _stream(dev)), "gcnn_collate")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == B.PATTERN).all()
    for name in B.NAMES:
        got, w = host[off[name]:off[name] + want[name].size], want[name]
        assert (w[-GUARD:] == B.PATTERN).all()
        if not np.array_equal(got, w):
            at = np.flatnonzero(got != w)
            raise AssertionError(f"{bid}: {name} (+ {GUARD} guard words) differs in {at.size} of {w.size} words, first at {at[:6].tolist()}")
