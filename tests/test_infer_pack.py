"""CPU checks of the host side of single-call inference (gcnn_cut_selector_amd/infer.py): the one packer writes, into a plain NumPy
buffer, exactly the bytes that the layout comments of include/gcnn_hip.h describe -- for gcnn_infer's layout and for a three-state
gcnn_infer_batch layout --, and the small helpers equal the expressions they replaced."""
import ctypes as C

import numpy as np
import pytest

f32, i32 = np.float32, np.int32
STRIDES = (16, 8, 4, 56, 24, 8, 4)     # bytes per row / edge of in_off[2..8] of the batch layout (gcnn_hip.h)
COLUMNS = (0, 3, 3, 1, 2, 4, 4)        # and the table column that holds each block's per-state offset: c, e1, e1, v, k, e2, e2


def _states():
    """Three states at scale 0.2: as get_state hands them over; int64 / float64 with the cut edges permuted out of row order;
    no constraint edges at all."""
    from gcnn_cut_selector_amd import synthetic, utils
    a, b, c = (utils.state_to_inputs(synthetic.make_sample(p, 3 + i, scale=0.2)[0]) for i, p in enumerate(("setcov", "capfac", "indset")))
    perm = np.random.default_rng(5).permutation(b[5].shape[1])
    assert np.any(np.diff(b[5][0, perm]) < 0)
    b = (b[0].astype(np.float64), b[1].astype(np.int64), b[2].astype(np.float64), b[3].astype(np.float64), b[4].astype(np.float64),
         b[5][:, perm].astype(np.int64), b[6][perm].astype(np.float64)) + b[7:]
    c = (c[0], np.zeros((2, 0), i32), np.zeros((0, 1), f32)) + c[3:]
    return a, b, c


def _restate(buf, arrays, where):
    """The layout comments of include/gcnn_hip.h: features fp32 row-major; an edge set as [rows | cols] int32 and fp32 values, in
    row order with the entries of a row in their input order."""
    def put(off, a, dt):
        raw = np.ascontiguousarray(a, dtype=dt).reshape(-1).view(np.uint8)
        buf[off:off + raw.size] = raw
    c, cei, cef, v, k, kei, kef = arrays
    put(where[0], c, f32), put(where[3], v, f32), put(where[4], k, f32)
    for io, fo, ei, ef in ((where[1], where[2], cei, cef), (where[5], where[6], kei, kef)):
        perm = np.argsort(ei[0], kind="stable")
        put(io, ei[:, perm], i32), put(fo, ef.reshape(-1)[perm], f32)


def test_pack_state_single_layout():
    from gcnn_cut_selector_amd import _lib, infer
    scratch = None
    for st in _states():
        arrays, key = infer.check_state(st)
        dims, L = _lib.Dims(*key), _lib.InferLayout()
        assert _lib.lib().gcnn_infer_layout_for(C.byref(dims), C.byref(L)) == 0
        where = list(L.in_off)[1:]
        got, want = np.full(L.in_bytes, 0xAB, np.uint8), np.full(L.in_bytes, 0xAB, np.uint8)
        scratch = infer.pack_state(got, got.ctypes.data, arrays, key, where, scratch)
        _restate(want, arrays, where)
        assert got.tobytes() == want.tobytes()
        assert scratch is None or (scratch.dtype == i32 and scratch.size >= max(key[0] if key[3] else 0, key[2] if key[4] else 0) + 1)
        assert infer._solo_layout(key)[2:5] == (L.in_off[0], L.in_off[1], tuple(where))


def test_pack_state_batch_layout():
    from gcnn_cut_selector_amd import _lib, infer
    checked = [infer.check_state(st) for st in _states()]
    n = len(checked)
    dims = (_lib.Dims * n)(*(_lib.Dims(*key) for _, key in checked))
    L = _lib.IbatchLayout()
    assert _lib.lib().gcnn_infer_batch_layout_for(n, dims, None, None, _lib.IBATCH_SCORES, C.byref(L)) == 0
    table = np.zeros(_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE, i32)
    assert _lib.lib().gcnn_infer_batch_fill_table(n, dims, None, None, table.ctypes.data) == 0
    off = table.reshape(_lib.IBATCH_TABLE_COLS, _lib.IBATCH_TABLE_STRIDE)
    in_off = list(L.in_off)
    got, want = np.full(L.in_bytes, 0xAB, np.uint8), np.full(L.in_bytes, 0xAB, np.uint8)
    session_where = infer._BatchSession(None)._layout(tuple(key for _, key in checked), (), _lib.IBATCH_SCORES).where
    scratch = None
    for s, (arrays, key) in enumerate(checked):
        where = tuple(in_off[2 + j] + STRIDES[j] * int(off[COLUMNS[j], s]) for j in range(7))
        assert session_where[s] == where
        scratch = infer.pack_state(got, got.ctypes.data, arrays, key, where, scratch)
        _restate(want, arrays, where)
    assert got.tobytes() == want.tobytes()
    # every state landed behind the one before it, inside its block
    for j in range(7):
        assert in_off[2 + j] + STRIDES[j] * int(off[COLUMNS[j], n]) <= (in_off[3 + j] if j < 6 else in_off[9])


def test_unsorted_list_comes_out_stably_sorted():
    from gcnn_cut_selector_amd import infer
    arrays, key = infer.check_state(_states()[1])
    kei, kef = arrays[5], arrays[6]
    E = kei.shape[1]
    sizes = [16 * key[0], 8 * key[3], 4 * key[3], 56 * key[1], 24 * key[2]]     # a dense layout of this test's own
    where = tuple(np.cumsum([0] + sizes).tolist()) + (sum(sizes) + 8 * E,)
    buf = np.zeros(where[6] + 4 * E, np.uint8)
    infer.pack_state(buf, buf.ctypes.data, arrays, key, where, None)
    inds = buf[where[5]:where[5] + 8 * E].view(i32).reshape(2, E)
    vals = buf[where[6]:where[6] + 4 * E].view(f32)
    perm = np.argsort(kei[0], kind="stable")
    assert np.all(np.diff(inds[0]) >= 0)
    assert np.array_equal(inds, kei[:, perm].astype(i32)) and np.array_equal(vals, kef.reshape(-1)[perm].astype(f32))


def test_check_state_messages():
    from gcnn_cut_selector_amd import infer
    st = list(_states()[0])
    st[5] = st[5].astype(np.int64)
    st[5][1, 0] = 2 ** 31
    with pytest.raises(ValueError) as e:
        infer.check_state(tuple(st))
    assert str(e.value) == "edge index out of range (left ids must be in [0,n_left), variable ids in [0,n_vars))" == infer.BAD_INDEX
    st = list(_states()[0])
    st[3] = st[3][:, :13]
    with pytest.raises(ValueError, match=r"var_feats must have shape \[N,14\], got \(\d+, 13\)"):
        infer.check_state(tuple(st))
    st = list(_states()[0])
    st[9] += 1
    with pytest.raises(ValueError, match=rf"n_cuts={st[9]} does not match the {st[9] - 1} feature rows"):
        infer.check_state(tuple(st))
    arrays, key = infer.check_state(_states()[0])
    assert key == (st[7], st[8], st[9] - 1, st[1].shape[1], st[5].shape[1]) and len(arrays) == 7
    assert infer.is_host_state(_states()[0])


def _same_rows(a, b):
    return len(a) == len(b) == 3 and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_normalize_forced_equals_pack_rows():
    from gcnn_cut_selector_amd import infer, ops
    fi, fv = np.array([[2, 0, 2, 1], [3, 1, 0, 4]], i32), np.array([0.5, -0.5, 1.0, 0.25], f32)
    assert _same_rows(infer.normalize_forced(None, 9), ops.pack_rows(np.zeros((2, 0), i32), np.zeros(0, f32), 0, 9))
    assert _same_rows(infer.normalize_forced((fi, fv), 9), ops.pack_rows(fi, fv, 3, 9))
    assert _same_rows(infer.normalize_forced((fi, fv, 5), 9), ops.pack_rows(fi, fv, 5, 9))
    empty = (np.zeros((2, 0), np.int64), np.zeros(0, np.float64))
    assert _same_rows(infer.normalize_forced(empty, 9), ops.pack_rows(empty[0], empty[1], 0, 9))
    ptr, col, val = infer.normalize_forced((fi, fv), 9)
    assert ptr.tolist() == [0, 1, 2, 4] and col.tolist() == [1, 4, 3, 0] and val.tolist() == [-0.5, 0.25, 0.5, 1.0]
    with pytest.raises(ValueError, match="forced rows"):
        infer.normalize_forced((fi, fv), 4)


def test_n_selected_and_stable_ranking():
    from gcnn_cut_selector_amd import infer
    for n_kept in (0, 1, 7):
        for ms in (None, 0, 3, 7, 100, 3.9):
            assert infer.n_selected(n_kept, ms) == (n_kept if ms is None else min(n_kept, int(ms)))
    scores = np.array([0.5, np.nan, 2.0, 0.5, -1.0, 2.0, 0.5], f32)
    got = infer.stable_ranking(scores.view(infer.ScoreArray))
    want = np.argsort(-np.asarray(scores), kind="stable").astype(np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert got.tolist()[:6] == [2, 5, 0, 3, 6, 4]          # ties in index order
    assert infer.stable_ranking(np.zeros(0, f32)).shape == (0,)
