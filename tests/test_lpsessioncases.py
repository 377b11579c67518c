"""CPU checks of the resident-LP session's host side (lpstate.LPRows / LPRound / assemble, the checks and the two packers) and of
the session cases themselves (tests/lpsessioncases.py): each case sits on the seam it claims, the restated session equals the
restatement of the assembled snapshot, every case discriminates the defects it is chosen against, and a round's upload is the
full snapshot's minus the resident arrays (plus at most the 256 bytes of mask and alignment: derived, not measured)."""
import dataclasses

import numpy as np
import pytest

import lpcases
import lpsessioncases as S
import lpstate_restate as R
from gcnn_cut_selector_amd import lpstate, synthetic

ROUND_NAMES = [n for n, _ in lpstate.ROUND_FIELDS]
ROW_NAMES = [n for n, _ in lpstate.ROW_FIELDS]


def _snap_equal(a, b):
    for f in dataclasses.fields(lpstate.LPSnapshot):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            assert x is not None and y is not None and np.array_equal(np.asarray(x), np.asarray(y)), f.name
        else:
            assert x == y, f.name


@pytest.mark.parametrize("name", S.ROW_CASES + ("big_v",) + tuple(S.hand_names()))
def test_split_and_assemble_round_trip(name):
    snap = S.case(name)[1][2]
    rows, rnd = S.split(snap)
    back = lpstate.assemble(rows, rnd)
    inc = snap.scalars()[4]
    for f in dataclasses.fields(lpstate.LPSnapshot):
        x, y = getattr(snap, f.name), getattr(back, f.name)
        if f.name == "has_incumbent":
            assert y == inc
        elif f.name.startswith("col_primal") and not inc:
            assert y is None
        elif x is None or np.isscalar(x):
            assert x == y, f.name
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), f.name
    a, b = R.restate(snap), R.restate(back)
    assert S.same_state((a["inputs"], a["cut_index"]), (b["inputs"], b["cut_index"]))


def test_assemble_uses_kept_arrays_and_refuses_missing_ones():
    snap = lpcases.snapshot("rows255")
    rows, rnd = S.split(snap)
    bare = dataclasses.replace(rnd, col_ub=None, col_primal=None, has_incumbent=True)
    with pytest.raises(ValueError, match="col_ub"):
        lpstate.assemble(rows, bare)
    with pytest.raises(ValueError, match="col_primal"):
        lpstate.assemble(rows, bare, {"col_ub": snap.col_ub})
    _snap_equal(lpstate.assemble(rows, bare, {"col_ub": snap.col_ub, "col_primal": snap.col_primal}),
                dataclasses.replace(snap, has_incumbent=True))
    off = lpstate.assemble(rows, dataclasses.replace(rnd, has_incumbent=False))
    assert off.col_primal is None and off.col_primal_avg is None and off.has_incumbent is False


def test_packers_write_what_the_layouts_say():
    snap = lpcases.snapshot("rows257")
    rows, rnd = S.split(snap)
    arrays, rdims = lpstate.check_rows(rows)
    assert [a.dtype for a in arrays] == [np.dtype(dt) for _, dt in lpstate.ROW_FIELDS]
    full_arrays, full_dims = lpstate.check_snapshot(snap)
    assert {k: rdims[k] for k in ("n_rows", "n_cols", "row_nnz", "n_state_rows", "n_state_edges", "obj_norm")} == \
           {k: full_dims[k] for k in ("n_rows", "n_cols", "row_nnz", "n_state_rows", "n_state_edges", "obj_norm")}
    # a round: every array lands at its offset, the header carries the mask, an absent array takes no room
    for drop, have in (((), {}), (("col_ub", "col_primal_avg"), {"col_ub": 1, "col_primal_avg": 1})):
        r2 = dataclasses.replace(rnd, **{n: None for n in drop}, has_incumbent=True)
        got, present, dims = lpstate.check_round(r2, rdims, have)
        assert present == sum(1 << q for q, n in enumerate(lpstate.OPTIONAL) if n not in drop)
        assert dims == dict(full_dims, has_incumbent=1)
        _, L = lpstate.lp_round_layout(dims, present, 2, 5)
        off = list(L.in_off)
        buf = np.full(L.in_bytes, 0xEE, np.uint8)
        lpstate.pack_round(buf, off, got, present)
        assert buf[:4].view(np.int32)[0] == present and not buf[4:16].any()
        for o, nxt, a, name in zip(off[1:], off[2:] + [L.forced_off[0]], got, ROUND_NAMES):
            if a is None:
                assert nxt == o, name
                continue
            assert o % 16 == 0 and o + a.nbytes <= nxt
            assert np.array_equal(buf[o:o + a.nbytes].view(a.dtype), a), name
            assert np.array_equal(a, np.asarray(getattr(snap, name)).astype(a.dtype)), name
        f = list(L.forced_off)
        assert f[0] + 12 <= f[1] and f[1] + 20 <= f[2] and f[2] + 20 <= L.in_bytes
    # a block of rows: the first carries R + 1 offsets, an appended one R, shifted by the resident entries
    for first, base in ((True, 0), (False, 1234)):
        offs, total = lpstate.rows_upload_layout(rdims["n_rows"], rdims["row_nnz"], first)
        buf = np.zeros(total, np.uint8)
        places = lpstate.pack_row_block(buf, arrays[:5], base, first)
        ptr = buf[places[0][0]:places[0][0] + places[0][1]].view(np.int32)
        want = arrays[0] if first else arrays[0][1:]
        assert np.array_equal(ptr, want + base) and [o for o, _ in places] == offs
        for (o, n), a in zip(places[1:], arrays[1:5]):
            assert n == a.nbytes and np.array_equal(buf[o:o + n].view(a.dtype), a)
    with pytest.raises(ValueError, match="int32"):
        lpstate.pack_row_block(np.zeros(total, np.uint8), arrays[:5], 2 ** 31 - 10, False)


def test_none_rules_and_every_check_error():
    snap = lpcases.snapshot("rows255")
    rows, rnd = S.split(snap)
    _, rdims = lpstate.check_rows(rows)
    rep = dataclasses.replace
    for name in ("col_lb", "col_ub"):
        with pytest.raises(ValueError, match=f"{name}: the first round"):
            lpstate.check_round(rep(rnd, **{name: None}), rdims)
        assert lpstate.check_round(rep(rnd, **{name: None}), rdims, {name: 1})[0][ROUND_NAMES.index(name)] is None
    with pytest.raises(ValueError, match="col_primal: has_incumbent"):
        lpstate.check_round(rep(rnd, col_primal=None, has_incumbent=True), rdims)
    with pytest.raises(ValueError, match="col_primal_avg: has_incumbent"):
        lpstate.check_round(rep(rnd, col_primal_avg=None), rdims)
    arrays, present, dims = lpstate.check_round(rep(rnd, has_incumbent=False), rdims)           # without an incumbent: not looked at
    assert present == 3 and dims["has_incumbent"] == 0 and arrays[7] is None and arrays[8] is None
    arrays, present, dims = lpstate.check_round(rep(rnd, col_primal=None, col_primal_avg=None), rdims)
    assert present == 3 and dims["has_incumbent"] == 0
    V, Rn, K = rdims["n_cols"], rdims["n_rows"], np.asarray(rnd.cut_lhs).shape[0]
    bad = [(dict(row_dual=np.zeros(Rn + 1)), "row_dual"), (dict(row_basis=np.zeros(Rn - 1, np.int8)), "row_basis"),
           (dict(col_lp=np.zeros(V + 1)), "col_lp"), (dict(col_ub=np.zeros((V, 1))), "col_ub"), (dict(col_primal=np.zeros(3)), "col_primal"),
           (dict(cut_rhs=np.zeros(K + 1)), "cut_rhs"), (dict(cut_lhs=np.zeros((K, 1))), "cut_lhs"),
           (dict(row_basis=np.full(Rn, 4, np.int8)), "row_basis: codes"), (dict(col_basis=np.full(V, -1, np.int8)), "col_basis: codes"),
           (dict(cut_ptr=np.asarray(rnd.cut_ptr)[:-1]), "cut_ptr must hold"), (dict(cut_col=np.asarray(rnd.cut_col)[:-1]), "one length"),
           (dict(cut_col=np.where(np.arange(rnd.cut_col.size) == 3, V, rnd.cut_col)), "outside"),
           (dict(cut_col=np.asarray(rnd.cut_col, np.int64) + 2 ** 40), "does not fit int32")]
    for over, text in bad:
        with pytest.raises(ValueError, match=text):
            lpstate.check_round(rep(rnd, **over), rdims)
    with pytest.raises(ValueError, match="at least one entry"):       # (cut 0 emptied into cut 1: deep would object to the columns first)
        lpstate.check_round(rep(rnd, cut_ptr=np.concatenate([rnd.cut_ptr[:1], rnd.cut_ptr[:1], rnd.cut_ptr[2:]])), rdims, deep=False)
    swapped = np.array(rnd.cut_col)
    e = int(np.flatnonzero(np.diff(rnd.cut_ptr) >= 2)[0])
    swapped[[rnd.cut_ptr[e], rnd.cut_ptr[e] + 1]] = swapped[[rnd.cut_ptr[e] + 1, rnd.cut_ptr[e]]]
    with pytest.raises(ValueError, match="strictly increasing"):
        lpstate.check_round(rep(rnd, cut_col=swapped), rdims)
    lpstate.check_round(rep(rnd, cut_col=swapped), rdims, deep=False)                              # left to the device
    for over, text in ((dict(row_rhs=np.zeros(Rn + 1)), "row_rhs"), (dict(col_obj=np.zeros(V + 1)), "col_obj"),
                       (dict(col_type=np.full(V, 4, np.int8)), "col_type: codes"), (dict(infinity=0.0), "infinity"),
                       (dict(n_model_vars=0), "n_model_vars"), (dict(row_ptr=np.asarray(rows.row_ptr)[::-1].copy()), "row_ptr must rise"),
                       (dict(row_col=np.where(np.arange(rows.row_col.size) == 5, -1, rows.row_col)), "outside")):
        with pytest.raises(ValueError, match=text):
            lpstate.check_rows(rep(rows, **over))


@pytest.mark.parametrize("name", S.ROW_CASES)
def test_row_cases_sit_on_their_chunk_seams(name):
    snap = S.case(name)[1][2]
    lpcases.assert_seams(name, snap, lpcases.reference(name))
    place = S._places(np.asarray(snap.row_lhs), np.asarray(snap.row_rhs), snap.infinity)
    n = place.shape[0]
    for b in range(0, n, S.CHUNK):
        rows = np.arange(b, min(b + S.CHUNK, n))
        listed = place[rows]
        assert ((listed >= 0) & (listed != rows[:, None])).any(), "a chunk whose places all equal the LP row index"
    assert (place < 0).all(1).any() and (place >= 0).all(1).any()                 # a free row, a row listed twice


def test_sequence_cases_sit_on_their_seams():
    ks = [np.asarray(s[2].cut_lhs).shape[0] for s in S.case("k_sequence") if s[0] == "round"]
    assert tuple(ks) == S.K_SEQUENCE and [-(-k // S.CHUNK) for k in ks] == [3, 1, 0, 3, 5]
    for s in S.case("k_sequence")[1:]:
        lens = np.diff(s[2].cut_ptr)
        assert lens.size == 0 or (lens.min() >= 1 and lens.max() <= 40)
    steps = S.case("appends")
    counts = [np.asarray(s[2].row_lhs).shape[0] for s in steps if s[0] == "round"]
    assert counts == [249, 252, 255, 255, 257]
    blocks = [s[1] for s in steps if s[0] == "append"]
    inf = lpcases.INF
    fin = lambda x: lpstate.finite(np.asarray(x), inf)  # noqa: E731
    assert not fin(blocks[0][3]).any() and fin(blocks[0][4]).all()                # 3 rhs-only rows
    assert fin(blocks[1][3]).all() and fin(blocks[1][4]).sum() == 2               # 2 ranged, 1 lhs-only: rhs places shift
    assert np.asarray(blocks[2][3]).shape[0] == 0 and np.asarray(blocks[3][3]).shape[0] == 2
    rounds = [s for s in S.case("none_rules") if s[0] == "round"]
    gave = [[getattr(r[1], n) is not None for n in lpstate.OPTIONAL] for r in rounds]
    assert gave[0] == [True, True, False, False] and gave[2] == [False] * 4 and gave[3][1] and gave[4] == [False, False, True, False]
    assert [r[2].scalars()[4] for r in rounds] == [False, True, True, False, True, True]
    has_ub = [lpstate.finite(np.asarray(r[2].col_ub), inf) for r in rounds]
    assert (has_ub[0] != has_ub[1]).any() and np.array_equal(has_ub[1], has_ub[2]) and (has_ub[2] != has_ub[3]).any()
    assert np.array_equal(rounds[5][2].col_primal_avg, rounds[1][2].col_primal_avg)


@pytest.mark.parametrize("name", S.CPU_CASES)
def test_restated_session_equals_the_assembled_snapshot_and_discriminates(name):
    steps = S.case(name)
    good = S.restated(steps)
    refs = [R.restate(s[2]) for s in steps if s[0] == "round"]
    assert len(good) == len(refs)
    for got, ref in zip(good, refs):
        assert S.same_state(got, (ref["inputs"], ref["cut_index"]))
    for defect in S.AGAINST[name]:
        bad = S.restated(steps, defect)
        assert any(not S.same_state(b, g) for b, g in zip(bad, good)), (name, defect, S.DEFECTS[defect])


def test_every_defect_has_a_case():
    assert {d for ds in S.AGAINST.values() for d in ds} == set(S.DEFECTS)


def _resident_bytes(arrays):
    return sum(arrays[i].nbytes for i in (0, 1, 2, 3, 4, 7, 8))       # row_ptr .. row_rhs, col_type, col_obj of check_snapshot


def test_upload_bytes_are_the_snapshot_minus_the_resident_arrays():
    rows = []
    snaps = [(f"{p} sample 0", synthetic.make_lp_snapshot(p, 0)) for p in synthetic.PROBLEMS]
    for name in S.CPU_CASES + ("big_v",):
        snaps += [(f"{name} round {i}", s[2]) for i, s in enumerate(x for x in S.case(name) if x[0] == "round")]
    for label, snap in snaps:
        arrays, dims = lpstate.check_snapshot(snap)
        _, full = lpstate.lp_layout(dims, 0, 0)
        r, rnd = S.split(snap)
        _, rdims = lpstate.check_rows(r)
        _, present, d2 = lpstate.check_round(rnd, rdims)
        _, L = lpstate.lp_round_layout(d2, present, 0, 0)
        bound = full.in_bytes - _resident_bytes(arrays) + 256
        rows.append((label, int(full.in_bytes), int(L.in_bytes), bound))
        assert L.in_bytes <= bound, rows[-1]
    print("\nupload bytes: snapshot | full call | round | bound")
    for label, a, b, c in rows:
        print(f"  {label:24s} {a:10,d} {b:10,d} {c:10,d}")
