"""CPU checks of the removal's cases (tests/lpremovecases.py) and of its host half (`lpstate.rows_without`, `split_remove`,
`removal_counts`, `lp_remove_layout`): the NumPy restatement of the removal equals a state built from scratch on the kept rows,
every case moves a named array under each defect it is chosen against, every host check raises, the host's account of a removal
equals a recount, and the one upload has the size the contract gives it."""
import numpy as np
import pytest

import lpappendcases as A
import lpremovecases as D
from gcnn_cut_selector_amd import lpstate


@pytest.mark.parametrize("name", D.CPU_CASES)
def test_restatement_equals_a_state_built_from_scratch(name):
    c = D.case(name)
    old = A.resident(c.rows)
    want = A.resident(lpstate.rows_without(c.rows, c.idx))
    got = D.removed(old, c.rows, c.idx)
    assert D.moved(got, want) == [] and A.same_resident(got, want)


@pytest.mark.parametrize("name", D.CPU_CASES)
def test_every_case_moves_an_array_under_its_defects(name):
    c = D.case(name)
    assert set(c.against) <= set(D.DEFECTS)
    old = A.resident(c.rows)
    want = D.removed(old, c.rows, c.idx)
    for defect in c.against:
        assert D.moved(D.removed(old, c.rows, c.idx, defect), want), (name, defect)


def test_every_defect_is_held_against_some_case():
    held = {d for n in D.CPU_CASES for d in D.case(n).against}
    assert held == set(D.DEFECTS)


def test_rows_without():
    c = D.case("kinds")
    rows = c.rows
    ptr = np.asarray(rows.row_ptr)
    out = lpstate.rows_without(rows, [9, 5, 7])                 # any order
    keep = [r for r in range(40) if r not in (5, 7, 9)]
    assert np.array_equal(out.row_lhs, np.asarray(rows.row_lhs)[keep]) and np.array_equal(out.row_rhs, np.asarray(rows.row_rhs)[keep])
    assert out.row_ptr[0] == 0 and out.row_ptr.dtype == np.int32 and np.array_equal(np.diff(out.row_ptr), np.diff(ptr)[keep])
    for new, r in enumerate(keep):
        for name in ("row_col", "row_val"):
            assert np.array_equal(getattr(out, name)[out.row_ptr[new]:out.row_ptr[new + 1]], np.asarray(getattr(rows, name))[ptr[r]:ptr[r + 1]])
    assert out.col_type is rows.col_type and out.infinity == rows.infinity
    same = lpstate.rows_without(rows, [])
    assert np.array_equal(same.row_ptr, rows.row_ptr) and np.array_equal(same.row_col, rows.row_col)
    joined = lpstate.rows_with(rows, A.case("kinds").block)
    assert np.asarray(lpstate.rows_without(joined, [41]).row_lhs).shape[0] == np.asarray(joined.row_lhs).shape[0] - 1


def test_host_checks():
    block = A.case("kinds").block                                # 10 rows
    for bad, match in (([1.0, 2.0], "integers"), ([True], "integers"), ([-1], "outside"), ([40], "outside"), ([3, 3], "twice"),
                       (np.arange(40), "no row at all")):
        with pytest.raises(ValueError, match=match):
            lpstate.split_remove(bad, 40)
    with pytest.raises(ValueError, match="outside"):
        lpstate.split_remove([50], 40, block)                    # the indices number the rows after the append
    with pytest.raises(ValueError, match="no row at all"):
        lpstate.split_remove(np.arange(50), 40, block)
    idx, blk = lpstate.split_remove([7, 3, 5], 40)               # any order is accepted; the host sorts it
    assert idx.tolist() == [3, 5, 7] and blk is None
    for empty in (None, [], np.zeros(0, np.int64)):              # an empty list is no removal
        idx, blk = lpstate.split_remove(empty, 40, block)
        assert idx.size == 0 and blk is block


def test_indices_that_point_into_the_block_are_resolved_on_the_host():
    block = A.case("kinds").block
    idx, blk = lpstate.split_remove([41, 3, 49], 40, block)
    assert idx.tolist() == [3]
    want = lpstate.rows_without(A.block_rows(A.case("kinds").rows, block), [1, 9])
    for got, name in zip(blk.arrays(), ("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs")):
        assert np.array_equal(got, getattr(want, name)), name
    idx, blk = lpstate.split_remove(40 + np.arange(10), 40, block)           # a block that loses all its rows
    assert idx.size == 0 and blk is None
    idx, blk = lpstate.split_remove([41], 40, block)                          # only the block: the device sees no removal
    assert idx.size == 0 and np.asarray(blk.row_lhs).shape[0] == 9
    # the definition: remove from the joined rows
    rows = A.case("kinds").rows
    direct = lpstate.rows_without(lpstate.rows_with(rows, block), [41, 3, 49])
    idx, blk = lpstate.split_remove([41, 3, 49], 40, block)
    staged = lpstate.rows_with(lpstate.rows_without(rows, idx), blk)
    for name in ("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs"):
        assert np.array_equal(getattr(direct, name), getattr(staged, name)), name


@pytest.mark.parametrize("name", ("kinds", "free_only", "all_lhs", "all_rhs", "free_left", "one_left", "var_edges", "hub300", "seam_513_chunk0"))
def test_the_hosts_account_of_a_removal_equals_a_recount(name):
    c = D.case(name)
    rows = c.rows
    arrays, _ = lpstate.check_row_block(rows.row_ptr, rows.row_col, rows.row_val, rows.row_lhs, rows.row_rhs, np.asarray(rows.col_type).shape[0],
                                        rows.infinity)
    book = lpstate.row_book(arrays, rows.infinity)
    old = A.resident(rows)
    col_deg = np.diff(old["v_ptr"]).astype(np.int64)
    idx = np.sort(c.idx)
    six, new_book, deg, lhs, max_deg = lpstate.removal_counts(book, col_deg, (old["n_lhs"], old["n_lhs_edges"]), idx)
    kept = lpstate.rows_without(rows, idx)
    want = A.resident(kept)
    assert lhs == (want["n_lhs"], want["n_lhs_edges"]) and max_deg == (want["l_max_deg"], want["v_max_deg"])
    assert np.array_equal(deg, np.diff(want["v_ptr"])) and np.array_equal(col_deg, np.diff(old["v_ptr"]))      # (the input is not written)
    R0, C0, E0 = np.asarray(rows.row_lhs).shape[0], old["cons_static"].shape[0], old["edge_row"].shape[0]
    assert six == (idx.size, int(rows.row_ptr[-1]) - int(kept.row_ptr[-1]), C0 - want["cons_static"].shape[0], E0 - want["edge_row"].shape[0],
                   old["n_lhs"] - want["n_lhs"], old["n_lhs_edges"] - want["n_lhs_edges"])
    karr, _ = lpstate.check_row_block(kept.row_ptr, kept.row_col, kept.row_val, kept.row_lhs, kept.row_rhs, deg.shape[0], rows.infinity)
    for got, ref in zip(new_book, lpstate.row_book(karr, rows.infinity)):
        assert np.array_equal(got, ref)
    assert R0 - idx.size == new_book[0].shape[0]


def _dims(rows, rnd):
    _, row_dims = lpstate.check_rows(rows)
    _, present, dims = lpstate.check_round(rnd, row_dims, {}, True)
    return present, dims


@pytest.mark.parametrize("n", (1, 64, 65, 200))
def test_the_upload_is_the_inner_calls_plus_the_padded_list(n):
    c = D.case("seam_513_alternate")
    idx = np.sort(c.idx)[:n]
    rows = c.rows
    arrays, _ = lpstate.check_row_block(rows.row_ptr, rows.row_col, rows.row_val, rows.row_lhs, rows.row_rhs, 64, rows.infinity)
    old = A.resident(rows)
    lhs0 = (old["n_lhs"], old["n_lhs_edges"])
    six, _, deg, lhs, _ = lpstate.removal_counts(lpstate.row_book(arrays, rows.infinity), np.diff(old["v_ptr"]).astype(np.int64), lhs0, idx)
    kept = lpstate.rows_without(rows, idx)
    rnd = A._round_for(np.random.default_rng(3), kept, c.snap)
    present, after = _dims(kept, rnd)
    before = dict(after, n_rows=513, row_nnz=int(rows.row_ptr[-1]), n_state_rows=old["cons_static"].shape[0], n_state_edges=old["edge_row"].shape[0])
    pad = (4 * n + 255) // 256 * 256
    for nf, ne in ((-1, 0), (3, 6)):
        _, _, _, L = lpstate.lp_remove_layout(before, six + lhs0, None, present, nf, ne)
        _, plain = lpstate.lp_round_layout(after, present, nf, ne)
        assert L.list_bytes == pad and L.in_bytes == plain.in_bytes + pad and L.block_bytes == 0
        # with an append behind the removal: the fused call's upload for the dims after the removal
        blk = A.case("kinds").block
        barr, counts = lpstate.check_row_block(*blk.arrays(), 64, rows.infinity)
        dL, dEL, _, _ = lpstate.block_sides(barr, 64, rows.infinity)
        block8 = counts + (dL, dEL) + lhs
        rnd2 = A._round_for(np.random.default_rng(4), lpstate.rows_with(kept, blk), c.snap)
        present2, _ = _dims(lpstate.rows_with(kept, blk), rnd2)
        _, _, _, L2 = lpstate.lp_remove_layout(before, six + lhs0, block8, present2, nf, ne)
        _, _, fused = lpstate.lp_append_layout(after, block8, present2, nf, ne)
        assert L2.in_bytes == fused.in_bytes + pad and L2.block_bytes == fused.block_bytes
