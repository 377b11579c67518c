"""The one case list of the host sanitizer run (helper for test_host_sanitizers.py): every size function, layout function, table
writer and host packer of include/gcnn_hip.h, as plain int32 records -- function id, word count, words -- which
tests/hostsan/hostsan_main.hip executes under ASan and UBSan and `run_ctypes` executes on the -O3 product library through the
binding.  Both write, per record, the return code and the raw bytes of what the library wrote; the test compares them.

Each integer field is swept one at a time around a base case over VALUES: 0, 1, 255, 256, 257, then L-1, L, L+1 for every limit
the header states (4,096 cuts, 32,768 variables, 2,048 edges per variable, 64 states, 8 models, 2^24 rows of a kind, 2^30 edges
of a set), INT32_MAX and -1; then all fields at their limits and all at INT32_MAX; counts of states, snapshots, members and
models at 0, 1, max, max + 1; null pointers.  No Cartesian product: about 10^4 records, a few seconds.

Run as a script (`python hostsancases.py --ctypes cases.bin results.bin`) it is the product-library side of the comparison, in
a process of its own so that it can run with every device hidden, as the sanitized program does: one size (the radix sort's
temporary storage, which rocprim sizes for the device it finds) would otherwise differ between the two where a GPU is present."""
from __future__ import annotations

import ctypes as C
import os
import struct
import sys

import numpy as np

INT32_MAX = 2 ** 31 - 1
LIMITS = (4096, 32768, 2048, 64, 8, 1 << 24, 1 << 30)
VALUES = sorted({0, 1, 255, 256, 257, INT32_MAX, -1} | {L + k for L in LIMITS for k in (-1, 0, 1)})
FILL = 0xA5
NULL_FIRST, NULL_NF, NULL_NFE, NULL_OUT, NULL_MODEL_OF = 1, 2, 4, 8, 16

# function id of every covered entry point (hostsan_main.hip's switch)
FUNCTIONS = {
    "gcnn_workspace_floats": 0, "gcnn_graph_temp_bytes": 1, "gcnn_select_workspace_bytes": 2, "gcnn_group_table_bytes": 3,
    "gcnn_param_info": 4, "gcnn_param_count": (5, 0), "gcnn_param_total_floats": (5, 1), "edges_without_nodes": 6,
    "gcnn_infer_layout_for": 10, "gcnn_infer_select_layout_for": 11, "gcnn_infer_batch_layout_for": 12,
    "gcnn_infer_models_layout_for": 13, "gcnn_infer_ensemble_layout_for": 14, "gcnn_infer_ensemble_batch_layout_for": 15,
    "gcnn_lp_layout_for": 16, "gcnn_lp_batch_layout_for": 17, "gcnn_lp_models_layout_for": 18, "gcnn_lp_collect_layout_for": 19,
    "gcnn_lp_rows_layout_for": 20, "gcnn_lp_round_layout_for": 21, "gcnn_lp_append_layout_for": 22, "gcnn_lp_remove_layout_for": 23,
    "gcnn_lp_rounds_layout_for": 24, "gcnn_lp_rounds_edit_layout_for": 25, "gcnn_lp_ensemble_layout_for": 26,
    "gcnn_lp_ensemble_batch_layout_for": 27, "gcnn_lp_round_ensemble_layout_for": 28, "gcnn_hybrid_layout_for": 29,
    "gcnn_infer_batch_fill_table": 30, "gcnn_infer_models_fill_table": 31, "gcnn_lp_batch_fill_table": 32,
    "gcnn_lp_models_fill_table": 33, "gcnn_hybrid_fill_table": 34,
    "gcnn_host_pack_edges": (40, 0), "gcnn_host_sort_edges_by_row": (40, 1),      # (id, first word): records of its own each
}
REFUSALS = 50
TABLE_CAP = 64 << 20
SKIPPED = -(2 ** 31)     # a table too large to allocate: both sides say so instead of writing

DIMS = (5, 6, 3, 7, 4)                                    # n_cons, n_vars, n_cuts, n_cons_edges, n_cut_edges
DIMS_AT_LIMIT = (1 << 24, 32768, 4096, 1 << 30, 1 << 30)
LP = (4, 6, 3, 9, 5, 1, 6, 5, 11, 0)                      # n_rows, n_cols, n_cuts, row_nnz, cut_nnz, has_incumbent, n_model_vars, C, E1, reserved
LP_AT_LIMIT = (1 << 23, 32768, 4096, 1 << 29, 1 << 30, 1, INT32_MAX, 1 << 24, 1 << 30, 0)
HYB = (6, 3, 5)                                           # n_cols, n_cuts, cut_nnz
HYB_AT_LIMIT = (1 << 24, 4096, 1 << 30)
APPEND = (2, 4, 3, 6, 1, 2, 2, 5)                         # n_rows, row_nnz, n_state_rows, n_state_edges, n_lhs_rows, n_lhs_edges, res_lhs_rows, res_lhs_edges
REMOVE = (1, 2, 1, 2, 0, 0, 2, 5)
NO_EDIT = (0,) * 8


def sweep(base, skip=()):
    """base with one field at a time at every value of VALUES, then every field at INT32_MAX."""
    out = [tuple(base)]
    for i in range(len(base)):
        if i not in skip:
            out += [tuple(base[:i]) + (v,) + tuple(base[i + 1:]) for v in VALUES]
    out.append(tuple(INT32_MAX if i not in skip else b for i, b in enumerate(base)))
    return out


def one(words, mask=0):
    return [mask, *words]


def many(items, nf=None, nfe=None, model_of=None, n=None, mask=0):
    k = len(items)
    w = [k if n is None else n, k, mask]
    for it in items:
        w += list(it)
    if nf is not None:
        w += list(nf) + list(nfe)
    if model_of is not None:
        w += list(model_of)
    return w


def _member(lp=LP, present=15, nf=-1, nfe=0, has_append=0, block=NO_EDIT, has_remove=None, removed=NO_EDIT):
    w = [*lp, present, nf, nfe, has_append, *block]
    return w if has_remove is None else w + [has_remove, *removed]


def _single_cases(fid, base, at_limit, tails, skip=()):
    """A layout of one struct: the sweep of its fields under the first tail, the limits under every tail, null pointers."""
    out = [(fid, one(d) + list(tails[0])) for d in sweep(base, skip)]
    for t in tails:
        out += [(fid, one(base) + list(t)), (fid, one(at_limit) + list(t))]
    out += [(fid, one(base, NULL_FIRST) + list(tails[0])), (fid, one(base, NULL_OUT) + list(tails[0]))]
    return out


def _many_cases(fid, base, at_limit, max_n, tails, models=False, skip=()):
    """A layout of several: the sweep in the second of two, the counts 0, 1, max, max + 1 (and INT32_MAX and -1 over one real
    entry), the union limits (two halves that pass them together), every tail, null pointers."""
    out = []
    z2 = lambda k: ([0] * k, [0] * k)  # noqa: E731
    mo = lambda k: ([0] * k if models else None)  # noqa: E731
    t0 = list(tails[0])
    for d in sweep(base, skip):
        out.append((fid, many([base, d], *z2(2), mo(2)) + t0))
    for k in (0, 1, max_n, max_n + 1):
        out.append((fid, many([base] * k, *z2(k), mo(k)) + t0))
    for n in (INT32_MAX, -1):
        out.append((fid, many([base], *z2(1), mo(1), n=n) + t0))
    for t in tails:
        out += [(fid, many([base, base], *z2(2), mo(2)) + list(t)), (fid, many([at_limit], *z2(1), mo(1)) + list(t)),
                (fid, many([at_limit, base], *z2(2), mo(2)) + list(t))]
    for mask in (NULL_FIRST, NULL_NF, NULL_NFE, NULL_NF | NULL_NFE, NULL_OUT) + ((NULL_MODEL_OF,) if models else ()):
        out.append((fid, many([base, base], *z2(2), mo(2), mask=mask) + t0))
    # forced rows: entries without a row, rows at their limits, negative counts
    for nf, nfe in ((0, 3), (1, 0), (2, 5), (1 << 24, 1 << 30), ((1 << 24) + 1, 0), (1, (1 << 30) + 1), (-1, 0), (1, -1), (INT32_MAX, INT32_MAX)):
        for t in tails:
            out.append((fid, many([base, base], [0, nf], [0, nfe], mo(2)) + list(t)))
    return out


def _pack_cases():
    out = []

    def rec(which, rows, n_left, cols=None, n_edges=None, mask=0, scratch=-1):
        k = len(rows)
        cols = list(range(k)) if cols is None else cols
        return (40, [which, k if n_edges is None else n_edges, n_left, k, mask, scratch, *rows, *cols])

    rng = np.random.default_rng(7)
    lists = {
        "sorted": ([0, 0, 1, 3, 3, 3, 4], 5), "unsorted": ([3, 0, 4, 1, 0, 3, 2], 5), "duplicates": ([2, 2, 0, 2, 0, 0, 2, 2], 3),
        "row -1": ([1, -1, 0], 3), "row n_left": ([1, 3, 0], 3), "sorted row n_left": ([0, 1, 3], 3), "sorted row -1": ([-1, 0, 1], 3),
        "empty": ([], 5), "empty no rows": ([], 0), "n_left 0 sorted": ([0, 0], 0), "n_left 0 unsorted": ([1, 0], 0),
        "one": ([0], 1), "last row only": ([256, 256, 256], 257), "long": (rng.integers(0, 257, 4097).tolist(), 257),
        "long sorted": (sorted(rng.integers(0, 4096, 2049).tolist()), 4096), "wide": ([5, 1 << 20, 0], (1 << 20) + 1),
    }
    for rows, n_left in lists.values():
        for which in (0, 1):
            out.append(rec(which, rows, n_left))
    for which in (0, 1):
        for mask in (1, 2, 4, 8, 16, 32, 63):                       # null-pointer combinations, with and without edges
            out += [rec(which, [1, 0, 2], 3, mask=mask), rec(which, [], 3, mask=mask), rec(which, [], 0, mask=mask)]
        out += [rec(which, [0, 1], 3, n_edges=-1), rec(which, [0, 1], -1), rec(which, [], -1), rec(which, [], 0, n_edges=-1)]
    # a sorted list never touches the scratch, whatever n_left is
    out += [rec(0, [0, 5, 9], v, scratch=1) for v in (1 << 24, (1 << 24) + 1, 1 << 30, INT32_MAX)]
    out += [rec(w, [3, 1, 2], 1 << 24) for w in (0, 1)]              # the counting sort over 2^24 rows: scratch of exactly 2^24 + 1 entries
    return out


# what a refusing entry point has to return (GCNN_E_BADARG -1, _WORKSPACE -2, _UNSUPPORTED -4), by entry and variant of
# hostsan_refusals.inc; the entries in its order
V = dict(short_arena=0, misaligned_arena=1, pmax_nan=2, pmax_inf=3, null_in=4, null_out=5, null_params=6, null_arena=7, n_zero=8, n_over=9,
         negative_dim=10, null_dims=11, null_staging=12, bad_mode=13, models_zero=14, models_over=15, short_workspace=16, null_misc=17)
REFUSAL_ENTRIES = ("gcnn_infer", "gcnn_infer_select", "gcnn_infer_batch", "gcnn_lp_infer", "gcnn_lp_infer_select", "gcnn_lp_batch",
                   "gcnn_hybrid_select", "gcnn_lp_collect", "gcnn_infer_models", "gcnn_lp_models", "gcnn_infer_ensemble", "gcnn_lp_ensemble",
                   "gcnn_infer_ensemble_batch", "gcnn_lp_ensemble_batch", "gcnn_select_cuts", "gcnn_rank_deviations", "gcnn_collate",
                   "gcnn_forward", "gcnn_forward_loss", "gcnn_backward", "gcnn_group_forward", "gcnn_group_train_step",
                   "gcnn_seg_sum_f32", "gcnn_seg_bcast_f32", "gcnn_linear_fwd", "gcnn_linear_bwd", "gcnn_conv_edge_fwd", "gcnn_conv_edge_bwd_recv",
                   "gcnn_conv_edge_bwd_send", "gcnn_adam_step", "gcnn_adam_step_dev", "gcnn_mse_loss", "gcnn_ranking_metric", "gcnn_ensemble_mean",
                   "gcnn_graph_check", "gcnn_graph_build", "gcnn_prenorm_stats", "gcnn_prenorm_merge", "gcnn_group_prenorm_merge", "gcnn_lp_state",
                   "gcnn_lp_rows_build", "gcnn_lp_round", "gcnn_lp_round_select", "gcnn_lp_rows_append", "gcnn_lp_round_append", "gcnn_lp_rows_remove",
                   "gcnn_lp_round_remove", "gcnn_lp_rounds", "gcnn_lp_rounds_edit", "gcnn_lp_round_ensemble")
# what the header declares besides: no launch, or nothing to refuse
NOT_LAUNCHING = ("gcnn_abi_version", "gcnn_profile_begin", "gcnn_profile_end")


def _refusal_cases():
    call = ["short_arena", "misaligned_arena", "null_in", "null_out", "null_arena", "negative_dim", "null_dims"]
    sel = ["pmax_nan", "pmax_inf"]
    several = ["n_zero", "n_over", "bad_mode"]
    ens = ["null_staging", "models_zero", "models_over"]
    want = {}
    for e in (0, 3):
        want[e] = {v: -1 for v in call + ["null_params"]}
    for e in (1, 4):
        want[e] = {v: -1 for v in call + ["null_params"] + sel}
    for e in (2, 5):
        want[e] = {v: -1 for v in call + ["null_params"] + sel + several}
    want[6] = {v: -1 for v in call + sel + several}
    want[7] = {v: -1 for v in call + sel}
    for e in (8, 9, 12, 13):
        want[e] = {v: -1 for v in call + ["null_params"] + sel + several + ens}
    for e in (10, 11):
        want[e] = {v: -1 for v in call + ["null_params"] + sel + ["bad_mode"] + ens}
    want[14] = dict(pmax_nan=-1, pmax_inf=-1, n_zero=-1, negative_dim=-1, null_misc=-1, bad_mode=-4, null_in=-1, null_out=-1, null_arena=-2,
                    short_workspace=-2)
    want[15] = dict(n_zero=-1, null_in=-1, null_out=-1, null_params=-1, models_over=-1, null_misc=-1)
    want[16] = dict(n_over=-1, n_zero=-1, negative_dim=-1, bad_mode=-1, null_misc=-1, null_in=-1, null_out=-1)
    for e in (17, 18, 19):
        want[e] = dict(null_dims=-1, null_params=-1, negative_dim=-1, null_misc=-1, null_arena=-2, short_workspace=-2)
    want[17]["null_out"] = want[18]["null_out"] = -1           # no scores buffer
    want[18]["null_in"] = -1                                   # no targets
    for e in (20, 21):
        want[e] = dict(n_zero=-1, n_over=-1, null_dims=-1, null_staging=-1, null_arena=-1, misaligned_arena=-1, short_arena=-2,
                       null_params=-1, negative_dim=-1, short_workspace=-2, null_out=-1)
    # the single ops, the optimiser, the metrics and the graph plan: a missing buffer with a positive count, a negative count
    bad = lambda *names: {v: -1 for v in names}  # noqa: E731
    want[22] = bad("null_in", "null_out", "negative_dim")
    want[23] = bad("null_in", "null_misc", "negative_dim")
    want[24] = bad("null_in", "null_out", "null_params", "negative_dim", "null_staging", "null_misc")    # bd without seg_ptr, xb without wb
    want[25] = bad("null_in", "null_out", "null_params", "negative_dim", "null_misc")                    # dx2 without wb
    want[26] = bad("null_in", "null_out", "null_params", "n_zero", "negative_dim", "null_misc")
    want[27] = bad("null_in", "null_out", "null_params", "negative_dim")
    want[28] = bad("null_in", "null_out", "null_params", "n_zero", "negative_dim", "null_misc")          # no n_parts
    want[29] = bad("null_in", "null_out", "null_params", "null_arena", "negative_dim")
    want[30] = bad("null_in", "null_out", "null_params", "null_arena", "negative_dim", "null_misc")      # no opt_state
    want[31] = bad("null_in", "null_params", "negative_dim")
    want[32] = {**bad("null_in", "null_out", "null_params", "n_zero", "negative_dim", "null_staging", "null_misc"), "bad_mode": -2}   # 4,097 cuts
    want[33] = bad("null_out", "null_params", "negative_dim", "models_zero", "models_over")
    want[34] = bad("null_in", "null_out", "negative_dim")
    want[35] = {**bad("null_in", "null_out", "null_arena", "n_zero", "negative_dim", "null_misc"), "short_workspace": -2}
    for e in (36, 37):
        want[e] = {**bad("null_out", "null_params", "negative_dim", "null_dims", "bad_mode", "null_misc"), "null_arena": -2, "short_workspace": -2}
    want[38] = {**bad("n_zero", "n_over", "null_dims", "null_in", "null_params", "null_staging", "null_arena", "misaligned_arena", "negative_dim",
                      "null_out", "null_misc", "bad_mode"), "short_arena": -2, "short_workspace": -2}     # layers, states, a misaligned state
    # the state from a snapshot and the calls on a resident LP
    want[39] = {**bad("null_in", "null_out", "null_arena", "negative_dim", "null_dims", "null_misc"), "short_workspace": -2}
    want[40] = {**bad("misaligned_arena", "null_in", "null_arena", "negative_dim", "null_dims"), "short_workspace": -2}
    round_call = ["short_arena", "misaligned_arena", "null_in", "null_out", "null_params", "null_arena", "negative_dim", "null_dims", "bad_mode", "null_misc"]
    want[41] = bad(*round_call)
    for e in (42, 44, 46):
        want[e] = bad(*round_call, *sel)
    for e in (43, 45):
        want[e] = {**bad("null_in", "null_out", "null_arena", "negative_dim", "null_dims", "null_misc"), "short_workspace": -2}
    for e in (47, 48):
        want[e] = bad("short_arena", "misaligned_arena", *sel, "null_in", "null_out", "null_params", "null_arena", "n_zero", "n_over", "negative_dim",
                      "null_dims", "null_staging", "bad_mode")
    want[49] = bad("short_arena", "misaligned_arena", *sel, "null_in", "null_out", "null_params", "null_arena", "negative_dim", "null_dims",
                   "null_staging", "bad_mode", "models_zero", "models_over", "null_misc")                    # one member's parameters missing
    return [(REFUSALS, [e, V[v], rc]) for e in sorted(want) for v, rc in want[e].items()]


def cases():
    """[(function id, [int32 words])] -- the whole list, in a fixed order."""
    out = []
    # ---- size functions
    out += [(0, one(d)) for d in sweep(DIMS)] + [(0, one(DIMS_AT_LIMIT)), (0, one(DIMS, NULL_FIRST))]
    out += [(1, [v]) for v in VALUES]
    out += [(2, list(t)) for t in sweep((3, 2, 3))] + [(2, [1 << 24, 1 << 24, 4096]), (2, [4096, 0, 4096]), (2, [4097, 0, 4097])]
    out += [(3, [n, 0]) for n in (0, 1, 8, 9, -1, INT32_MAX)] + [(3, [2, NULL_OUT])]
    out += [(4, [i, 0]) for i in (-1, 0, 1, 61, 62, INT32_MAX)] + [(4, [3, m]) for m in (1, 2, 4, 8, 15)]
    out += [(5, [0]), (5, [1])]
    out += [(6, one(d)) for d in ((0, 5, 5, 3, 5), (5, 0, 5, 0, 2), (5, 5, 0, 0, 1), DIMS, (0, 0, 0, 0, 0), (0, 0, 0, 1, 1))]
    # ---- layouts of one state or snapshot; every mode each takes
    modes = [(m,) for m in (0, 1, 2)] + [(3,), (-1,)]
    ens_tails = [(1, 2, m, k) for m in (2, 0, 1) for k in (2, 1, 8)] + [(1, 2, 2, k) for k in (0, 9, -1, INT32_MAX)] + [(1, 2, 3, 2), (1, 2, -1, 2)]
    forced = [(1, 2), (-1, 0), (0, 0), (0, 3), (1, -1), (1 << 24, 1 << 30), (INT32_MAX, INT32_MAX), (4096, 1 << 20)]
    out += _single_cases(10, DIMS, DIMS_AT_LIMIT, [()])
    out += _single_cases(11, DIMS, DIMS_AT_LIMIT, forced)
    out += _single_cases(14, DIMS, DIMS_AT_LIMIT, ens_tails)
    lp_skip = (5, 9)    # has_incumbent is a flag, reserved is not read
    out += _single_cases(16, LP, LP_AT_LIMIT, forced, lp_skip) + [(16, one(LP[:5] + (0,) + LP[6:]) + [1, 2])]
    out += _single_cases(19, LP, LP_AT_LIMIT, forced, lp_skip)
    out += _single_cases(20, LP, LP_AT_LIMIT, [()], lp_skip)
    round_tails = [(p, nf, nfe) for p in (15, 0, 5) for nf, nfe in ((-1, 0), (1, 2))] + [(16, -1, 0), (-1, -1, 0), (15, 0, 3), (15, 1, -1),
                                                                                       (15, 1 << 24, 1 << 30), (15, INT32_MAX, INT32_MAX)]
    out += _single_cases(21, LP, LP_AT_LIMIT, round_tails, lp_skip)
    for b in sweep(APPEND):
        out.append((22, one(LP) + one(b) + [15, 1, 2]))
    for d in sweep(LP, lp_skip):
        out.append((22, one(d) + one(APPEND) + [15, 1, 2]))
    for t in round_tails:
        out += [(22, one(LP) + one(APPEND) + list(t)), (22, one(LP_AT_LIMIT) + one(APPEND) + list(t))]
    out += [(22, one(LP, m1) + one(APPEND, m2) + [15, 1, 2]) for m1, m2 in ((NULL_FIRST, 0), (0, NULL_FIRST), (NULL_OUT, 0))]
    for m in sweep(REMOVE):
        out.append((23, one(LP) + one(m) + one(APPEND) + [15, 1, 2]))
    for b in sweep(APPEND):
        out.append((23, one(LP) + one(REMOVE) + one(b) + [15, 1, 2]))
    for d in sweep(LP, lp_skip):
        out.append((23, one(d) + one(REMOVE) + one(APPEND, NULL_FIRST) + [15, 1, 2]))
    for t in round_tails:
        out += [(23, one(LP) + one(REMOVE) + one(APPEND, k) + list(t)) for k in (0, NULL_FIRST)]
        out.append((23, one(LP_AT_LIMIT) + one(REMOVE) + one(APPEND, NULL_FIRST) + list(t)))
    out += [(23, one(LP, m1) + one(REMOVE, m2) + one(APPEND) + [15, 1, 2]) for m1, m2 in ((NULL_FIRST, 0), (0, NULL_FIRST), (NULL_OUT, 0))]
    out += _single_cases(26, LP, LP_AT_LIMIT, ens_tails, lp_skip)
    edit = lambda **kw: _member(has_remove=kw.pop("has_remove", 0), **kw)  # noqa: E731
    ens_round = [(m, k) for m in (2, 0, 1) for k in (2, 1, 8)] + [(2, 0), (2, 9), (2, -1), (2, INT32_MAX), (3, 2), (-1, 2)]
    members = [edit(nf=1, nfe=2), edit(), edit(nf=1, nfe=2, has_append=1, block=APPEND), edit(nf=1, nfe=2, has_remove=1, removed=REMOVE),
               edit(nf=1, nfe=2, has_append=1, block=APPEND, has_remove=1, removed=REMOVE), edit(lp=LP_AT_LIMIT, nf=1, nfe=2)]
    members += [edit(lp=d, nf=1, nfe=2) for d in sweep(LP, lp_skip)]
    members += [edit(nf=1, nfe=2, has_append=1, block=b) for b in sweep(APPEND)]
    members += [edit(nf=1, nfe=2, has_remove=1, removed=m) for m in sweep(REMOVE)]
    members += [edit(present=p, nf=nf, nfe=nfe) for p, nf, nfe in round_tails]
    for w in members:
        out.append((28, one(w) + [2 if w[11] >= 0 else 1, 2]))
    out += [(28, one(members[0]) + list(t)) for t in ens_round] + [(28, one(members[1]) + list(t)) for t in ens_round]
    out += [(28, one(members[0], m) + [2, 2]) for m in (NULL_FIRST, NULL_OUT)]
    # ---- layouts of several
    out += _many_cases(12, DIMS, DIMS_AT_LIMIT, 64, modes)
    mb_tails = [(m, 1) for m in (2, 0, 1)] + [(2, k) for k in (0, 2, 8, 9, -1, INT32_MAX)] + [(3, 1), (-1, 1)]
    out += _many_cases(13, DIMS, DIMS_AT_LIMIT, 64, mb_tails, models=True)
    eb_tails = [(m, k) for m in (2, 0, 1) for k in (2, 1, 8)] + [(2, k) for k in (0, 9, -1, INT32_MAX)] + [(3, 2), (-1, 2)]
    out += _many_cases(15, DIMS, DIMS_AT_LIMIT, 64, eb_tails)
    out += _many_cases(17, LP, LP_AT_LIMIT, 64, modes, skip=lp_skip)
    out += _many_cases(18, LP, LP_AT_LIMIT, 64, mb_tails, models=True, skip=lp_skip)
    out += _many_cases(27, LP, LP_AT_LIMIT, 64, eb_tails, skip=lp_skip)
    out += _many_cases(29, HYB, HYB_AT_LIMIT, 64, modes)
    # the models of the states: 8 models of 8 states, a decreasing list, an index out of range, a model without a state
    for fid, base in ((13, DIMS), (18, LP)):
        z = lambda k: ([0] * k, [0] * k)  # noqa: E731
        out.append((fid, many([base] * 64, *z(64), [s // 8 for s in range(64)]) + [2, 8]))
        out.append((fid, many([base] * 9, *z(9), list(range(9))) + [2, 9]))
        for mo, k in (([0, 1, 0], 2), ([0, 2], 2), ([-1, 0], 2), ([1, 1], 2), ([0, 2], 3), ([0, 0], 2), ([0, INT32_MAX], 2), ([0, 1], 2)):
            out.append((fid, many([base] * len(mo), *z(len(mo)), mo) + [2, k]))
    for fid, extra in ((24, {}), (25, {"has_remove": 0})):
        mem = lambda **kw: _member(**{**extra, **kw})  # noqa: E731
        plain, sel = mem(), mem(nf=1, nfe=2)
        for k in (0, 1, 8, 9):
            out += [(fid, many([sel] * k) + [2]), (fid, many([plain] * k) + [1])]
        out += [(fid, many([sel], n=n) + [2]) for n in (INT32_MAX, -1)]
        out += [(fid, many([plain, plain]) + [m]) for m in (0, 1, 3, -1)] + [(fid, many([sel, plain]) + [2]), (fid, many([sel, sel]) + [1])]
        for d in sweep(LP, lp_skip):
            out.append((fid, many([sel, mem(lp=d, nf=1, nfe=2)]) + [2]))
        for b in sweep(APPEND):
            out.append((fid, many([sel, mem(nf=1, nfe=2, has_append=1, block=b)]) + [2]))
        if fid == 25:
            for m in sweep(REMOVE):
                out.append((fid, many([sel, mem(nf=1, nfe=2, has_remove=1, removed=m)]) + [2]))
            out.append((fid, many([mem(nf=1, nfe=2, has_remove=1, removed=REMOVE, has_append=1, block=APPEND)] * 8) + [2]))
        for p, nf, nfe in round_tails:
            out.append((fid, many([sel, mem(present=p, nf=nf, nfe=nfe)]) + [2 if nf >= 0 else 1]))
        out += [(fid, many([sel, mem(lp=LP_AT_LIMIT, nf=1, nfe=2)]) + [2]), (fid, many([mem(lp=LP_AT_LIMIT)] * 8) + [0])]
        out += [(fid, many([sel, sel], mask=m) + [2]) for m in (NULL_FIRST, NULL_OUT)]
    # ---- table writers: every record of their layouts, and each with a null table
    layouts = list(out)
    for table, layout in ((30, 12), (31, 13), (32, 17), (33, 18), (34, 29)):
        for fid, w in layouts:
            if fid == layout and not w[2] & NULL_OUT:
                out.append((table, w + [0]))
        first = next(w for fid, w in layouts if fid == layout)
        out.append((table, first + [1]))
    out += _pack_cases()
    out += _refusal_cases()
    return out


def write_cases(path, records=None):
    records = cases() if records is None else records
    with open(path, "wb") as f:
        for fid, w in records:
            f.write(np.asarray([fid, len(w), *w], np.int64).astype(np.int32).tobytes())
    return records


def read_results(path):
    """[(return code, bytes)] as either executor wrote them."""
    blob, at, out = open(path, "rb").read(), 0, []
    while at < len(blob):
        rc, n = struct.unpack_from("<qq", blob, at)
        out.append((rc, blob[at + 16:at + 16 + n]))
        at += 16 + n
    return out


# ---- the same records on the product library, through the binding ---------------------------------------------------------------

class _Reader:
    def __init__(self, words):
        self.w, self.at = words, 0

    def i(self):
        self.at += 1
        return self.w[self.at - 1]

    def take(self, n):
        self.at += n
        return self.w[self.at - n:self.at]


def _filled(ctype):
    return ctype.from_buffer_copy(bytes([FILL]) * C.sizeof(ctype))


def _null(p, mask, bit):
    return None if mask & bit else p


def run_ctypes(records, out_path):
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()

    def lp_dims(w):
        return _lib.LpDims(*w, 1e20, 1e-6, 1.0)

    def hyb_dims(w):
        return _lib.HybridDims(*w, 0, 1e20)

    def member(cls, r):
        m = cls()
        m.dims = lp_dims(r.take(10))
        m.present, m.n_forced, m.n_forced_entries, m.has_append = r.take(4)
        m.block = _lib.LpAppendDims(*r.take(8))
        if cls is _lib.LpRoundsEditMember:
            m.has_remove = r.i()
            m.removed = _lib.LpRemoveDims(*r.take(8))
        return m

    readers = {"dims": lambda r: _lib.Dims(*r.take(5)), "lp": lambda r: lp_dims(r.take(10)), "hyb": lambda r: hyb_dims(r.take(3)),
               "append": lambda r: _lib.LpAppendDims(*r.take(8)), "remove": lambda r: _lib.LpRemoveDims(*r.take(8)),
               "member": lambda r: member(_lib.LpRoundsMember, r), "edit": lambda r: member(_lib.LpRoundsEditMember, r)}

    class One:
        def __init__(self, r, kind):
            self.mask = r.i()
            self.d = readers[kind](r)

        def ptr(self):
            return _null(C.byref(self.d), self.mask, NULL_FIRST)

        def out(self, L):
            return _null(C.byref(L), self.mask, NULL_OUT)

    class Many:
        def __init__(self, r, kind, forced=True, models=False):
            self.n, k, self.mask = r.take(3)
            items = [readers[kind](r) for _ in range(k)]
            self.d = (type(items[0]) * k)(*items) if k else (C.c_int32 * 1)()
            ints = lambda: (C.c_int32 * max(k, 1))(*r.take(k))  # noqa: E731
            self.nf, self.nfe = (ints(), ints()) if forced else (None, None)
            self.model_of = ints() if models else None

        def args(self):
            return self.n, _null(self.d, self.mask, NULL_FIRST), _null(self.nf, self.mask, NULL_NF), _null(self.nfe, self.mask, NULL_NFE)

        def mo(self):
            return _null(self.model_of, self.mask, NULL_MODEL_OF)

        def out(self, L):
            return _null(C.byref(L), self.mask, NULL_OUT)

    results = []

    def layout(ctype, call):
        L = _filled(ctype)
        rc = call(L)
        results.append((rc, bytes(L)))

    def table(layout_rc, nbytes, refused_bytes, null_table, call):
        if null_table:
            results.append((call(None), b""))
            return
        n = nbytes if layout_rc == 0 else refused_bytes
        if n > TABLE_CAP:
            results.append((SKIPPED, b""))
            return
        t = C.create_string_buffer(bytes([FILL]) * n, n)
        rc = call(t)
        results.append((rc, t.raw))

    size = lambda v: results.append((0, struct.pack("<Q", v)))  # noqa: E731
    for fid, words in records:
        r = _Reader(words)
        if fid == 0:
            a = One(r, "dims")
            size(lib.gcnn_workspace_floats(a.ptr()))
        elif fid == 1:
            size(lib.gcnn_graph_temp_bytes(r.i()))
        elif fid == 2:
            size(lib.gcnn_select_workspace_bytes(*r.take(3)))
        elif fid == 3:
            n, mask = r.take(2)
            v = _filled(C.c_size_t)
            results.append((lib.gcnn_group_table_bytes(n, _null(C.byref(v), mask, NULL_OUT)), bytes(v)))
        elif fid == 4:
            index, mask = r.take(2)
            v = _filled(C.c_int * 4)
            at = lambda k: None if mask & (1 << k) else C.cast(C.byref(v, 4 * k), C.POINTER(C.c_int))  # noqa: E731
            results.append((lib.gcnn_param_info(index, at(0), at(1), at(2), at(3)), bytes(v)))
        elif fid == 5:
            results.append((0, struct.pack("<i", lib.gcnn_param_total_floats() if r.i() else lib.gcnn_param_count())))
        elif fid == 6:     # a static of the library: restated here, there is no export to call
            d = One(r, "dims").d
            v = (d.n_cons_edges > 0 and (d.n_cons == 0 or d.n_vars == 0)) or (d.n_cut_edges > 0 and (d.n_cuts == 0 or d.n_vars == 0))
            results.append((0, struct.pack("<i", int(v))))
        elif fid == 10:
            a = One(r, "dims")
            layout(_lib.InferLayout, lambda L: lib.gcnn_infer_layout_for(a.ptr(), a.out(L)))
        elif fid == 11:
            a, t = One(r, "dims"), r.take(2)
            layout(_lib.SelectLayout, lambda L: lib.gcnn_infer_select_layout_for(a.ptr(), *t, a.out(L)))
        elif fid == 14:
            a, t = One(r, "dims"), r.take(4)
            layout(_lib.EnsembleLayout, lambda L: lib.gcnn_infer_ensemble_layout_for(a.ptr(), *t, a.out(L)))
        elif fid == 16:
            a, t = One(r, "lp"), r.take(2)
            layout(_lib.LpLayout, lambda L: lib.gcnn_lp_layout_for(a.ptr(), *t, a.out(L)))
        elif fid == 19:
            a, t = One(r, "lp"), r.take(2)
            layout(_lib.LpCollectLayout, lambda L: lib.gcnn_lp_collect_layout_for(a.ptr(), *t, a.out(L)))
        elif fid == 20:
            a = One(r, "lp")
            layout(_lib.LpRowsLayout, lambda L: lib.gcnn_lp_rows_layout_for(a.ptr(), a.out(L)))
        elif fid == 21:
            a, t = One(r, "lp"), r.take(3)
            layout(_lib.LpRoundLayout, lambda L: lib.gcnn_lp_round_layout_for(a.ptr(), *t, a.out(L)))
        elif fid == 22:
            a, b, t = One(r, "lp"), One(r, "append"), r.take(3)
            layout(_lib.LpAppendLayout, lambda L: lib.gcnn_lp_append_layout_for(a.ptr(), b.ptr(), *t, a.out(L)))
        elif fid == 23:
            a, m, b, t = One(r, "lp"), One(r, "remove"), One(r, "append"), r.take(3)
            layout(_lib.LpRemoveLayout, lambda L: lib.gcnn_lp_remove_layout_for(a.ptr(), m.ptr(), b.ptr(), *t, a.out(L)))
        elif fid == 26:
            a, t = One(r, "lp"), r.take(4)
            layout(_lib.LpEnsembleLayout, lambda L: lib.gcnn_lp_ensemble_layout_for(a.ptr(), *t, a.out(L)))
        elif fid == 28:
            a, t = One(r, "edit"), r.take(2)
            layout(_lib.LpRoundEnsembleLayout, lambda L: lib.gcnn_lp_round_ensemble_layout_for(a.ptr(), *t, a.out(L)))
        elif fid == 12:
            a, mode = Many(r, "dims"), r.i()
            layout(_lib.IbatchLayout, lambda L: lib.gcnn_infer_batch_layout_for(*a.args(), mode, a.out(L)))
        elif fid == 13:
            a, (mode, nm) = Many(r, "dims", models=True), r.take(2)
            layout(_lib.MbatchLayout, lambda L: lib.gcnn_infer_models_layout_for(*a.args(), mode, nm, a.mo(), a.out(L)))
        elif fid == 15:
            a, (mode, nm) = Many(r, "dims"), r.take(2)
            layout(_lib.EnsembleLayout, lambda L: lib.gcnn_infer_ensemble_batch_layout_for(*a.args(), mode, nm, a.out(L)))
        elif fid == 17:
            a, mode = Many(r, "lp"), r.i()
            layout(_lib.LpBatchLayout, lambda L: lib.gcnn_lp_batch_layout_for(*a.args(), mode, a.out(L)))
        elif fid == 18:
            a, (mode, nm) = Many(r, "lp", models=True), r.take(2)
            layout(_lib.LpModelsLayout, lambda L: lib.gcnn_lp_models_layout_for(*a.args(), mode, nm, a.mo(), a.out(L)))
        elif fid in (24, 25):
            a, mode = Many(r, "member" if fid == 24 else "edit", forced=False), r.i()
            n, d = a.args()[:2]
            d = None if d is None else C.cast(d, C.POINTER(_lib.LpRoundsMember if fid == 24 else _lib.LpRoundsEditMember))
            if fid == 24:
                layout(_lib.LpRoundsLayout, lambda L: lib.gcnn_lp_rounds_layout_for(n, d, mode, a.out(L)))
            else:
                layout(_lib.LpRoundsEditLayout, lambda L: lib.gcnn_lp_rounds_edit_layout_for(n, d, mode, a.out(L)))
        elif fid == 27:
            a, (mode, nm) = Many(r, "lp"), r.take(2)
            layout(_lib.LpEnsembleLayout, lambda L: lib.gcnn_lp_ensemble_batch_layout_for(*a.args(), mode, nm, a.out(L)))
        elif fid == 29:
            a, mode = Many(r, "hyb"), r.i()
            layout(_lib.HybridLayout, lambda L: lib.gcnn_hybrid_layout_for(*a.args(), mode, a.out(L)))
        elif fid == 30:
            a, (mode, null_table) = Many(r, "dims"), r.take(2)
            nb = 4 * _lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE
            table(0, nb, nb, null_table, lambda t: lib.gcnn_infer_batch_fill_table(*a.args(), t))
        elif fid == 31:
            a, (mode, nm, null_table) = Many(r, "dims", models=True), r.take(3)
            nb = 4 * _lib.MBATCH_TABLE_WORDS
            table(0, nb, nb, null_table, lambda t: lib.gcnn_infer_models_fill_table(*a.args(), nm, a.mo(), t))
        elif fid == 32:
            a, (mode, null_table) = Many(r, "lp"), r.take(2)
            L = _filled(_lib.LpBatchLayout)
            lrc = lib.gcnn_lp_batch_layout_for(*a.args(), mode, C.byref(L))
            table(lrc, L.table_bytes, 16, null_table, lambda t: lib.gcnn_lp_batch_fill_table(*a.args(), mode, t))
        elif fid == 33:
            a, (mode, nm, null_table) = Many(r, "lp", models=True), r.take(3)
            L = _filled(_lib.LpModelsLayout)
            lrc = lib.gcnn_lp_models_layout_for(*a.args(), mode, nm, a.mo(), C.byref(L))
            table(lrc, L.lp.table_bytes, 16, null_table, lambda t: lib.gcnn_lp_models_fill_table(*a.args(), mode, nm, a.mo(), t))
        elif fid == 34:
            a, (mode, null_table) = Many(r, "hyb"), r.take(2)
            L = _filled(_lib.HybridLayout)
            lrc = lib.gcnn_hybrid_layout_for(*a.args(), mode, C.byref(L))
            table(lrc, L.table_bytes, 16, null_table, lambda t: lib.gcnn_hybrid_fill_table(*a.args(), mode, t))
        elif fid == 40:
            which, n_edges, n_left, k, mask, scratch = r.take(6)
            scratch = n_left + 1 if scratch < 0 else scratch
            rows, cols = np.asarray(r.take(k), np.int32), np.asarray(r.take(k), np.int32)
            vals = (1.0 + 0.25 * np.arange(k)).astype(np.float32)
            oi, ov, sc = np.full(2 * k, FILL * 0x01010101, np.uint32), np.full(k, FILL * 0x01010101, np.uint32), np.zeros(max(scratch, 1), np.int32)
            p = [None if mask & (1 << b) else x.ctypes.data for b, x in enumerate((rows, cols, vals, oi, ov, sc))]
            fn = lib.gcnn_host_sort_edges_by_row if which else lib.gcnn_host_pack_edges
            results.append((fn(p[0], p[1], p[2], n_edges, n_left, p[3], p[4], p[5]), oi.tobytes() + ov.tobytes()))
        elif fid == REFUSALS:
            results.append((words[2], b""))     # the sanitized program alone makes these calls; it checks the code itself
        else:
            raise ValueError(fid)
        assert fid == REFUSALS or r.at == len(words), (fid, r.at, len(words))
    with open(out_path, "wb") as f:
        for rc, blob in results:
            f.write(struct.pack("<qq", rc, len(blob)) + blob)


def read_cases(path):
    w, at, out = np.fromfile(path, np.int32).tolist(), 0, []
    while at < len(w):
        out.append((w[at], w[at + 2:at + 2 + w[at + 1]]))
        at += 2 + w[at + 1]
    return out


if __name__ == "__main__":
    assert len(sys.argv) == 4 and sys.argv[1] == "--ctypes", sys.argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    run_ctypes(read_cases(sys.argv[2]), sys.argv[3])
