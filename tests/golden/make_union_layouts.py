#!/usr/bin/env python3
"""Record every field of gcnn_ibatch_layout, gcnn_mbatch_layout and gcnn_lp_batch_layout, and the filled tables, for a fixed list
of unions into tests/golden/union_layouts.json.  The layouts are host arithmetic (no device): tests/test_union_layouts.py asserts
that the built library still returns exactly these, so a change to the shared layout code cannot move a byte unnoticed.

    python tests/golden/make_union_layouts.py        (at a commit whose layouts are known good)

A case is named call/union/mode/forced and holds (return code, layout, return code, table).  Structures are stored as the list of
their fields' values in declaration order (gcnn_cut_selector_amd/_lib.py).  Arrays are stored without their trailing zeros (an
all-zero structure counts as one), those of more than 16 entries as (length, sha256 of their JSON text), tables as (words,
sha256 of their bytes); the first 16 hex digits of each hash.  A case equal to an earlier one holds that case's name."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "union_layouts.json")

ONE, EMPTY, NO_CONS_EDGES = (5, 6, 3, 7, 4), (0, 0, 0, 0, 0), (5, 6, 3, 0, 4)
KINDS = (ONE, EMPTY, NO_CONS_EDGES)
# S in {1, 2, 64}: every kind alone, two pairs, all three in turn
UNIONS = [[k] for k in KINDS] + [[ONE, EMPTY], [NO_CONS_EDGES, ONE]] + [[KINDS[i % 3] for i in range(64)]]
# (states, model of every state): the unions above as one model, and the model lists of their own
MODELS = [(u, [0] * len(u)) for u in UNIONS] + [([ONE, NO_CONS_EDGES, ONE], [0, 0, 1]), ([KINDS[i % 3] for i in range(8)], list(range(8))),
                                                 ([KINDS[i % 3] for i in range(64)], [i // 8 for i in range(64)])]
FORCED = (2, 3)


def plain(x):
    """A ctypes value as JSON data: structures as the list of their fields' values, arrays as lists without their trailing zeros."""
    if isinstance(x, C.Structure):
        return [plain(getattr(x, name)) for name, _ in x._fields_]
    if isinstance(x, C.Array):
        items = [plain(v) for v in x]
        while items and (items[-1] in (0, 0.0) or (isinstance(items[-1], list) and not any(items[-1]))):
            items.pop()
        return items if len(items) <= 16 else [len(items), hashlib.sha256(json.dumps(items).encode()).hexdigest()[:16]]
    return x


def digest(table):
    return [int(table.size), hashlib.sha256(table.tobytes()).hexdigest()[:16]]


def _forced(n, forced):
    if not forced:
        return None, None
    return (C.c_int32 * n)(*[FORCED[0]] * n), (C.c_int32 * n)(*[FORCED[1]] * n)


def record():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    out = {}
    for mode in (0, 1, 2):
        for forced in (False, True):
            for i, shapes in enumerate(UNIONS):
                n = len(shapes)
                nf, nfe = _forced(n, forced)
                dims = (_lib.Dims * n)(*(_lib.Dims(*s) for s in shapes))
                L = _lib.IbatchLayout()
                rc = lib.gcnn_infer_batch_layout_for(n, dims, nf, nfe, mode, C.byref(L))
                table = np.full(_lib.IBATCH_TABLE_COLS * _lib.IBATCH_TABLE_STRIDE, -1, np.int32)
                rt = lib.gcnn_infer_batch_fill_table(n, dims, nf, nfe, table.ctypes.data)
                out[f"ibatch/u{i}/{mode}/{int(forced)}"] = [rc, plain(L), rt, digest(table)]
                # the same states built from LP snapshots
                lp = (_lib.LpDims * n)(*(_lib.LpDims(n_rows=c, n_cols=v, n_cuts=k, row_nnz=e1, cut_nnz=e2, has_incumbent=1,
                                                     n_model_vars=max(v, 1), n_state_rows=c, n_state_edges=e1, reserved=0,
                                                     infinity=1e20, sum_epsilon=1e-6, obj_norm=1.0) for c, v, k, e1, e2 in shapes))
                LL = _lib.LpBatchLayout()
                rc = lib.gcnn_lp_batch_layout_for(n, lp, nf, nfe, mode, C.byref(LL))
                table = np.full(LL.table_bytes // 4, -1, np.int32)
                rt = lib.gcnn_lp_batch_fill_table(n, lp, nf, nfe, mode, table.ctypes.data)
                out[f"lp_batch/u{i}/{mode}/{int(forced)}"] = [rc, plain(LL), rt, digest(table)]
            for i, (shapes, model_of) in enumerate(MODELS):
                n, n_models = len(shapes), model_of[-1] + 1
                nf, nfe = _forced(n, forced)
                dims = (_lib.Dims * n)(*(_lib.Dims(*s) for s in shapes))
                mos = (C.c_int32 * n)(*model_of)
                ML = _lib.MbatchLayout()
                rc = lib.gcnn_infer_models_layout_for(n, dims, nf, nfe, mode, n_models, mos, C.byref(ML))
                table = np.full(_lib.MBATCH_TABLE_WORDS, -1, np.int32)
                rt = lib.gcnn_infer_models_fill_table(n, dims, nf, nfe, n_models, mos, table.ctypes.data)
                out[f"mbatch/m{i}/{mode}/{int(forced)}"] = [rc, plain(ML), rt, digest(table)]
    first = {}          # a case that equals an earlier one (modes 0 and 1 mostly do) is stored as that case's name
    for name in sorted(out):
        same = first.setdefault(json.dumps(out[name]), name)
        if same != name:
            out[name] = same
    return out


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(record(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes")
