"""The layouts and tables of the three union calls (gcnn_infer_batch, gcnn_infer_models, gcnn_lp_batch) are byte for byte the
recorded ones (tests/golden/union_layouts.json, written by tests/golden/make_union_layouts.py): every field, for S in {1, 2, 64},
an ordinary state, an all-zero one and one without constraint edges, every mode with and without forced rows, one to eight models."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_layouts_and_tables_equal_the_recorded_ones():
    spec = importlib.util.spec_from_file_location("make_union_layouts", os.path.join(GOLDEN, "make_union_layouts.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(gen.PATH))
    got = json.loads(json.dumps(gen.record()))
    assert sorted(got) == sorted(want) and len(want) == 3 * 2 * (2 * len(gen.UNIONS) + len(gen.MODELS))
    assert all(isinstance(v, str) or (v[0] == 0 and v[2] == 0) for v in want.values())      # the library takes every recorded case
    for case in sorted(want):
        assert got[case] == want[case], case
