"""CPU checks of the test stage: the restatement of model_tester.test_model (tests/tester_restate.py) on hand-worked cases -- all ties,
one cut, improvements that tie in fp32 but not in fp64, a known shuffle -- and the host pieces of `tester.test_group` against it:
the random rankings, the host ranking of samples above 4,096 cuts, and the CSV / .npy outputs."""
import csv

import numpy as np
import pytest

import tester_restate as R
from gcnn_cut_selector_amd import synthetic


def _sample(improvements, efficacy, int_support=None, parallelism=None, dtype=np.float64):
    n = len(improvements)
    zero = np.zeros(n)
    cut = np.stack([zero, zero, zero if int_support is None else int_support, efficacy, zero,
                    zero if parallelism is None else parallelism], axis=1).astype(dtype)
    names = synthetic.FEATURE_NAMES
    state = ({"features": names["cons"], "values": np.zeros((1, 4))},
             {"features": names["edge"], "indices": np.zeros((2, 1), np.int64), "values": np.ones((1, 1))},
             {"features": names["var"], "values": np.zeros((1, 14))},
             {"features": names["cut"], "values": cut},
             {"features": names["edge"], "indices": np.stack([np.arange(n), np.zeros(n, np.int64)]), "values": np.ones((n, 1))})
    return state, np.asarray(improvements, np.float64)


# A: 5 cuts, distinct improvements, hybrid all tied; B: fp32-tied / fp64-distinct improvements; C: one cut; D: all ties
A = _sample([5, 4, 3, 2, 1], [0.5] * 5)
B = _sample([0.1, 0.1 + 1e-12, 0.05], [0.3, 0.2, 0.1])
C = _sample([0.7], [0.2])
D = _sample([0.5] * 4, [0.1] * 4, [1.0] * 4, [0.2] * 4)


def test_fp32_tie_is_fp64_distinct():
    imp = B[1]
    assert imp[0] != imp[1] and np.float32(imp[0]) == np.float32(imp[1])
    assert R.deviation(np.float32([0.3, 0.2, 0.1]), imp.astype(np.float32)) == 3   # fp32 truth: ties in index order
    assert R.deviation(np.float32([0.3, 0.2, 0.1]), imp) == 0                      # fp64 truth: cut 1 first


def test_hand_worked_cases():
    # seed 7: one draw for TensorFlow, then the shuffles [0, 1, 3, 2, 4], [0, 2, 1], [0] (PCG64, pinned below)
    preds = [np.float32([1, 2, 3, 4, 5, 0.3, 0.2, 0.1]), np.float32([9])]
    got = R.test_model([A, B, C], preds, [np.float32(0.5), np.float32(0.25)], seed=7, test_batch_size=2)
    assert got["random"] == (0.4 + 0 / 3 + 1.0) / 3       # A: deviates at 2; B: at 0 (fp64 truth ranks cut 1 first); C: never
    assert got["hybrid"] == (5 / 5 + 0 / 3 + 1 / 1) / 3   # A: all tied = index order = the truth; B: fp64 truth differs at 0
    assert got["gcnn"] == ((0 / 5 + 3 / 3) + 1 / 1) / 3   # B: the fp32 truth ties, so index order: the whole ranking agrees
    assert got["loss"] == (np.int32(8) * np.float32(0.5) + np.int32(1) * np.float32(0.25)) / 9
    assert isinstance(got["loss"], np.float64)


def test_all_ties_and_one_cut():
    got = R.test_model([D, C], [np.float32([0.7] * 4 + [1.0])], [np.float32(0)], seed=3, test_batch_size=4)
    assert got["gcnn"] == 1.0 and got["hybrid"] == 1.0
    rng = np.random.default_rng(3)
    rng.integers(np.iinfo(int).max)
    r = np.arange(4)
    rng.shuffle(r)
    assert got["random"] == (R.random_deviation(r, D[1]) / 4 + 1.0) / 2


def test_known_shuffle_and_driver_rankings():
    from gcnn_cut_selector_amd import tester
    want = [[0, 1, 3, 2, 4], [0, 2, 1], [0]]
    assert [r.tolist() for r in tester.random_rankings(7, [5, 3, 1])] == want
    assert [r.tolist() for r in tester.random_rankings(np.int64(7), np.array([5, 3, 1]))] == want
    rng = np.random.default_rng(7)
    rng.integers(np.iinfo(int).max)
    for n, w in zip((5, 3, 1), want):
        r = np.arange(n)
        rng.shuffle(r)
        assert r.tolist() == w


@pytest.mark.parametrize("n", [1, 2, 7, 300, 5000])
def test_host_ranking_matches_sorted(n):
    """The driver ranks samples above 4,096 cuts on the host: stable argsort of the negated key, as sorted(..., reverse=True)."""
    from gcnn_cut_selector_amd import tester
    rng = np.random.default_rng(n)
    for dtype in (np.float32, np.float64):
        for trial in range(3):
            true = rng.integers(0, 4, n).astype(dtype) * dtype(0.25)      # many ties
            pred = true.copy() if trial == 0 else rng.integers(0, 3 + trial, n).astype(dtype)
            assert tester._deviation(tester._order(pred), tester._order(true)) == R.deviation(pred, true)
            perm = rng.permutation(n)
            assert tester._deviation(perm, tester._order(true)) == R.random_deviation(perm, true)


def test_outputs_match_the_reference_writer(tmp_path):
    from gcnn_cut_selector_amd import tester
    seed = np.int64(123)
    want = {"loss": np.float64(0.0123456789), "gcnn": 2 / 3, "hybrid": np.float64(0.1) + np.float64(0.2), "random": 1e-05}
    R.write(str(tmp_path / "want"), seed, want)
    tester.write_results("setcov", seed, tester.GroupTestResult(want["loss"], want["gcnn"], want["hybrid"], want["random"], None),
                         root=str(tmp_path / "got"))
    folder = tmp_path / "got" / "results" / "test" / "setcov"
    assert (folder / "123.csv").read_bytes() == (tmp_path / "want" / "123.csv").read_bytes()
    with open(folder / "123.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert [r["type"] for r in rows] == ["random", "hybrid", "gcnn"]
    got, ref = np.load(folder / "123_loss.npy"), np.load(tmp_path / "want" / "123_loss.npy")
    assert got.dtype == ref.dtype == np.float64 and got.shape == ref.shape == () and got == ref


def test_hybrid_quality_in_the_sample_dtype():
    from gcnn_cut_selector_amd.store import hybrid_quality
    rng = np.random.default_rng(0)
    for dtype in (np.float32, np.float64):
        s = _sample(np.zeros(50), rng.random(50), rng.random(50), rng.random(50), dtype)
        got = hybrid_quality(s[0][3])
        want = R.hybrid_pred(s[0][3])
        assert got.dtype == want.dtype == dtype and np.array_equal(got, want)
    cut = dict(s[0][3], features=["rhs", "support", "int_support", "efficacy", "cutoff", "other"])
    assert hybrid_quality(cut) is None


def test_baselines_refused_with_a_process_group():
    from gcnn_cut_selector_amd.store import SampleStore
    with pytest.raises(ValueError, match="baselines"):
        SampleStore.from_files([], process_group=object(), baselines=True)


def test_problem_folders_are_the_reference_map():
    from gcnn_cut_selector_amd import tester
    assert tester.PROBLEM_FOLDERS == {'setcov': 'setcov/500r', 'combauc': 'combauc/100i_500b', 'capfac': 'capfac/100c_100f',
                                      'indset': 'indset/500n'}
    assert tester.RANK_MAX_CUTS == 4096
