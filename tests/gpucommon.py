"""What the GPU test modules share: the device fixture, a model with the oracle's seeded random weights, and the fp64 oracle's
scores.  A module takes the fixture by importing `dev`; it stays module-scoped there."""
import numpy as np
import pytest
import torch

from oracle import gcnn_oracle as O  # (checker only)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def make_model(seed, dev, randomize_seed=None):
    """(model, params): the oracle's initial weights for `seed`, randomised with seed + 1 unless `randomize_seed` is given."""
    from gcnn_cut_selector_amd.model import GCNN
    params = O.randomize_params(O.init_params(seed, np.float32), seed + 1 if randomize_seed is None else randomize_seed)
    m = GCNN(device=dev)
    m.set_weights([params[n] for n in O.PARAM_NAMES])
    return m, params


def oracle_scores(params, state):
    return O.scores({k: v.astype(np.float64) for k, v in params.items()}, state, torch.float64)
