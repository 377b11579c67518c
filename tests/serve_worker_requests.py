"""The requests the workers of tests/test_gpu_serve.py send (NumPy only): shared by the worker script and the test that checks them."""
from gcnn_cut_selector_amd import synthetic, utils

PROBLEMS = ("setcov", "combauc", "capfac", "indset")
N_REQUESTS = 20


def request(wid, j):
    """(model key, kind, state, thresholds) of worker wid's j-th request: kinds cycle score / rank / select, the model key and the
    selection thresholds change every three requests."""
    state, _ = synthetic.make_sample(PROBLEMS[(wid + j) % 4], 200 + 20 * wid + j, scale=0.2)
    return ("a", "b")[(wid + j // 3) % 2], j % 3, utils.state_to_inputs(state), ((0.1, 0.5), (0.3, 0.6))[(j // 3) % 2]
