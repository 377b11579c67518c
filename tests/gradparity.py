"""Gradient parity against the fp64 oracle, with rounding-level ReLU flips proven instead of tolerated (helper for the GPU tests).

The kernels compute in fp32.  A ReLU pre-activation z within rounding of 0 can take the other branch there than in fp64; the
unit's whole share then moves the gradients (one column of its own layer's weight gradient, and through the backward pass every
tensor before it).  A tolerance wide enough to absorb that would also absorb a real defect of the same size, so a tensor beyond
the regular bound passes only if a flip is PROVEN: the fp64 oracle, with some set of ambiguous units forced onto the other
branch (oracle.ReluHook), must bring every tensor within the regular bound.

Ambiguous unit: |z| <= AMBIGUITY * u32 * m, with u32 = 2^-24 and m the sum of the absolute values of z's summands (the
oracle's record).  AMBIGUITY = 128 (AMBIGUITY * u32 = 7.6e-6): z is a dot product of at most 129 terms (output_module's first
layer: 128 inputs and the bias; the joint: 64 + 1 terms of the left projection, the edge term and 64 of the right one), so
the rounding of its own evaluation in any order stays below 129 * u32 * m (gamma_n, worst case) and is typically sqrt(n) * u32 *
m <= 12 * u32 * m; the relative error its inputs carry in from the fp32 layers before it (measured 2e-7 .. 5e-6 of each
tensor's largest entry on the parity cases) enters through the same |x| |W| products that make up m, and the headroom above 12
covers roughly 1e-6 of it.  Units beyond that are not rounding-level, and forcing them could hide a defect.
A large state has hundreds of units that close to 0 (7.6e-6 of the summands' magnitude); almost all of them are invisible: their
flip moves the gradients by less than rounding.  So a unit counts as ambiguous only if its flip is also VISIBLE: the first-order
change of its own layer's bias or kernel gradient (oracle.ReluHook: g, and g times the row's largest input) is at least
VISIBLE = 1e-5 of that tensor's largest entry, a tenth of the 1e-4 bound.  The filter only narrows which units may be forced;
what passes is still decided by the forced fp64 oracle meeting the regular bound on every tensor.
At most MAX_AMBIGUOUS = 4 ambiguous units are enumerated (16 flip sets, 15 oracle runs); more is a failure."""
from __future__ import annotations

import itertools

import numpy as np
import torch

from oracle import gcnn_oracle as O

U32 = 2.0 ** -24
AMBIGUITY = 128
MAX_AMBIGUOUS = 4
VISIBLE = 1e-5
assert AMBIGUITY * U32 <= 1e-5

NAMES = [n for n, _, t in O.PARAM_SPEC if t]


def _misses(got, want, gap, bound):
    """Tensors of `got` farther from `want` than bound(ref, fp32 gap): [(name, err, allowed)]."""
    out = []
    for name in NAMES:
        g, w = got[name], want[name]
        err = float(np.abs(g - w).max())
        allowed = bound(max(float(np.abs(w).max()), 1e-6), gap[name])
        if not err <= allowed:
            out.append((name, err, allowed))
    return out


def _layer_of(site):
    """(kernels, bias, bias factor) of the layer whose pre-activation a ReLU site reads."""
    if site.endswith("_joint"):
        conv = site[: -len("_joint")]
        return [f"{conv}_feat_left/kernel", f"{conv}_feat_right/kernel"], f"{conv}_feat_left/bias", f"{conv}_final_prenorm/scale"
    return [f"{site}/kernel"], f"{site}/bias", None


def ambiguous_units(params64, state, y, visible=True):
    """Units whose fp64 pre-activation lies within AMBIGUITY * u32 * m of 0 and (visible=True) whose flip is visible:
    [(site, row, col, z, m, effect)], largest effect first."""
    rec = O.ReluHook()
    _, _, want = O.loss_and_grads(params64, state, y, torch.float64, relu_hook=rec)
    units = []
    for site, (z, m) in rec.sites.items():
        near = z.abs() <= AMBIGUITY * U32 * m
        kernels, bias, bscale = _layer_of(site)
        g = rec.grads.get(site, torch.zeros_like(z)).abs()
        s = abs(float(params64[bscale].reshape(-1)[0])) if bscale else 1.0
        kref = min(max(float(np.abs(want[k]).max()), 1e-30) for k in kernels)
        bref = max(float(np.abs(want[bias]).max()), 1e-30)
        effect = torch.maximum(g * rec.rows[site][:, None] / kref, g * s / bref)
        hit = (near & (effect >= VISIBLE)) if visible else near
        units += [(site, r, c, float(z[r, c]), float(m[r, c]), float(effect[r, c])) for r, c in hit.nonzero().tolist()]
    return sorted(units, key=lambda u: -u[5])


def check(got, params, state, y, bound, want64=None):
    """`got`: name -> fp32 gradient of the kernels (numpy); `params`: the fp32 weights they ran with; `bound(ref, gap)`: the
    largest error allowed for a tensor whose largest fp64 entry is `ref` and whose fp32 restatement sits `gap` from fp64.
    `want64`: the fp64 gradients if already at hand (a golden fixture), else the oracle's.
    Returns the flip set that was needed ([] if none); raises AssertionError when no proof exists."""
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    got = {k: np.asarray(v, np.float64) for k, v in got.items()}
    if want64 is None:
        _, _, want64 = O.loss_and_grads(p64, state, y, torch.float64)
    _, _, want32 = O.loss_and_grads(params, state, y, torch.float32)
    gap = {n: float(np.abs(want32[n].astype(np.float64) - want64[n]).max()) for n in NAMES}
    bad = _misses(got, want64, gap, bound)
    if not bad:
        return []
    units = ambiguous_units(p64, state, y)
    assert len(units) <= MAX_AMBIGUOUS, (
        f"{len(bad)} gradient tensors beyond the bound ({bad[:4]}) and {len(units)} ambiguous ReLU units "
        f"(> {MAX_AMBIGUOUS}: not provable as rounding flips): {units[:8]}")
    for k in range(1, len(units) + 1):
        for subset in itertools.combinations(units, k):
            hook = O.ReluHook(force=[u[:3] for u in subset], record=False)
            _, _, forced = O.loss_and_grads(p64, state, y, torch.float64, relu_hook=hook)
            if not _misses(got, forced, gap, bound):
                return [u[:3] for u in subset]
    raise AssertionError(f"gradient tensors beyond the bound and no flip of the {len(units)} ambiguous ReLU units "
                         f"{[u[:3] for u in units]} explains them: {bad}")
