"""The loss head, the Adam update in its four copies and the ranking metric (csrc/k_misc.hpp: k_mse, k_adam, k_adam_tick /
k_adam_dev, k_ranking; csrc/k_wgrad.hpp: the tail of reduce_body and `emit` in fold_block) restated in fp64, emulated in float32,
with the cases at the places where these kernels change path, the bounds a float32 evaluation has to meet, and planted defects.
Host only, NumPy only; tests/test_headcases.py proves on the host that the emulations stay inside every bound and that every
defect leaves it on a named case, tests/test_gpu_head_seams.py runs the cases on the device.

u = 2^-24 is the unit roundoff of float32, TINY = 2^-126 its smallest normal number: an operation whose result falls below the
normal range is off by at most TINY in absolute terms, whether the device keeps denormals or flushes them.

MSE head.  loss = scale * sum_k (s_k - t_k)^2, d_k = 2 * scale * (s_k - t_k).  k_mse is ONE block of 256 threads: thread i runs
over k = i, i + 256, ... with one fused multiply-add per element, an LDS tree of 8 levels sums the 256 thread sums, and the result is
scaled once.  Every term is non-negative, so a sum of them in any order, each term having passed through r roundings, is within
(1 + u)^r - 1 of the exact sum, relatively.  The roundings on the longest path, counted (MSE_K):
    2               d = fl(s - t) rounds once; it enters squared
    1               the product d * d, when the multiply-add is NOT contracted (the emulation's plain form; the kernel's fmaf has none)
    ceil(n / 256)   accumulations of one thread
    8               tree levels
    1               the scaling
so the relative bound is k * u / (1 - k * u) with k = ceil(n / 256) + 12 (`mse_bound`): 1.7e-6 at n = 4,097.  The float32 value of
`scale` is the one both sides use.  d is exact in another sense: the factor 2 is a power of two, so 2 * d * scale rounds once after
the subtraction, and the kernel's value is `mse_d32`, bit for bit.
Planted elements (`mse_planted`): index n - 1, 255, 256 and the last multiple of 256 carry errors of 0.5 .. 1.25 (MSE_PLANTS), all
other errors are 1e-2 * N(0, 1), as real improvements are.  One planted element is at least a twentieth of the whole sum at
every size here (the smallest, 0.25, beside the other three and 4,097 * 1e-4 = 0.41), three orders above ten times the bound.

Adam, Keras form (eps outside the square root), on the values the kernels receive -- float32 b1, b2, eps, lr_t and grad scale, and
1 - b formed in float32:
    gi = g * gs  (gs = *grad_scale, or 1 / *grad_scale when it is a divisor)        m' = b1 * m + (1 - b1) * gi
    v' = b2 * v + ((1 - b2) * gi) * gi                                              p' = p - lr_t * m' / (sqrt(v') + eps)
A divisor that is not > 0 makes the call a no-step: parameters, moments and the device's step counter stay.  `adam64` evaluates this
in fp64 (the divisor divides once there); `adam_bounds` gives, per slot, what a float32 evaluation may differ by.  With e_g the
roundings gi has behind it (0 without a scale, 1 with a factor, 2 with a divisor: the reciprocal and the product):
    |dm| <= u * (2 |b1 m| + (2 + e_g) |(1 - b1) gi|) + 3 TINY         each term: its product and the sum; gi's own on top
    |dv| <= u * (2 |b2 v| + (3 + 2 e_g) |(1 - b2) gi^2|) + 4 TINY      two products on the gradient term, gi enters twice
    |d sqrt(v)| <= min(|dv| / (2 sqrt(v)), sqrt(|dv|)) + u sqrt(v)
    |d upd| <= lr_t |dm| / den + |upd| (|d sqrt(v)| / den + 3 u)       den = sqrt(v') + eps; lr_t * m, + eps and the division round
    |d (p' - p)| <= |d upd| + half an ulp of p (taken at max(|p|, |p'|) + |d upd|) + TINY
A contracted multiply-add only removes roundings from these counts.  The bounds are first order; SLACK = 1 + 2^-10 on the u terms
covers the products of two errors (the largest relative error above is 7 u).  Slots whose fp64 value is NaN, infinite or exactly 0
are compared by class and sign instead (`adam_compare`).
Gradient classes (ADAM_CLASSES), rotating through the slots and by one slot per step, so that every slot meets every class and a zero
gradient follows an O(1) one (the moments decay and the parameter still moves): O(1); exactly 0; |g| = 1e-30 (g^2 underflows), 1e-9,
1e-7 (= eps), 1e-5; 1e19; 1e20; and NaN in one slot (ADAM_NAN_SLOT), which must stay in that slot.  (1e19)^2 = 1e38 is still finite
in float32, so 1e20 is there as well: its square overflows, and v' stays finite only because the kernels multiply (1 - b2) * gi
first, as the restatement does.
The device's lr_t (`tick64`: k_adam_tick evaluates lr * sqrt(1 - b2^t) / (1 - b1^t) in double from the float32 entries of its
state) and the host's (`tick_host`: Adam._tick, from the double betas) differ, because float32(0.999) is not 0.999:
d ln(1 - b^t) / db = -t b^(t-1) / (1 - b^t), whose magnitude grows with b, so over the interval between b and float32(b)
    |lr_host / lr_dev - 1| <= 0.5 * t b2^(t-1) |db2| / (1 - b2^t) + t b1^(t-1) |db1| / (1 - b1^t) + 3 u     (b: the larger of the two)
(`lr_gap_bound`; 3 u: lr and both results are rounded to float32).  At t = 1 that is 6.7e-6, the measured gap 6.4e-6, and the
largest over all t (t b^(t-1) / (1 - b^t) falls with t); at t = 1,000 the bound is 3.9e-6, at t = 100,000 it is the 3 u.  Each form is held to the restatement with its own lr_t.

Ranking metric.  `ranking(key)` is Python's sorted(range(n), key=..., reverse=True) after NaN -> -inf: descending, ties in index
order, +0.0 and -0.0 tied.  `fraction` is the first position where the two rankings differ over n, 0.0 for n = 0.  Everything is
exact: the device's fraction is float32(first) / float32(n), the credits are integers.  Two rankings of the same n entries that
agree on n - 1 positions agree on all, so the last position a first deviation can have is n - 2; the cases "last" and "one below
1.0" sit there.  k_ranking counts positions for n <= 256 (RK_COUNT) and sorts with a bitonic network above, padded to a power of two
with (-inf, 0x7fffffff) entries; `rank_emul` restates both in NumPy.

DEFECTS: the emulation with that one line changed; DEFECT_CASES names a case on which tests/test_headcases.py shows it caught."""
import functools
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10
THREADS = 256
_f32, _f64 = np.float32, np.float64

DEFECTS = {
    "mse": ("no_stride", "tree_short", "no_two", "scale_twice"),
    "adam": ("eps_inside", "betas_swapped", "g_not_squared", "scale_ignored", "divide_as_multiply", "cap_untouched",
             "zero_count_steps", "tick_prev", "moments_not_stored"),
    "ranking": ("ties_reverse", "nan_plus_inf", "negzero_below", "pad_first", "frac_padded", "gt_for_ge", "empty_credited"),
}


def cdiv(a, b):
    return -(-a // b)


# ---- MSE head --------------------------------------------------------------------------------------------------------------------------
MSE_SIZES = (0, 1, 255, 256, 257, 511, 512, 513, 4097)
MSE_SCALES = ("mean", "sum", "share")     # 1/n; 1.0 (the data-parallel sum); 1/(3n) (another rank's share)
MSE_PLANTS = (0.5, -0.75, 1.0, -1.25)


def mse_scale(kind, n):
    return {"mean": 1.0 / n if n else 0.0, "sum": 1.0, "share": 1.0 / (3 * n) if n else 0.0}[kind]


def mse_planted(n):
    return sorted(i for i in {n - 1, 255, 256, (n - 1) // THREADS * THREADS} if 0 <= i < n)


@functools.lru_cache(maxsize=None)
def mse_case(n):
    """(scores, targets) float32[n]."""
    rng = np.random.default_rng(1000 + n)
    t = rng.uniform(0.0, 0.2, n).astype(_f32)
    err = 1e-2 * rng.standard_normal(n)
    for i, e in zip(mse_planted(n), MSE_PLANTS):
        err[i] = e
    s = (t + err).astype(_f32)
    s.setflags(write=False), t.setflags(write=False)
    return s, t


def mse(scores, targets, scale):
    """(loss, d) in fp64 from the float32 inputs and the float32 value of `scale`."""
    d = np.asarray(scores, _f64) - np.asarray(targets, _f64)
    sc = float(_f32(scale))
    return sc * math.fsum(d * d), 2.0 * sc * d


def mse_d32(scores, targets, scale):
    return _f32(2) * (np.asarray(scores, _f32) - np.asarray(targets, _f32)) * _f32(scale)


def mse_k(n):
    return cdiv(n, THREADS) + 12


def mse_bound(n):
    """Relative bound on the loss (module docstring)."""
    k = mse_k(n)
    return k * U / (1.0 - k * U)


def _fma(a, b, c):
    """float32 fma through fp64: the product of two float32 values is exact there."""
    return (np.asarray(a, _f64) * np.asarray(b, _f64) + np.asarray(c, _f64)).astype(_f32)


def mse_emul(scores, targets, scale, fma=True, defect=None):
    """k_mse in float32 NumPy: (loss float32, d float32[n]); `fma=False`: product and sum rounded separately."""
    s, t, sc = np.asarray(scores, _f32), np.asarray(targets, _f32), _f32(scale)
    n = s.size
    d = s - t
    red = np.zeros(THREADS, _f32)
    dd = np.full(n, np.nan, _f32)
    for lo in range(0, n, THREADS):
        c = d[lo:lo + THREADS]
        red[:c.size] = _fma(c, c, red[:c.size]) if fma else red[:c.size] + c * c
        dd[lo:lo + THREADS] = (c if defect == "no_two" else _f32(2) * c) * sc
        if defect == "no_stride":
            break
    w = THREADS // 2
    while w > (1 if defect == "tree_short" else 0):
        red[:w] = red[:w] + red[w:2 * w]
        w >>= 1
    loss = red[0] * sc
    if defect == "scale_twice":
        loss = loss * sc
    return _f32(loss), dd


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
ADAM_MAX_BLOCKS = 1024
ADAM_CAP = ADAM_MAX_BLOCKS * THREADS      # 262,144: the first element of a thread's second trip
ADAM_SIZES = (1, 255, 256, 257, ADAM_CAP - 1, ADAM_CAP, ADAM_CAP + 1, 2 * ADAM_CAP + 1)
ADAM_CLASSES = ("O1", 0.0, 1e-30, 1e-9, 1e-7, 1e-5, 1e19, 1e20)
ADAM_STARTS = (0, 999, 99999)             # `iterations` before the first step; 0: zero moments
ADAM_SCALES = ("none", "factor", "divisor")
ADAM_COUNT = 37.0                         # the cut count of the scale settings
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7


def adam_nan_slot(n):
    return n // 3 if n > 1 else None


def adam_grad(n, step, with_nan=True):
    """float32[n]: slot i is of class (i + step) mod 8, signs and the O(1) values random."""
    rng = np.random.default_rng(77 * n + step + 1000)
    cls = (np.arange(n) + step) % len(ADAM_CLASSES)
    sign = rng.choice([-1.0, 1.0], n)
    g = rng.standard_normal(n)
    for c, val in enumerate(ADAM_CLASSES):
        if val != "O1":
            g = np.where(cls == c, sign * val, g)
    if with_nan and adam_nan_slot(n) is not None:
        g[adam_nan_slot(n)] = np.nan
    return g.astype(_f32)


def adam_start(n, iterations):
    """(p, m, v) float32[n] before the first step: zero moments at iterations 0, else moments as the previous step's gradient class
    leaves them."""
    rng = np.random.default_rng(5 * n + iterations)
    p = (0.1 * rng.standard_normal(n)).astype(_f32)
    p[p == 0] = _f32(0.1)
    if iterations == 0:
        return p, np.zeros(n, _f32), np.zeros(n, _f32)
    g = adam_grad(n, -1, with_nan=False).astype(_f64)
    return p, (0.5 * g).astype(_f32), (0.01 * g * g).astype(_f32)


def adam_scale(kind):
    """(grad_scale value or None, recip)"""
    return {"none": (None, False), "factor": (float(_f32(1.0) / _f32(ADAM_COUNT)), False), "divisor": (ADAM_COUNT, True)}[kind]


def _hyper(lr_t, b1, b2, eps):
    b1, b2 = _f32(b1), _f32(b2)
    return _f32(lr_t), b1, b2, _f32(eps), _f32(1) - b1, _f32(1) - b2


def _no_step(gscale, recip):
    return gscale is not None and recip and not float(_f32(gscale)) > 0.0


def adam64(p, g, m, v, lr_t, b1, b2, eps, gscale=None, recip=False):
    """One step in fp64 on the float32 values the kernels receive: (p', m', v')."""
    p, g, m, v = (np.asarray(a, _f64) for a in (p, g, m, v))
    if _no_step(gscale, recip):
        return p.copy(), m.copy(), v.copy()
    lr_t, b1, b2, eps, c1, c2 = (float(x) for x in _hyper(lr_t, b1, b2, eps))
    with np.errstate(all="ignore"):
        gi = g if gscale is None else (g / float(_f32(gscale)) if recip else g * float(_f32(gscale)))
        m2 = b1 * m + c1 * gi
        v2 = b2 * v + (c2 * gi) * gi
        p2 = p - lr_t * m2 / (np.sqrt(v2) + eps)
    return p2, m2, v2


def _ulp32(x):
    return np.spacing(np.minimum(np.abs(x), 3e38).astype(_f32)).astype(_f64)


def adam_bounds(p, g, m, v, lr_t, b1, b2, eps, gscale=None, recip=False):
    """(bound on m', on v', on p' - p), per slot (module docstring); nan where the fp64 values are not finite."""
    p, g, m, v = (np.asarray(a, _f64) for a in (p, g, m, v))
    lr_t, b1, b2, eps, c1, c2 = (float(x) for x in _hyper(lr_t, b1, b2, eps))
    eg = 0 if gscale is None else (2 if recip else 1)
    p2, m2, v2 = adam64(p, g, m, v, lr_t, b1, b2, eps, gscale, recip)
    if _no_step(gscale, recip):
        return np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)     # nothing is computed: the buffers stay bit for bit
    with np.errstate(all="ignore"):
        gi = g if gscale is None else (g / float(_f32(gscale)) if recip else g * float(_f32(gscale)))
        bm = SLACK * U * (2 * np.abs(b1 * m) + (2 + eg) * np.abs(c1 * gi)) + 3 * TINY
        bv = SLACK * U * (2 * np.abs(b2 * v) + (3 + 2 * eg) * np.abs(c2 * gi * gi)) + 4 * TINY
        root = np.sqrt(v2)
        den = root + eps
        upd = np.abs(lr_t * m2 / den)
        droot = np.minimum(np.where(root > 0, bv / (2 * np.where(root > 0, root, 1.0)), np.inf), np.sqrt(bv)) + SLACK * U * root
        bupd = lr_t * bm / den + upd * (droot / den + 3 * SLACK * U)
        bdp = bupd + 0.5 * _ulp32(np.maximum(np.abs(p), np.abs(p2)) + bupd) + TINY
    return bm, bv, bdp


def adam_compare(got, want, bound):
    """`got` (float32 values, as fp64) against `want` within `bound`, per slot; slots whose `want` is NaN, infinite or exactly 0 by
    class and sign.  Returns (largest error / bound over the ordinary slots, indices that fail)."""
    got, want, bound = (np.asarray(a, _f64) for a in (got, want, bound))
    special = ~np.isfinite(want) | (want == 0)
    with np.errstate(all="ignore"):
        same = np.where(np.isnan(want), np.isnan(got),
                        (got == want) & (np.signbit(got) == np.signbit(want)))
        err = np.abs(got - want)
        ratio = np.where(special | (err == 0), 0.0, err / bound)
        ok = np.where(special, same, np.isfinite(got) & (err <= bound))
    return float(ratio.max(initial=0.0)), np.flatnonzero(~ok)


def adam_emul(p, g, m, v, lr_t, b1, b2, eps, gscale=None, recip=False, form="plain", defect=None):
    """The kernels' update in float32 NumPy: (p', m', v') float32.  form: "plain" (every operation rounded), "fma" (the second
    product of each moment contracted into the sum), "fma2" (the first one)."""
    p, g, m, v = (np.asarray(a, _f32) for a in (p, g, m, v))
    if _no_step(gscale, recip) and defect != "zero_count_steps":
        return p.copy(), m.copy(), v.copy()
    lr_t, b1, b2, eps, c1, c2 = _hyper(lr_t, b1, b2, eps)
    if defect == "betas_swapped":
        b1, b2, c1, c2 = b2, b1, c2, c1
    with np.errstate(all="ignore"):
        gs = _f32(1)
        if gscale is not None and defect != "scale_ignored":
            gs = _f32(1) / _f32(gscale) if recip and defect != "divide_as_multiply" else _f32(gscale)
        gi = g * gs
        t2 = c2 * gi if defect == "g_not_squared" else (c2 * gi) * gi
        if form == "plain":
            mi, vi = b1 * m + c1 * gi, b2 * v + t2
        elif form == "fma":
            mi = _fma(c1, gi, b1 * m)
            vi = _fma(c2, gi, b2 * v) if defect == "g_not_squared" else _fma(c2 * gi, gi, b2 * v)
        else:
            mi, vi = _fma(b1, m, c1 * gi), _fma(b2, v, t2)
        root = np.sqrt(vi + eps) if defect == "eps_inside" else np.sqrt(vi) + eps
        pi = p - lr_t * mi / root
    if defect == "cap_untouched":
        pi[ADAM_CAP:], mi[ADAM_CAP:], vi[ADAM_CAP:] = p[ADAM_CAP:], m[ADAM_CAP:], v[ADAM_CAP:]
    if defect == "moments_not_stored":
        mi, vi = m.copy(), v.copy()
    return pi.astype(_f32), mi.astype(_f32), vi.astype(_f32)


def opt_state(iterations, lr=LR, b1=B1, b2=B2, eps=EPS):
    """The device form's state {lr, b1, b2, eps, t, lr_t} as Adam.apply_flat_dev creates it."""
    return np.array([lr, b1, b2, eps, float(iterations), 0.0], _f32)


def tick64(opt, shift=0):
    """lr_t of the step k_adam_tick is about to take, in fp64 from the float32 entries of `opt`."""
    lr, b1, b2, t = float(opt[0]), float(opt[1]), float(opt[2]), float(opt[4]) + 1.0 - shift
    with np.errstate(all="ignore"):
        return float(_f64(lr) * np.sqrt(_f64(1.0) - _f64(b2) ** t) / (_f64(1.0) - _f64(b1) ** t))


def tick_emul(opt, gscale=None, recip=False, defect=None):
    """k_adam_tick: the state after the tick."""
    out = np.array(opt, _f32)
    if _no_step(gscale, recip) and defect != "zero_count_steps":
        return out
    out[5] = _f32(tick64(opt, shift=1 if defect == "tick_prev" else 0))
    out[4] = _f32(float(opt[4]) + 1.0)
    return out


def tick_host(t, lr=LR, b1=B1, b2=B2):
    """Adam._tick's lr_t for step t (double betas), before it is rounded to float32 on its way into the kernel."""
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def lr_gap_bound(t, b1=B1, b2=B2):
    """Bound on |lr_host / lr_dev - 1| at step t (module docstring)."""
    def slope(b):
        hi = max(b, float(_f32(b)))
        return t * hi ** (t - 1) * abs(b - float(_f32(b))) / (1.0 - hi ** t)
    return 0.5 * slope(b2) + slope(b1) + 3 * U


# ---- ranking metric --------------------------------------------------------------------------------------------------------------------
RK_MAX = 4096
RK_COUNT = 256
RK_PAD_INDEX = 0x7FFFFFFF
FRACTIONS = (0.25, 0.5, 0.75, 1.0)
RANK_SIZES = (1, 2, 255, 256, 257, 512, 513, 4095, 4096)


def ranking(key):
    k = [-math.inf if math.isnan(x) else x for x in np.asarray(key, _f64).tolist()]
    return sorted(range(len(k)), key=lambda i: k[i], reverse=True)


def first_deviation(pred, truth):
    pr, tr = ranking(pred), ranking(truth)
    return next((i for i, (a, b) in enumerate(zip(pr, tr)) if a != b), len(pr))


def fraction(pred, truth):
    n = len(pred)
    return first_deviation(pred, truth) / n if n else 0.0


def frac32(pred, truth):
    n = len(pred)
    return _f32(first_deviation(pred, truth)) / _f32(n) if n else _f32(0)


def _before(va, ia, vb, ib, defect):
    return (va > vb) | ((va == vb) & ((ia > ib) if defect == "ties_reverse" else (ia < ib)))


def rank_emul(pred, truth, fractions=FRACTIONS, defect=None):
    """k_ranking for one sample in NumPy: (fraction float32, credits int[len(fractions)])."""
    fr = np.asarray(fractions, _f32)
    n = len(pred)
    credit = lambda frac: ((frac > fr) if defect == "gt_for_ge" else (frac >= fr)).astype(np.int64)
    if n <= 0:
        return (_f32(1), credit(_f32(1))) if defect == "empty_credited" else (_f32(0), np.zeros(fr.size, np.int64))

    def keyed(x):
        x = np.array(x, _f32)
        x[np.isnan(x)] = np.inf if defect == "nan_plus_inf" else -np.inf
        if defect == "negzero_below":
            x[(x == 0) & np.signbit(x)] = -_f32(1e-45)
        return x

    a, b = keyed(pred), keyed(truth)
    idx = np.arange(n)
    if n <= RK_COUNT:
        ra = _before(a[None, :], idx[None, :], a[:, None], idx[:, None], defect).sum(1)
        rb = _before(b[None, :], idx[None, :], b[:, None], idx[:, None], defect).sum(1)
        dev = ra[ra != rb]
        first, length = (int(dev.min()) if dev.size else n), n
    else:
        m = 1
        while m < n:
            m <<= 1
        lists = []
        for x in (a, b):
            val = np.concatenate([x, np.full(m - n, -np.inf, _f32)])
            ix = np.concatenate([idx, np.full(m - n, -1 if defect == "pad_first" else RK_PAD_INDEX)]).astype(np.int64)
            i = np.arange(m)
            k = 2
            while k <= m:
                j = k >> 1
                while j > 0:
                    lo = i[(i ^ j) > i]
                    hi = lo ^ j
                    up = (lo & k) == 0
                    swap = np.where(up, _before(val[hi], ix[hi], val[lo], ix[lo], defect), _before(val[lo], ix[lo], val[hi], ix[hi], defect))
                    s_lo, s_hi = lo[swap], hi[swap]
                    val[s_lo], val[s_hi] = val[s_hi], val[s_lo]
                    ix[s_lo], ix[s_hi] = ix[s_hi], ix[s_lo]
                    j >>= 1
                k <<= 1
            lists.append(ix[:n])
        dev = np.flatnonzero(lists[0] != lists[1])
        first, length = (int(dev[0]) if dev.size else n), (m if defect == "frac_padded" else n)
    frac = _f32(first) / _f32(length)
    return frac, credit(frac)


def rank_sample(n, first, seed=0):
    """(pred, truth) float32[n] without ties whose rankings first differ at position `first` (n: nowhere), ranks in shuffled slots."""
    assert first == n or 0 <= first <= n - 2
    rng = np.random.default_rng(31 * n + first + seed)
    truth = (0.5 * rng.permutation(n)).astype(_f32)
    pred = truth.copy()
    if first < n:
        order = np.argsort(-truth, kind="stable")
        i, j = order[first], order[first + 1]
        pred[i], pred[j] = truth[j], truth[i]
    return pred, truth


def _descending(n):
    return np.arange(n, 0, -1).astype(_f32)      # no ties; its ranking is the index order


@functools.lru_cache(maxsize=None)
def rank_cases():
    """name -> (pred, truth), insertion ordered.  Names ending in /c run the counting path, /n the network."""
    nan, inf = np.nan, np.inf
    out = {}
    for n in RANK_SIZES:
        out[f"size{n}"] = rank_sample(n, {1: 1, 2: 0}.get(n, n // 3))
    for tag, n in (("c", 40), ("n", 300)):
        d = _descending(n)
        out[f"ties/{tag}"] = (np.full(n, 1.5, _f32), d)                           # all tied: index order, as the truth's
        out[f"ties_both/{tag}"] = (np.full(n, 1.5, _f32), np.full(n, -2.0, _f32))
        out[f"zeros/{tag}"] = (np.where(np.arange(n) % 2, -0.0, 0.0).astype(_f32), d)  # +0.0 and -0.0 tie
        x = d.copy(); x[0], x[-1] = inf, -inf
        out[f"inf/{tag}"] = (x, d)                                                  # the same order with infinite ends
        x = d.copy(); x[:3] = inf
        out[f"inf_ties/{tag}"] = (x, d)                                             # three +inf tie in index order
        low = np.zeros(n, bool); low[n // 2:] = True                                # the lower half: NaN beside real -inf
        mixed = np.where(np.arange(n) % 3 == 0, nan, -inf).astype(_f32)
        x, y = d.copy(), d.copy()
        x[low], y[low] = mixed[low], -inf
        out[f"nan_pred/{tag}"] = (x, y)
        out[f"nan_truth/{tag}"] = (y, x)
        out[f"nan_both/{tag}"] = (x, np.where(low, mixed[::-1], d).astype(_f32))
        out[f"dev0/{tag}"] = rank_sample(n, 0)
        out[f"last/{tag}"] = rank_sample(n, n - 2)
        out[f"none/{tag}"] = rank_sample(n, n)
    out["nan_issue/c"] = (np.array([nan, -inf, 1], _f32), np.array([-inf, -inf, 1], _f32))
    for n in (257, 513):   # the entry both rank last is NaN / -inf for the prediction only: it must sort before the padding
        for tag, val in (("nan", nan), ("ninf", -inf)):
            d = _descending(n)
            x = d.copy(); x[-1] = val
            out[f"tail{n}_{tag}/n"] = (x, d)
    for tag, n in (("c", 16), ("n", 512)):
        for thr in FRACTIONS:
            on = int(thr * n)
            out[f"on{thr}/{tag}"] = rank_sample(n, on)
            out[f"below{thr}/{tag}"] = rank_sample(n, on - 1 if on < n else n - 2)
    p, t = rank_sample(256, 100, seed=9)
    out["twin256/c"] = (p, t)
    low = _f32(min(p.min(), t.min()) - 1)
    out["twin257/n"] = (np.append(p, low), np.append(t, low))
    for p, t in out.values():
        p.setflags(write=False), t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rank_batch():
    """The ragged batch: ordinary samples (integers 0..5, many ties), half of the cases, an empty sample, the other half, ordinary
    samples.  dict(names, pred, truth float32[total], n_cuts int64[samples])."""
    rng = np.random.default_rng(2024)
    ordinary = lambda k: {f"ordinary{k}_{i}": (rng.integers(0, 6, n).astype(_f32), rng.integers(0, 6, n).astype(_f32))
                          for i, n in enumerate((7, 33, 290))}
    cases = list(rank_cases().items())
    half = len(cases) // 2
    empty = (np.zeros(0, _f32), np.zeros(0, _f32))
    samples = list(ordinary(0).items()) + cases[:half] + [("empty", empty)] + cases[half:] + list(ordinary(1).items())
    return dict(names=[k for k, _ in samples], samples=[s for _, s in samples],
                pred=np.concatenate([s[0] for _, s in samples]), truth=np.concatenate([s[1] for _, s in samples]),
                n_cuts=np.array([len(s[0]) for _, s in samples], np.int64))


@functools.lru_cache(maxsize=None)
def rank_expected():
    """(fractions float32[samples], credits int64[samples, 4]) of `rank_batch` by the restatement."""
    b = rank_batch()
    fr = np.asarray(FRACTIONS, _f32)
    frac = np.array([frac32(p, t) for p, t in b["samples"]], _f32)
    credits = np.array([(f >= fr) if n else np.zeros(fr.size, bool) for f, n in zip(frac, b["n_cuts"])]).astype(np.int64)
    return frac, credits


# ---- readout gradient ------------------------------------------------------------------------------------------------------------------
SB_ROWS = 64
READOUT_CUTS = (63, 64, 65, 127, 128, 129)

# ---- a named case per defect: tests/test_headcases.py shows the defect leaves the bound (or changes an exact result) there --------------
DEFECT_CASES = {
    "no_stride": ("mse", 257, "mean"), "tree_short": ("mse", 256, "mean"), "no_two": ("mse", 1, "mean"), "scale_twice": ("mse", 513, "share"),
    "eps_inside": ("adam", 257, 0, "none"), "betas_swapped": ("adam", 257, 0, "none"), "g_not_squared": ("adam", 257, 999, "none"),
    "scale_ignored": ("adam", 257, 0, "factor"), "divide_as_multiply": ("adam", 257, 0, "divisor"),
    "cap_untouched": ("adam", ADAM_CAP + 1, 0, "none"), "zero_count_steps": ("adam", 257, 999, "zero"),
    "tick_prev": ("adam", 1, 999, "none"), "moments_not_stored": ("adam", 257, 0, "none"),
    "ties_reverse": ("ranking", "ties/c", "ties/n"), "nan_plus_inf": ("ranking", "nan_pred/c", "nan_truth/n"),
    "negzero_below": ("ranking", "zeros/c", "zeros/n"), "pad_first": ("ranking", "tail257_nan/n", "tail513_ninf/n"),
    "frac_padded": ("ranking", "size257", "twin257/n"), "gt_for_ge": ("ranking", "on0.25/c", "on1.0/n"),
    "empty_credited": ("ranking", "empty"),
}
