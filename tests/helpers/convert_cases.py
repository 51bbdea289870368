"""Cases and bounds shared by the host checks (tests/test_score_convert.py, no GPU) and the device
checks (tests/test_device_custom_objective.py) of the objective output transforms of
src/device/score_convert.h (kinds 0..5 of ObjectiveFunction::DeviceOutputKind).

The bound between two evaluations of one transform (none of it is tuned to the code under test).
Write u = 2^-53 for the relative error of one correctly rounded double operation and E = 2^-52 for
that of an exp within 1 ulp (1 ulp of a value in [2^k, 2^(k+1)) is 2^(k-52), at most 2^-52 of the
value).  Both sides feed exp the same argument: -param * s and s - max are one rounding of the same
inputs, so they are the same bits.  A computed value is then its exact value times a product of
factors, each in [1 - E, 1 + E] (an exp) or [1 - u, 1 + u] (a rounding):

* kinds 0 and 2 (copy; sign(s) * s * s, two roundings of the same operands): no exp, the same
  operations on the same values -- equal bits.
* kind 3, exp(s): one exp factor per side.
* kinds 1 and 5, 1 / (1 + e) with e = exp(-param * s): the error of e reaches 1 + e scaled by
  e / (1 + e) <= 1, so one exp factor, then the add and the divide: two roundings per side.
* kind 4, softmax over K classes, e_k = exp(s_k - max), S the sum of e_k in class order, e_k / S:
  the numerator carries one exp factor; every term of S is positive and carries one exp factor and
  at most K - 1 roundings of the running sum, so S as a whole carries one exp factor and K - 1
  roundings; the divide adds one rounding: two exp factors and K roundings per side.

With a exp factors and r roundings per side, the ratio of the two sides lies between
((1 - E)^a (1 - u)^r)^2 and its inverse, so |x - y| <= rel(a, r) * min(|x|, |y|) with
rel(a, r) = (1 - E)^(-2a) (1 - u)^(-2r) - 1, evaluated below in exact rational arithmetic and
rounded up.  That holds for normal results.  A result in the subnormal range (exp(s) below 2^-1022,
a sigmoid of a score beyond 708 / param) is off by an absolute error instead: at most one
subnormal step 2^-1074 from the exp and half a step from the last rounding, per side; 2^-1072
covers both sides.  Where either side is infinite or NaN the two must agree exactly (both sides get
there by the same overflow: exp above 709.78 is +inf whatever its last bit).

Rows of a softmax sum to 1: each e_k / S is one rounding off the exact quotient of the computed
numbers, the computed S is at most K - 1 roundings off the exact sum of the computed e_k, and
summing the K results again costs at most K - 1 more: |sum - 1| <= (1 - u)^(-2K) - 1.
"""
import math
from fractions import Fraction

import numpy as np

_U = Fraction(1, 2 ** 53)
_E = Fraction(1, 2 ** 52)
ABS_FLOOR = 2.0 ** -1072

# (exp factors, roundings) per side; kind 4 takes the class count
_FACTORS = {0: (0, 0), 1: (1, 2), 2: (0, 0), 3: (1, 0), 5: (1, 2)}


def _up(fr):
    """a float >= the fraction"""
    x = float(fr)
    return x if Fraction(x) >= fr else math.nextafter(x, math.inf)


def rel_bound(kind, num_class=1):
    a, r = (2, num_class) if kind == 4 else _FACTORS[kind]
    if a == 0 and r == 0:
        return 0.0
    return _up((1 - _E) ** (-2 * a) * (1 - _U) ** (-2 * r) - 1)


def softmax_row_sum_bound(num_class):
    return _up((1 - _U) ** (-2 * num_class) - 1)


def assert_within_bound(got, ref, kind, num_class=1, what=""):
    """got / ref: float64 arrays of one shape, two evaluations of transform `kind`."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    special = ~(np.isfinite(got) & np.isfinite(ref))
    same_special = (got == ref) | (np.isnan(got) & np.isnan(ref))
    assert np.all(same_special[special]), "%s: non-finite results differ at %s" % (what, np.nonzero(special & ~same_special)[0][:8])
    rel = rel_bound(kind, num_class)
    if rel == 0.0:
        bad = ~special & (got.view(np.uint64) != ref.view(np.uint64))
        assert not bad.any(), "%s: kind %d must be bit-equal, differs at %s" % (what, kind, np.nonzero(bad.reshape(-1))[0][:8])
        return
    g, r = got[~special], ref[~special]
    err = np.abs(g - r)
    lim = rel * np.minimum(np.abs(g), np.abs(r)) + ABS_FLOOR
    worst = float(np.max(err / lim)) if err.size else 0.0
    print("%s kind %d K %d: rel bound %.3e, worst error / bound %.3f over %d values" % (what, kind, num_class, rel, worst, err.size))
    assert np.all(err <= lim), "%s: %d values beyond the bound, worst %.3f of it" % (what, int(np.sum(err > lim)), worst)


def reference(kind, param, scores):
    """The transform in plain float64 NumPy, written from the definitions (not from the header):
    scores [num_class, n] -> [num_class, n]."""
    s = np.asarray(scores, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == 0:
            return s.copy()
        if kind in (1, 5):
            return 1.0 / (1.0 + np.exp(-param * s))
        if kind == 2:
            return np.sign(s) * s * s
        if kind == 3:
            return np.exp(s)
        mx = np.max(s, axis=0, keepdims=True)
        e = np.exp(s - mx)
        total = np.zeros(s.shape[1])
        for k in range(s.shape[0]):  # (class order, as the rule sums)
            total = total + e[k]
        return e / total


def edge_scores(num_class, n_random=301, seed=5):
    """[num_class, n] raw scores: the named edge values in every class position against ordinary
    neighbours, rows of equal values, and random rows.  n is not a multiple of 64."""
    tiny = np.finfo(np.float64).tiny
    edges = [0.0, -0.0, tiny, -tiny, 5e-324, -5e-324, 700.0, -700.0, 745.2, -745.2, 709.9, -709.9, np.inf, -np.inf,
             1.0, -1.0, 36.8, -36.8]
    rng = np.random.RandomState(seed)
    cols = []
    for v in edges:
        for pos in range(num_class):
            c = rng.uniform(-3, 3, size=num_class)
            c[pos] = v
            cols.append(c)
        cols.append(np.full(num_class, v))
    cols.append(np.array([700.0 if k % 2 == 0 else -700.0 for k in range(num_class)]))
    body = np.stack(cols, axis=1) if cols else np.zeros((num_class, 0))
    rand = rng.normal(0, 4, size=(num_class, n_random))
    out = np.concatenate([body, rand], axis=1)
    if out.shape[1] % 64 == 0:
        out = np.concatenate([out, rng.normal(0, 1, size=(num_class, 1))], axis=1)
    return np.ascontiguousarray(out)
