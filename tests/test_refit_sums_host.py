"""Refit on the device, the parts that need no GPU.

* LGBM_AMD_RefitLeafSums evaluates the fixed-point rule of the leaf-sum kernel
  (src/device/refit_quant.h, shared with src/device/refit_kernels.hip) on the host.  It is checked
  against exact per-leaf sums of the fp32 inputs (Python integers).  A row is rounded once, to a
  multiple of 2^-scale_exp, and the integer sums are exact, so
  |sum - exact| <= count_leaf * 2^-(scale_exp + 1); counts are exact; empty leaves give (0, 0, 0).
* The leaf-output formula the CPU learner and the device refit share (RefitLeafOutputs): the CPU
  learner's refit of a stored model gives the model text it gave before the formula was factored
  out (tests/golden/refit_cpu_*.txt), and a three-leaf case is computed by hand.
"""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_EPSILON = 1e-15


def host_leaf_sums(leaf, grad, hess, num_leaves):
    """(sum_g, sum_h, count, scale_exp) of LGBM_AMD_RefitLeafSums"""
    leaf = np.ascontiguousarray(leaf, dtype=np.int32)
    grad = np.ascontiguousarray(grad, dtype=np.float32)
    hess = np.ascontiguousarray(hess, dtype=np.float32)
    sums = np.full(2 * num_leaves, 7.0)
    counts = np.full(num_leaves, -1, dtype=np.int64)
    exps = np.zeros(2, dtype=np.int32)
    nat.call("LGBM_AMD_RefitLeafSums", leaf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
             grad.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), hess.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
             ctypes.c_int64(len(leaf)), ctypes.c_int32(num_leaves), sums.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
             counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), exps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return sums[:num_leaves], sums[num_leaves:], counts, exps


def exact_leaf_sums(leaf, values, num_leaves):
    """per-leaf sums of fp32 values as exact integers in units of 2^-149 (every finite fp32 is one)"""
    ints = [int(x) for x in np.ldexp(values.astype(np.float64), 149)]  # (exact: a double holds fp32 * 2^149)
    out = [0] * num_leaves
    for l, v in zip(leaf.tolist(), ints):
        out[l] += v
    return out


def check_against_exact(leaf, grad, hess, num_leaves, result):
    sum_g, sum_h, count, exps = result
    assert np.array_equal(count, np.bincount(leaf, minlength=num_leaves))
    for got, values, e in ((sum_g, grad, int(exps[0])), (sum_h, hess, int(exps[1]))):
        exact = exact_leaf_sums(leaf, values, num_leaves)
        for l in range(num_leaves):
            err = abs(Fraction(float(got[l])) - Fraction(exact[l], 1 << 149))
            assert err <= int(count[l]) * Fraction(2) ** -(e + 1), (l, float(got[l]), e)
            if count[l] == 0:
                assert got[l] == 0.0
    # the scale: n * max * 2^e < 2^53 < 2^62, a power of two by construction
    n = len(leaf)
    for values, e in ((grad, int(exps[0])), (hess, int(exps[1]))):
        m = Fraction(float(np.max(np.abs(values)))) if n else Fraction(0)
        assert n * m * Fraction(2) ** e < 2 ** 53


def columns(n, seed):
    """leaf ids and gradients with magnitudes from 1e-6 to 1e3 in one column, hessians partly negative"""
    rs = np.random.RandomState(seed)
    grad = (rs.randn(n) * 10.0 ** rs.uniform(-6, 3, n)).astype(np.float32)
    grad[0] = np.float32(1e3)
    if n > 1:
        grad[1] = np.float32(1e-6)
    hess = (rs.rand(n) * 10.0 ** rs.uniform(-6, 3, n) * np.where(rs.rand(n) < 0.3, -1.0, 1.0)).astype(np.float32)
    return rs, grad, hess


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
@pytest.mark.parametrize("num_leaves", [1, 7, 64])
def test_leaf_sums_within_the_rounding_bound(n, num_leaves):
    rs, grad, hess = columns(n, 100 + n)
    leaf = rs.randint(0, num_leaves, n).astype(np.int32)
    check_against_exact(leaf, grad, hess, num_leaves, host_leaf_sums(leaf, grad, hess, num_leaves))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_all_zero_gradients_give_a_finite_scale(n):
    leaf = (np.arange(n) % 5).astype(np.int32)
    z = np.zeros(n, dtype=np.float32)
    sum_g, sum_h, count, exps = host_leaf_sums(leaf, z, z, 5)
    assert np.all(sum_g == 0.0) and np.all(sum_h == 0.0)
    assert np.array_equal(count, np.bincount(leaf, minlength=5))
    assert abs(int(exps[0])) < 1000 and abs(int(exps[1])) < 1000


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_negative_hessians_keep_their_sign(n):
    rs, grad, hess = columns(n, 200 + n)
    hess = -np.abs(hess) - np.float32(0.5)
    leaf = rs.randint(0, 3, n).astype(np.int32)
    res = host_leaf_sums(leaf, grad, hess, 3)
    check_against_exact(leaf, grad, hess, 3, res)
    assert np.all(res[1][res[2] > 0] < 0.0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_every_row_in_one_leaf(n):
    rs, grad, hess = columns(n, 300 + n)
    for only in (0, 8):
        leaf = np.full(n, only, dtype=np.int32)
        res = host_leaf_sums(leaf, grad, hess, 9)
        check_against_exact(leaf, grad, hess, 9, res)
        empty = np.arange(9) != only
        assert np.all(res[0][empty] == 0.0) and np.all(res[1][empty] == 0.0) and np.all(res[2][empty] == 0)


def test_a_leaf_id_outside_the_tree_is_an_error():
    one = np.ones(4, dtype=np.float32)
    for bad in (3, -1):
        with pytest.raises(lgb.basic.LightGBMError):
            host_leaf_sums(np.array([0, 1, bad, 2], dtype=np.int32), one, one, 3)


# ---------------------------------------------------------------- the shared leaf-output formula
REFIT_CASES = {
    "regression": dict(objective="regression", lambda_l2=1.5, max_delta_step=0.3, path_smooth=2.0, lambda_l1=0.1),
    "binary": dict(objective="binary"),
}


def refit_data(seed, n=400, f=6):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, f)
    y = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.1 * rs.randn(n)
    return X, y


def cpu_refit_text(name):
    """the CPU learner's refit of the stored base model on fixed data, as model text"""
    params = dict(REFIT_CASES[name], device_type="cpu", verbose=-1, num_threads=1)
    base = lgb.Booster(model_file=os.path.join(GOLDEN, "refit_cpu_%s_base.txt" % name), params=params)
    X, y = refit_data(11)
    if name == "binary":
        y = (y > 0).astype(np.float64)
    out = base.refit(X, y, decay_rate=0.7)
    return trees_only(out.model_to_string())


def trees_only(text):
    """the model text up to its parameter dump"""
    return text.split("\nparameters:")[0]


@pytest.mark.parametrize("name", sorted(REFIT_CASES))
def test_cpu_refit_gives_the_model_text_from_before_the_formula_was_shared(name):
    with open(os.path.join(GOLDEN, "refit_cpu_%s_refit.txt" % name)) as f:
        assert cpu_refit_text(name) == f.read()


def _tree_arrays(text, key):
    for ln in text.split("\n"):
        if ln.startswith(key + "="):
            return ln.split("=", 1)[1].split()
    raise KeyError(key)


def test_three_leaf_refit_by_hand():
    """One regression tree of three leaves: the scores of a refit start at 0, so g = float32(-y),
    h = 1, and a leaf's value is decay * old + (1 - decay) * shrinkage * out with
    out = -T(sum_g) / (kEps + count + lambda_l2) (T: lambda_l1 soft threshold), clipped to
    max_delta_step, then for leaves after the first smoothed towards the parent term (the index
    of the leaf's parent node, as the reference passes it): out * w / (w + 1) + parent / (w + 1)
    with w = count / path_smooth."""
    l1, l2, mds, ps, decay = 0.05, 2.0, 0.4, 3.0, 0.6
    rs = np.random.RandomState(5)
    X = rs.randn(300, 3)
    y = np.where(X[:, 0] > 0.3, 2.0, np.where(X[:, 1] > 0.0, -1.0, 0.5)) + 0.05 * rs.randn(300)
    params = dict(objective="regression", num_leaves=3, min_data_in_leaf=5, learning_rate=0.25, verbose=-1,
                  device_type="cpu", lambda_l1=l1, lambda_l2=l2, max_delta_step=mds, path_smooth=ps, num_threads=1)
    bst = lgb.train(params, lgb.Dataset(X, y), num_boost_round=1)
    text = bst.model_to_string()
    assert int(_tree_arrays(text, "num_leaves")[0]) == 3
    old = [float(v) for v in _tree_arrays(text, "leaf_value")]
    shrinkage = float(_tree_arrays(text, "shrinkage")[0])
    left = [int(v) for v in _tree_arrays(text, "left_child")]
    right = [int(v) for v in _tree_arrays(text, "right_child")]
    parent = {}
    for node, (a, b) in enumerate(zip(left, right)):
        for child in (a, b):
            if child < 0:
                parent[~child] = node
    X2 = rs.randn(200, 3)
    y2 = (np.where(X2[:, 0] > 0.3, 1.5, -0.5) + 0.05 * rs.randn(200)).astype(np.float32).astype(np.float64)
    leaves = bst.predict(X2, pred_leaf=True).reshape(-1)
    refit = bst.refit(X2, y2, decay_rate=decay)
    got = [float(v) for v in _tree_arrays(refit.model_to_string(), "leaf_value")]
    g = (0.0 - y2).astype(np.float32)
    for leaf in range(3):
        rows = np.nonzero(leaves == leaf)[0]
        sg, sh = 0.0, K_EPSILON
        for i in rows:  # (the learner's order: ascending rows, double accumulators)
            sg += float(g[i])
            sh += 1.0
        thr = max(0.0, abs(sg) - l1) * ((sg > 0) - (sg < 0))
        out = -thr / (sh + l2)
        if abs(out) > mds:
            out = mds if out > 0 else -mds
        if leaf > 0:
            w = len(rows) / ps
            out = out * w / (w + 1) + parent[leaf] / (w + 1)
        want = decay * old[leaf] + (1.0 - decay) * (out * shrinkage)
        # the same double operations in the same order: equal up to the model text's 17 digits
        assert got[leaf] == pytest.approx(want, rel=1e-15, abs=0.0), (leaf, got[leaf], want)
