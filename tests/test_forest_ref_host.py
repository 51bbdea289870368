"""The walker of tests/helpers/forest_ref.py (the decision rule of a node, written down apart from
the code) against the host predictor, and against the host evaluator of the SHAP path tables
(LGBM_AMD_BoosterPathTableContrib, which decides with dev::ForestGoesLeft, the device kernels'
rule): hand-written forests that meet every edge value of a split -- NaN at a categorical node,
values in (-1, 0), categories past the bitset, +-1e-35, a float32 just beyond a float64
threshold -- and four trained models with such values injected.  Raw scores and leaf indices
must be equal, as float32 and float64, dense and CSR, with no value left out.  No GPU: this is
what makes the host predictor a reference for tests/test_device_forest_decisions.py.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lightgbmv1_amd as lgb
from helpers import contrib_cases as cc
from helpers import forest_ref as fr

DTYPES = [np.float32, np.float64]
TRAINED = ["categorical_zero_missing", "repeat3", "multiclass3", "single_leaf"]


def cast(X, dtype):
    with np.errstate(over="ignore"):  # (1e300 is inf as float32: the walker takes what the cast gives)
        return np.ascontiguousarray(np.asarray(X).astype(dtype))


@functools.lru_cache(maxsize=None)
def booster_of(name):
    return lgb.Booster(model_str=fr.FORESTS[name].text)


@functools.lru_cache(maxsize=None)
def walked(name, dtype):
    f = fr.FORESTS[name]
    return fr.walk(f.text, cast(f.rows, dtype), f.start, f.num)


def injected(name):
    """the rows of a contrib_cases model with the awkward values of a split put in"""
    c = cc.case(name)
    X = c.X[:400].copy()
    rng = np.random.RandomState(23)
    for value in (np.nan, -0.5, 1e10, 1e-36, -1.0, 0.0):
        X[rng.rand(*X.shape) < 0.04] = value
    return c, X


@functools.lru_cache(maxsize=None)
def walked_trained(name, dtype):
    c, X = injected(name)
    return fr.walk(c.booster.model_to_string(), cast(X, dtype), c.start, c.num)


def stored_csr(X):
    """every element stored, zeros and tiny values too"""
    n, f = X.shape
    return sp.csr_matrix((X.ravel(), np.tile(np.arange(f, dtype=np.int32), n), np.arange(n + 1, dtype=np.int32) * f),
                         shape=X.shape)


def host(booster, X, start=0, num=-1, **kw):
    n = X.shape[0]
    raw = booster.predict(X, raw_score=True, start_iteration=start, num_iteration=num, **kw)
    leaf = booster.predict(X, pred_leaf=True, start_iteration=start, num_iteration=num, **kw)
    return np.asarray(raw, dtype=np.float64).reshape(n, -1), np.asarray(leaf, dtype=np.float64).reshape(n, -1)


def check_routes(booster, X, want, start, num, what):
    """dense, CSR without its zeros and CSR with every element stored"""
    raw_w, leaf_w = want
    for route, M in (("dense", X), ("csr", sp.csr_matrix(X)), ("stored csr", stored_csr(X))):
        assert M.dtype == X.dtype
        raw, leaf = host(booster, M, start, num)
        bad = np.nonzero((leaf != leaf_w).any(axis=1) | (raw != raw_w).any(axis=1))[0]
        assert raw.shape == raw_w.shape and leaf.shape == leaf_w.shape and bad.size == 0, \
            "%s %s: rows %s differ, first %s" % (what, route, bad[:8], X[bad[:1]])


def test_model_text_round_trip():
    """parse() reads back what model_text() wrote, and the project loads it as the same forest"""
    for f in fr.FORESTS.values():
        per_iteration, features, trees = fr.parse(f.text)
        assert (per_iteration, features, len(trees)) == (f.num_class, f.num_features, len(f.trees))
        bst = booster_of(f.name)
        assert bst.num_trees() == len(trees) and bst.num_feature() == features
        assert bst.num_model_per_iteration() == per_iteration
        again = fr.parse(bst.model_to_string())
        assert again == (per_iteration, features, trees)
    _, _, trees = fr.parse(fr.FORESTS["offsets"].text)
    assert [t["cat_boundaries"] for t in trees] == [[0, 1, 4, 6], [0, 3, 4], [0, 2, 3, 6]]
    _, _, trees = fr.parse(fr.FORESTS["table"].text)
    assert trees[6]["cat_threshold"] == [(1 << 0) | (1 << 5) | (1 << 31), (1 << 0) | (1 << 31)]


def test_the_rule_on_values_worked_by_hand():
    words = [(1 << 0) | (1 << 5) | (1 << 31), (1 << 0) | (1 << 31)]  # {0, 5, 31, 32, 63}
    left = [0.0, -0.0, -0.5, -0.999, 0.999, 5.0, 5.5, 31.0, 31.9, 32.0, 63.0, 63.99, fr.ZERO, 1e-40]
    for m in (0, 1, 2):
        dt = fr.CATEGORICAL | (m << 2)
        for v in fr.CATEGORICAL_EDGES:
            assert fr.goes_left(v, 0.0, dt, words) == any(v == x for x in left), (v, m)
    f32_tenth = float(np.float32(0.1))
    assert f32_tenth > 0.1 and not fr.goes_left(f32_tenth, 0.1, 0)
    assert fr.goes_left(float(np.nextafter(np.float32(0.1), np.float32(0))), 0.1, 0)
    for default_left in (False, True):
        d = fr.DEFAULT_LEFT if default_left else 0
        # missing None: NaN is 0, which is <= 0.1; the default side is never used
        assert fr.goes_left(float("nan"), 0.1, d) and fr.goes_left(0.0, 0.1, d) and not fr.goes_left(1.0, 0.1, d)
        # missing Zero: 0, +-1e-35 and NaN (read as 0) take the default side, the next double does not
        for v in (0.0, -0.0, fr.ZERO, -fr.ZERO, 5e-324, float("nan")):
            assert fr.goes_left(v, 0.1, d | 4) == default_left
        assert fr.goes_left(float(np.nextafter(fr.ZERO, 1.0)), 0.1, d | 4)
        # missing NaN: only NaN takes the default side
        assert fr.goes_left(float("nan"), 0.1, d | 8) == default_left
        assert fr.goes_left(0.0, 0.1, d | 8) and not fr.goes_left(float("inf"), 0.1, d | 8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(fr.FORESTS))
def test_hand_written_forests_match_the_host(name, dtype):
    f = fr.FORESTS[name]
    check_routes(booster_of(name), cast(f.rows, dtype), walked(name, dtype), f.start, f.num,
                 "%s %s" % (name, np.dtype(dtype).name))


def test_table_rows_reach_both_sides_of_every_stump():
    """(the table would prove nothing if a stump sent every edge value one way)"""
    for dtype in DTYPES:
        leaf = walked("table", dtype)[1]
        assert all(set(leaf[:, t]) == {0.0, 1.0} for t in range(9))
    leaf = walked("offsets", np.float64)[1]
    assert [len(set(leaf[:, t])) for t in range(3)] == [5, 5, 5]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", TRAINED)
def test_trained_models_match_the_host(name, dtype):
    c, X = injected(name)
    check_routes(c.booster, cast(X, dtype), walked_trained(name, dtype), c.start, c.num,
                 "%s %s" % (name, np.dtype(dtype).name))


def _check_additive(booster, X, raw, num_class, start, num, what):
    """the rows of the path-table contributions sum to the walker's raw score"""
    f1 = X.shape[1] + 1
    got = cc.path_table_contrib(booster, X.astype(np.float64), start, num)
    bound = f1 * cc.tolerance(booster, start, num)
    defect = float(np.max(np.abs(got.reshape(len(X), num_class, f1).sum(axis=2) - raw)))
    print("%s: additivity defect %.3e (bound %.3e)" % (what, defect, bound))
    assert defect <= bound, what
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_table_evaluator_sums_to_the_walker(dtype):
    for name in fr.DEVICE_FORESTS:
        f = fr.FORESTS[name]
        _check_additive(booster_of(name), cast(f.rows, dtype), walked(name, dtype)[0], f.num_class, f.start, f.num, name)
    for name in TRAINED:
        c, X = injected(name)
        _check_additive(c.booster, cast(X, dtype), walked_trained(name, dtype)[0], c.num_class, c.start, c.num, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_table_contribution_of_a_stump_is_its_leaf_minus_its_mean(dtype):
    f = fr.FORESTS["table"]
    X = cast(f.rows, dtype)
    got = cc.path_table_contrib(booster_of("table"), X.astype(np.float64))
    leaf = walked("table", dtype)[1].astype(int)
    tol = cc.tolerance(booster_of("table"))
    bias = 0.0
    for t, tr in enumerate(f.trees):
        (v0, v1), (c0, c1) = tr["leaf_values"], tr["leaf_counts"]
        total = float(c0 + c1)
        expected = 0.0  # (the sum as the table builder rounds it: Tree::ExpectedValue)
        expected += (c0 / total) * v0
        expected += (c1 / total) * v1
        bias += expected
        want = np.where(leaf[:, t] == 0, v0, v1) - expected
        assert np.max(np.abs(got[:, t] - want)) <= tol, "stump %d" % t
    assert np.max(np.abs(got[:, 9] - bias)) <= tol


@pytest.mark.parametrize("name", ["table", "offsets", "classes16"])
def test_narrower_and_wider_matrices_read_absent_columns_as_zero(name):
    f = fr.FORESTS[name]
    bst = booster_of(name)
    wide = np.concatenate([f.rows, np.full((len(f.rows), 3), 7.0)], axis=1)
    for cols in (1, 2, f.num_features + 3):
        X = np.ascontiguousarray(wide[:, :cols])
        with pytest.raises(lgb.LightGBMError):
            bst.predict(X, raw_score=True)
        raw_w, leaf_w = fr.walk(f.text, X, f.start, f.num)
        raw, leaf = host(bst, X, f.start, f.num, predict_disable_shape_check=True)
        assert np.array_equal(raw, raw_w) and np.array_equal(leaf, leaf_w), cols
