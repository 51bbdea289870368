"""SHAP contributions and leaf indices on the device (src/device/shap_kernels.hip) against the
host predictor (LGBM_AMD_HOST_PREDICT=1): through Booster.predict / LGBM_BoosterPredictForMat
(row gate, column-major input, row chunks) and through lightgbmv1_amd.ops.forest_predict on GPU
tensors.  Leaf indices and raw scores must be equal; contributions are held to the tolerance of
tests/helpers/contrib_cases.py (64 * 2**-52 * S) and must sum to the device raw score.
LGBM_AMD_DevicePredictCount tells which path a call took, so a silent host fallback fails.

Long paths: TreeSHAP itself loses accuracy on a deep path whose one-fractions are mostly 1 (at
100 distinct features the host recursion's contributions no longer sum to the raw score: the
unwound sums cancel), so where the host is to be matched the chain-tree rows take at most six
right turns: there the host's own additivity defect is within the bound and it is a reference.
"""
import ctypes

import numpy as np
import pytest
import torch  # (before the native library loads, as in tests/test_ops.py: one HIP runtime for both)

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from lightgbmv1_amd import ops
from helpers import contrib_cases as cc

pytestmark = pytest.mark.gpu

GPU = {"device_type": "gpu"}
MAX_DISTINCT = 119  # dev::kShapMaxPathLen - 1: features on one path besides the bias element


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    pass


def _device_calls():
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DevicePredictCount", ctypes.byref(out))
    return out.value


def _host(monkeypatch, booster, X, **kw):
    monkeypatch.setenv("LGBM_AMD_HOST_PREDICT", "1")
    before = _device_calls()
    out = booster.predict(X, **kw, **GPU)
    assert _device_calls() == before
    monkeypatch.delenv("LGBM_AMD_HOST_PREDICT")
    return out


def _device(booster, X, calls=1, **kw):
    before = _device_calls()
    out = booster.predict(X, **kw, **GPU)
    assert _device_calls() == before + calls, "the prediction did not run on the device"
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", cc.CASES)
def test_model_cases_match_the_host(name, dtype, monkeypatch):
    c = cc.case(name)
    X = np.ascontiguousarray(c.X.astype(dtype))
    leaf_h = _host(monkeypatch, c.booster, X, pred_leaf=True, **c.window)
    contrib_h = _host(monkeypatch, c.booster, X, pred_contrib=True, **c.window)
    leaf_d = _device(c.booster, X, pred_leaf=True, **c.window)
    contrib_d = _device(c.booster, X, pred_contrib=True, **c.window)
    raw_d = _device(c.booster, X, raw_score=True, **c.window)
    assert leaf_d.shape == leaf_h.shape and np.array_equal(leaf_d, leaf_h)
    cc.check_contrib(contrib_d.reshape(len(X), -1), contrib_h.reshape(len(X), -1), raw_d, c,
                     "%s %s" % (name, np.dtype(dtype).name))


def test_column_major_input(monkeypatch):
    c = cc.case("repeat3")
    X = np.asfortranarray(c.X)
    width = c.num_class * (c.num_features + 1)
    out = np.empty((len(X), width))
    got = ctypes.c_int64(0)
    before = _device_calls()
    nat.call("LGBM_BoosterPredictForMat", c.booster.handle, X.ctypes.data_as(ctypes.c_void_p), nat.c_int(1),
             ctypes.c_int32(X.shape[0]), ctypes.c_int32(X.shape[1]), nat.c_int(0), nat.c_int(nat.PREDICT_CONTRIB),
             nat.c_int(0), nat.c_int(-1), nat.cstr("device_type=gpu"), ctypes.byref(got),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert got.value == out.size and _device_calls() == before + 1
    want = _host(monkeypatch, c.booster, c.X, pred_contrib=True)
    cc.check_contrib(out, want, _device(c.booster, c.X, raw_score=True), c, "column-major")


def test_row_gate(monkeypatch):
    c = cc.case("window")
    for kw in ({"pred_contrib": True}, {"pred_leaf": True}):
        before = _device_calls()
        below = c.booster.predict(c.X[:1023], **kw, **GPU)
        assert _device_calls() == before, "1023 rows stay on the host"
        at = _device(c.booster, c.X[:1024], **kw)
        want = _host(monkeypatch, c.booster, c.X[:1024], **kw)
        if "pred_leaf" in kw:
            assert np.array_equal(at, want) and np.array_equal(below, want[:1023])
        else:
            whole = cc.Case(c.booster, c.X)
            assert np.array_equal(below, want[:1023])
            cc.check_contrib(at, want, _device(c.booster, c.X[:1024], raw_score=True), whole, "1024 rows")


def test_chunked_rows_are_bit_equal(monkeypatch):
    c = cc.case("multiclass3")
    X = np.concatenate([c.X, c.X[::-1]])  # 3000 rows: two chunks of 1024 and one of 952
    for kw in ({"pred_contrib": True}, {"pred_leaf": True}, {"raw_score": True}):
        whole = _device(c.booster, X, **kw)
        monkeypatch.setenv("LGBM_AMD_PREDICT_CHUNK_ROWS", "1024")
        chunked = _device(c.booster, X, **kw)
        monkeypatch.delenv("LGBM_AMD_PREDICT_CHUNK_ROWS")
        assert np.array_equal(whole, chunked)
    Xf = np.asfortranarray(X)  # (column-major chunks are strided copies)
    out = np.empty((len(X), c.num_class * (c.num_features + 1)))
    got = ctypes.c_int64(0)
    monkeypatch.setenv("LGBM_AMD_PREDICT_CHUNK_ROWS", "1024")
    nat.call("LGBM_BoosterPredictForMat", c.booster.handle, Xf.ctypes.data_as(ctypes.c_void_p), nat.c_int(1),
             ctypes.c_int32(X.shape[0]), ctypes.c_int32(X.shape[1]), nat.c_int(0), nat.c_int(nat.PREDICT_CONTRIB),
             nat.c_int(0), nat.c_int(-1), nat.cstr("device_type=gpu"), ctypes.byref(got),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert np.array_equal(out, _device(c.booster, X, pred_contrib=True).reshape(out.shape))


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_ops_forest_predict(rows, monkeypatch):
    c = cc.case("multiclass3")
    X = c.X[:rows]
    host = {k: _host(monkeypatch, c.booster, X, **{f: True}).reshape(rows, -1)
            for k, f in (("raw", "raw_score"), ("leaf", "pred_leaf"), ("contrib", "pred_contrib"))}
    for dtype in (torch.float32, torch.float64):
        Xd = torch.tensor(X, dtype=dtype, device="cuda")
        Xh = Xd.cpu().numpy().astype(np.float64)
        if dtype == torch.float32:
            host32 = {k: _host(monkeypatch, c.booster, Xh, **{f: True}).reshape(rows, -1)
                      for k, f in (("raw", "raw_score"), ("leaf", "pred_leaf"), ("contrib", "pred_contrib"))}
        want = host32 if dtype == torch.float32 else host
        got = {k: ops.forest_predict(c.booster, Xd, kind=k) for k in ("raw", "leaf", "contrib")}
        for k, t in got.items():
            assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == want[k].shape
        assert np.array_equal(got["raw"].cpu().numpy(), want["raw"])
        assert np.array_equal(got["leaf"].cpu().numpy(), want["leaf"])
        cc.check_contrib(got["contrib"].cpu().numpy(), want["contrib"], got["raw"].cpu().numpy(), c,
                         "ops %d rows %s" % (rows, dtype))
    win = ops.forest_predict(c.booster, Xd, kind="leaf", start_iteration=2, num_iteration=3)
    assert tuple(win.shape) == (rows, 9)
    with pytest.raises(lgb.LightGBMError):
        ops.forest_predict(c.booster, Xd[:, :4].contiguous(), kind="contrib")
    with pytest.raises(lgb.LightGBMError):
        ops.forest_predict(c.booster, Xd, kind="normal")


def test_wide_features_leave_unused_columns_zero(monkeypatch):
    rng = np.random.RandomState(5)
    X = rng.randn(1500, 300)
    y = X[:, ::30].sum(axis=1) + 0.1 * rng.randn(1500)
    p = {"objective": "regression", "num_leaves": 15, "min_data_in_leaf": 5, "verbose": -1, "num_threads": 4,
         "feature_fraction": 1.0}
    Xt = np.zeros_like(X[:800])
    Xt[:, ::30] = X[:800, ::30]  # only 10 columns carry signal (the rest are constant: never split on)
    bst = lgb.train(p, lgb.Dataset(Xt, y[:800], params=p), num_boost_round=10)
    c = cc.Case(bst, X)
    used = set(np.nonzero(bst.feature_importance())[0])
    assert 0 < len(used) <= 10
    got = _device(bst, X, pred_contrib=True)
    want = _host(monkeypatch, bst, X, pred_contrib=True)
    cc.check_contrib(got, want, _device(bst, X, raw_score=True), c, "300 features")
    unused = [f for f in range(300) if f not in used]
    assert np.all(got[:, unused] == 0.0)


def test_longest_path_runs_on_the_device(monkeypatch):
    bst = lgb.Booster(model_str=cc.chain_model_text(MAX_DISTINCT))
    X = cc.chain_rows(MAX_DISTINCT)
    c = cc.Case(bst, X)
    want = _host(monkeypatch, bst, X, pred_contrib=True)
    raw = _host(monkeypatch, bst, X, raw_score=True)
    # (the host is a reference on these rows: its own contributions sum to its raw score)
    assert np.max(np.abs(want.sum(axis=1) - raw)) <= (MAX_DISTINCT + 1) * cc.tolerance(bst)
    got = _device(bst, X, pred_contrib=True)
    cc.check_contrib(got, want, _device(bst, X, raw_score=True), c, "chain of %d" % MAX_DISTINCT)
    assert np.array_equal(_device(bst, X, pred_leaf=True), _host(monkeypatch, bst, X, pred_leaf=True))


def test_path_past_the_limit_falls_back_to_the_host(monkeypatch):
    k = MAX_DISTINCT + 1
    bst = lgb.Booster(model_str=cc.chain_model_text(k))
    X = cc.chain_rows(k)
    before = _device_calls()
    got = bst.predict(X, pred_contrib=True, **GPU)
    assert _device_calls() == before, "a path of %d features does not fit the kernel" % k
    assert np.array_equal(got, _host(monkeypatch, bst, X, pred_contrib=True))
    # leaf indices and scores have no such limit
    assert np.array_equal(_device(bst, X, pred_leaf=True), _host(monkeypatch, bst, X, pred_leaf=True))
    with pytest.raises(lgb.LightGBMError):
        ops.forest_predict(bst, torch.tensor(X, device="cuda"), kind="contrib")


def test_two_device_calls_are_bitwise_equal():
    c = cc.case("repeat3")
    a = _device(c.booster, c.X, pred_contrib=True)
    b = _device(c.booster, c.X, pred_contrib=True)
    assert np.array_equal(a, b, equal_nan=True)
    Xd = torch.tensor(c.X, device="cuda")
    t1 = ops.forest_predict(c.booster, Xd, kind="contrib")
    t2 = ops.forest_predict(c.booster, Xd, kind="contrib")
    assert torch.equal(t1, t2)
    assert np.array_equal(t1.cpu().numpy(), a.reshape(len(c.X), -1))


def test_booster_trained_on_the_device(monkeypatch):
    """device_type=gpu on the booster itself (no predict parameter) routes contributions and leaf
    indices to the device; train() returns such a booster with keep_training_booster=True"""
    rng = np.random.RandomState(4)
    X = rng.randn(1500, 8).astype(np.float32)
    y = (X[:, 0] * X[:, 1] + X[:, 2] > 0).astype(np.float32)
    p = {"objective": "binary", "device_type": "gpu", "num_leaves": 31, "max_bin": 63, "verbose": -1}
    bst = lgb.train(p, lgb.Dataset(X, y, params=p), num_boost_round=6, keep_training_booster=True)
    before = _device_calls()
    got = bst.predict(X, pred_contrib=True)
    leaf = bst.predict(X, pred_leaf=True)
    raw = bst.predict(X, raw_score=True)
    assert _device_calls() == before + 3
    monkeypatch.setenv("LGBM_AMD_HOST_PREDICT", "1")
    want, want_leaf = bst.predict(X, pred_contrib=True), bst.predict(X, pred_leaf=True)
    assert _device_calls() == before + 3
    assert np.array_equal(leaf, want_leaf)
    cc.check_contrib(got, want, raw, cc.Case(bst, X), "trained on the device")


def test_nan_in_a_categorical_column_goes_where_the_host_sends_it(monkeypatch):
    """the host predictor sends a NaN right at every categorical split (its int cast is negative),
    whatever the split's missing type; raw scores, leaf indices and contributions follow it"""
    c = cc.case("categorical_zero_missing")
    X = c.X.copy()
    X[::3, 1] = np.nan
    X[1::4, 3] = np.nan
    assert np.array_equal(_device(c.booster, X, pred_leaf=True), _host(monkeypatch, c.booster, X, pred_leaf=True))
    raw_d = _device(c.booster, X, raw_score=True)
    assert np.array_equal(raw_d, _host(monkeypatch, c.booster, X, raw_score=True))
    cc.check_contrib(_device(c.booster, X, pred_contrib=True), _host(monkeypatch, c.booster, X, pred_contrib=True),
                     raw_d, c, "NaN categories")
