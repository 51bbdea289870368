"""The rule of the binning of a GPU tensor (src/device/tensor_bins.h), evaluated on the host
(LGBM_AMD_TensorGroupBinsOnHost) against the group bins of the Dataset the host builds from the same
matrix (LGBM_AMD_DatasetGetGroupBins): equal in every group the rule does not hand to the host.
Two categorical columns carry 0, a negative value, NaN, 2.9, 100000 and -- in the reference= set --
a category the training matrix never shows.  Needs no GPU.
"""
import ctypes

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from lightgbmv1_amd import ops

PARAMS = {"max_bin": 63, "min_data_in_bin": 1, "min_data_in_leaf": 1, "verbose": -1, "num_threads": 2}
SETTINGS = {"default": {}, "no_missing": {"use_missing": False}, "zero_as_missing": {"zero_as_missing": True},
            "no_bundle": {"enable_bundle": False}}
CATS = [10, 11]


def matrix(n, seed, unseen=False):
    """n x 12: dense columns with NaN and exact zeros (0-3), a mutually exclusive sparse-ish pair
    that bundles (4, 5), sparse filler (6-9), two categorical columns (10, 11)"""
    rng = np.random.RandomState(seed)
    X = rng.randn(n, 12)
    X[rng.rand(n) < 0.1, 1] = np.nan
    X[rng.rand(n) < 0.3, 2] = 0.0
    side = rng.rand(n)
    X[:, 4] = np.where(side < 0.25, rng.randint(1, 9, n), 0.0)
    X[:, 5] = np.where(side > 0.75, rng.randint(1, 9, n) * 0.5, 0.0)
    X[:, 6:10] *= rng.rand(n, 4) < 0.05
    X[:, 10] = rng.choice([0.0, 1.0, 2.9, 3.0, 7.0, -1.0, np.nan, 100000.0], n)
    X[:, 11] = rng.choice(np.arange(40.0), n)
    if unseen:
        X[::7, 10] = 5.0
        X[::5, 11] = 77.5
    return X


def bins(ds, X, call):
    """[rows][groups] of LGBM_AMD_DatasetGetGroupBins / LGBM_AMD_TensorGroupBinsOnHost"""
    ng = ctypes.c_int(0)
    nat.call("LGBM_AMD_DatasetGetGroupBins", ds.handle, None, None, ctypes.byref(ng))
    out = np.full((X.shape[0], ng.value), -7, dtype=np.int32)
    p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    if call == "dataset":
        nat.call("LGBM_AMD_DatasetGetGroupBins", ds.handle, p, None, ctypes.byref(ng))
    else:
        code = {2: nat.DTYPE_FLOAT16, 4: nat.DTYPE_FLOAT32, 8: nat.DTYPE_FLOAT64}[X.itemsize]
        nat.call("LGBM_AMD_TensorGroupBinsOnHost", ds.handle, ctypes.c_void_p(X.ctypes.data), nat.c_int(code),
                 ctypes.c_int32(X.shape[0]), ctypes.c_int32(X.shape[1]), ctypes.c_int64(X.strides[0] // X.itemsize),
                 ctypes.c_int64(X.strides[1] // X.itemsize), p, ctypes.byref(ng))
    return out


@pytest.mark.parametrize("layout", ["f64", "f32_column_major", "f16_view"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_rule_equals_the_host_dataset(monkeypatch, setting, layout):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", "0")
    params = dict(PARAMS, **SETTINGS[setting])
    train, valid = matrix(600, 1), matrix(300, 2, unseen=True)
    if layout == "f32_column_major":
        train, valid = (np.asfortranarray(m.astype(np.float32)) for m in (train, valid))
    if layout == "f16_view":
        # (100000 is infinity as float16, where the host's cast to int is undefined: 60000 instead)
        train, valid = (np.pad(np.where(m == 100000.0, 60000.0, m), ((0, 0), (1, 0))).astype(np.float16)
                        .repeat(2, axis=0)[::2, 1:] for m in (train, valid))
        assert not train.flags.c_contiguous
    y = np.zeros(len(train), dtype=np.float32)
    tr = lgb.Dataset(train, y, params=params, categorical_feature=CATS, free_raw_data=False).construct()
    va = lgb.Dataset(valid, y[:len(valid)], reference=tr, free_raw_data=False).construct()
    for ds, X in ((tr, train), (va, valid)):
        host, rule = bins(ds, X, "dataset"), bins(ds, X, "rule")
        assert host.shape[1] >= 8 and (rule >= 0).all()
        assert (host.shape[1] < 12) == (setting != "no_bundle")
        bad = np.argwhere(host != rule)
        assert bad.shape[0] == 0, (bad[:8], host[host != rule][:8], rule[host != rule][:8])
    assert (bins(tr, train, "rule") > 0).any(axis=0).all()


def test_sparse_groups_and_wide_categoricals_are_handed_to_the_host(monkeypatch):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", "1")
    X = matrix(600, 3)
    y = np.zeros(len(X), dtype=np.float32)
    ds = lgb.Dataset(X, y, params=dict(PARAMS, enable_bundle=False), categorical_feature=CATS).construct()
    assert (bins(ds, X, "rule") == -1).all()
    monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", "0")
    cap = ops.tensor_bin_launch_info()["max_categories"]
    X = np.tile(X, (4, 1))
    X[:, 11] = np.arange(len(X)) % (cap + 2)
    ds = lgb.Dataset(X, np.zeros(len(X), dtype=np.float32), categorical_feature=CATS,
                     params=dict(PARAMS, enable_bundle=False, max_bin=4096)).construct()
    host, rule = bins(ds, X, "dataset"), bins(ds, X, "rule")
    handed = (rule == -1).all(axis=0)
    assert handed.sum() == 1 and host[:, handed].max() > cap
    assert np.array_equal(host[:, ~handed], rule[:, ~handed])
