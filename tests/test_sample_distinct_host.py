"""The first step of the bin finder as the device computes it (src/device/sample_distinct.h),
evaluated on the host (LGBM_AMD_SampleDistinct) against a NumPy reference, bit for bit; and the
bin finder split at that seam (LGBM_AMD_DEVICE_BIN_FIND=2: the evaluator's lists into
BinMapper::FindBinFromDistinct) against BinMapper::FindBin on the same NumPy matrix: the same
binary file.  Needs no GPU.
"""
import ctypes

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat

ZERO = float(np.float32(1e-35))  # kZeroThreshold: a float constant


def reference(col):
    """(distinct, counts, na_cnt) of one column"""
    x = np.asarray(col, dtype=np.float64)
    na = int(np.isnan(x).sum())
    x = x[~np.isnan(x)]
    x = np.sort(x[np.abs(x) > ZERO])
    if x.size == 0:
        return x, np.zeros(0, dtype=np.int32), na
    with np.errstate(over="ignore"):  # (DBL_MAX's neighbour is inf)
        start = np.r_[True, x[1:] > np.nextafter(x[:-1], np.inf)]
    counts = np.diff(np.r_[np.flatnonzero(start), x.size]).astype(np.int32)
    return x[np.r_[start[1:], True]], counts, na


def assert_same(got, want, what):
    assert len(got) == len(want)
    for c, (g, r) in enumerate(zip(got, want)):
        assert g[2] == r[2], (what, c, "NaN count", g[2], r[2])
        assert np.array_equal(g[0].view(np.int64), r[0].view(np.int64)), (what, c, g[0][:8], r[0][:8])
        assert np.array_equal(g[1], r[1]) and g[1].dtype == np.int32, (what, c, g[1][:8], r[1][:8])


def f64(*bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def edge_columns():
    """name -> values; edge_matrix pads them with zeros, which every column drops"""
    t = np.float32(1e-35)
    around = [t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))]
    bf = (int(np.array([t]).view(np.uint32)[0]) >> 16) + np.arange(-1, 3)  # bfloat16 values on both sides of it
    around += list((bf << 16).astype(np.uint32).view(np.float32))
    one = 0x3FF0000000000000
    return {
        "all_zero": [0.0] * 5,
        "all_nan": [np.nan] * 7,
        "one_value": [3.5] * 40,
        "top_byte": list(f64(one, 0x40F0000000000000)) * 3,
        "low_byte": list(f64(one, one + 5)) * 3,
        "every_byte": list(f64(*[one ^ (5 << (8 * p)) for p in range(8)], one)) * 2,
        "signs_and_zeros": [-2.5, 0.0, 3.0, -1.0, 0.0, 7.0, -2.5, 0.0, 1e-3, -1e-3],
        "negative_zero": [-0.0, 1.0, -0.0, -1.0],
        "infinities": [np.inf, np.finfo(np.float64).max, -np.inf, -np.finfo(np.float64).max, 1.0, np.inf],
        "zero_threshold": [float(s * v) for v in around for s in (1, -1)],
        "subnormals": [5e-324, -5e-324, 1e-310, float(np.float32(1e-40)), 2.0],
        "ulp_chain": list(f64(0x3FF8000000000000, 0x3FF8000000000001, 0x3FF8000000000002, 0x3FF8000000000004)),
        "nans": list(f64(0x7FF8000000000001, 0xFFF8000000000000)) + [1.0, 2.0] + list(f64(0x7FF0000000000001,
                                                                                           0xFFFFFFFFFFFFFFFF)) + [1.0],
        "categories": [3, 1, 3, 7, 1, 0, 3, 100000, 7, 7],
    }


def edge_matrix():
    """[rows][columns] float64, the columns of edge_columns() in a fixed shuffle"""
    cols = edge_columns()
    n = max(len(v) for v in cols.values()) + 3
    rng = np.random.RandomState(5)
    X = np.zeros((n, len(cols)))
    for c, v in enumerate(cols.values()):
        X[:len(v), c] = v
        X[:, c] = X[rng.permutation(n), c]
    return X


def evaluate(X):
    """LGBM_AMD_SampleDistinct on the columns of X"""
    sample = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
    ncol, ns = sample.shape
    distinct, counts = np.empty(ns * ncol + 1), np.empty(ns * ncol + 1, dtype=np.int32)
    begin, na = np.zeros(ncol + 1, dtype=np.int64), np.zeros(ncol, dtype=np.int32)
    nat.call("LGBM_AMD_SampleDistinct", sample.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int64(ns),
             ctypes.c_int32(ncol), distinct.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
             counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
             na.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return [(distinct[begin[c]:begin[c + 1]], counts[begin[c]:begin[c + 1]], int(na[c])) for c in range(ncol)]


def test_edge_columns():
    X = edge_matrix()
    want = [reference(X[:, c]) for c in range(X.shape[1])]
    by_name = dict(zip(edge_columns(), want))
    assert by_name["all_zero"][0].size == 0 and by_name["all_nan"][2] == 7 and by_name["subnormals"][0].tolist() == [2.0]
    assert by_name["ulp_chain"][1].tolist() == [3, 1] and by_name["infinities"][1].tolist() == [2, 1, 3]
    assert_same(evaluate(X), want, "edge")


def test_random_columns():
    rng = np.random.RandomState(3)
    X = np.stack([rng.randn(500), rng.randn(500).astype(np.float32), rng.randint(-3, 4, 500) * 0.5,
                  np.where(rng.rand(500) < 0.2, np.nan, rng.randn(500).round(1))], axis=1)
    assert_same(evaluate(X), [reference(X[:, c]) for c in range(4)], "random")


@pytest.mark.parametrize("setting", [{}, {"use_missing": False}, {"zero_as_missing": True},
                                     {"max_bin_by_feature": True, "min_data_in_bin": 3}])
def test_split_bin_finder_builds_the_same_dataset(monkeypatch, tmp_path, setting):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    rng = np.random.RandomState(11)
    E = edge_matrix()
    names = list(edge_columns())
    X = np.hstack([E[rng.randint(0, len(E), 400)], rng.randn(400, 3).round(2), rng.randint(0, 30, (400, 1)) * 1.0])
    params = {"max_bin": 63, "min_data_in_bin": 1, "min_data_in_leaf": 1, "verbose": -1, "num_threads": 2}
    params.update(setting)
    if setting.get("max_bin_by_feature"):
        params["max_bin_by_feature"] = [5 + 3 * c for c in range(X.shape[1])]
    files = []
    for knob in ("0", "2"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BIN_FIND", knob)
        ds = lgb.Dataset(X, np.zeros(len(X), dtype=np.float32), params=params,
                         categorical_feature=[names.index("categories"), X.shape[1] - 1])
        ds.construct().save_binary(str(tmp_path / (knob + ".bin")))
        files.append((tmp_path / (knob + ".bin")).read_bytes())
    assert len(files[0]) > 1000 and files[0] == files[1]
