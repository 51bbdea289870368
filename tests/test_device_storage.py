"""The learner's binned rows built on the device (src/device/storage_kernels.hip,
LGBM_AMD_DEVICE_STORAGE=1) against the host branch (=0), byte for byte, and against an independent
reading: every group's field cut out of the row image where the layout record says it is equals
that group's column of LGBM_AMD_DatasetGetGroupBins, every other byte is zero, the column image
holds the same columns and the row-sparse lists the rows' non-zero cells in ascending order."""
import ctypes

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from lightgbmv1_amd import ops
from lightgbmv1_amd._native import call

pytestmark = pytest.mark.gpu

INFO = ops.storage_launch_info()
T, S = INFO["tile_rows"], INFO["scan_rows"]
M = 2 * S + 1  # rows of the data: two scan blocks plus 1
MAX_BIN = {"n": 63, "w": 1000, "b": 15}  # narrow, wide (more than 256 bins) and 4-bit features

# name -> (feature kinds, training rows, environment, what else the case does)
CASES = {
    "rows 1": ("nnnnn", 1, {}, ""), "rows tile-1": ("nnnnn", T - 1, {}, ""), "rows tile": ("nnnnn", T, {}, ""),
    "rows tile+1": ("nnnnn", T + 1, {}, ""), "rows two scan blocks+1": ("nnnnn", M, {"LGBM_AMD_SPARSE_ROWS": "1"}, ""),
    "1 group": ("n", T + 1, {}, ""), "3 groups": ("nnn", T + 1, {}, ""), "4 groups": ("nnnn", T + 1, {}, ""),
    "4-bit, 8 groups": ("b" * 8, T + 1, {"LGBM_AMD_NIBBLE_BINS": "1"}, ""),
    "4-bit, 9 groups": ("b" * 9, T + 1, {"LGBM_AMD_NIBBLE_BINS": "1"}, ""),
    "mixed": ("nwn", T + 1, {}, ""), "all wide": ("www", T + 1, {}, ""),
    "mixed, row-sparse": ("nwn", T + 2, {"LGBM_AMD_SPARSE_ROWS": "1"}, ""),
    "host-sparse": ("nnwn", T + 1, {"LGBM_AMD_HOST_SPARSE": "1"}, "empty"),
    "row-sparse": ("nnnnn", T + 1, {"LGBM_AMD_SPARSE_ROWS": "1"}, ""),
    "row-sparse of host-sparse": ("nnnnn", T + 1, {"LGBM_AMD_SPARSE_ROWS": "1", "LGBM_AMD_HOST_SPARSE": "1"}, ""),
    "row align": ("nnnnn", T + 1, {"LGBM_AMD_ROW_ALIGN_WORDS": "8"}, ""),
    "gh in rows": ("nnnnn", T + 1, {"LGBM_AMD_GH_IN_ROWS": "1"}, ""),
    "wide row, two slices": ("n" * (4 * INFO["slice_words"] + 1), T + 1, {}, ""),
    "validation set": ("nnwnn", T + 1, {}, "valid"),
    "three windows": ("nnnnn", M, {"LGBM_AMD_COLUMN_COPY": "0"}, "windows"),
}


def _data(kinds, empty):
    rng = np.random.RandomState(len(kinds))
    cols = [rng.randint(0, 600, M) if k == "w" else rng.randint(1, 41 if k == "n" else 10, M) * (rng.rand(M) < 0.4)
            for k in kinds]
    X = np.stack(cols, axis=1).astype(np.float64)
    X[0], X[1] = 0, 3  # a row with no stored bin, a row with every group stored
    if empty:
        X[:T + 1, 0] = 0  # host-sparse: an empty stored list
        X[T, -1] = 5      # ... and a stored last row
    return X, rng.rand(M)


def _boosters(kinds, n, env, monkeypatch, empty=False):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params = {"objective": "regression", "device_type": "gpu", "verbose": -1, "enable_bundle": False, "min_data_in_bin": 1,
              "max_bin_by_feature": [MAX_BIN[k] for k in kinds], "min_data_in_leaf": 1}
    X, y = _data(kinds, empty)
    ref = lgb.Dataset(X, y, params=params).construct()
    train = lgb.Dataset(X[:n], y[:n], reference=ref, params=params).construct()
    out = []
    for branch in "01":
        monkeypatch.setenv("LGBM_AMD_DEVICE_STORAGE", branch)
        out.append(lgb.Booster(params=params, train_set=train))
    return X, train, out


def _group_bins(ds):
    ng = ctypes.c_int(0)
    call("LGBM_AMD_DatasetGetGroupBins", ds.handle, None, None, ctypes.byref(ng))
    bins = np.zeros((ds.num_data(), ng.value), np.int32)
    bound = np.zeros(ng.value + 1, np.int64)
    call("LGBM_AMD_DatasetGetGroupBins", ds.handle, bins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
         bound.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(ng))
    return bins, bound


def _check_reading(booster, ds, data_idx):
    gb, bound = _group_bins(ds)
    lay = ops.device_storage(booster, "layout", data_idx)
    n = gb.shape[0]
    assert lay["rows"] == n and len(lay["byte"]) == gb.shape[1]
    rows = ops.device_storage(booster, "rows", data_idx)
    if not lay["sparse_rows"]:
        image = rows.view(np.uint8).reshape(n, 4 * lay["row_words"]).astype(np.int64)
        used = np.zeros(4 * lay["row_words"], np.int64)
        for g, (b, w, nib) in enumerate(zip(lay["byte"], lay["width"], lay["nibble"])):
            field = (image[:, b] >> (4 * nib)) & 15 if w == 4 else image[:, b] + (image[:, b + 1] << 8 if w == 16 else 0)
            assert np.array_equal(field, gb[:, g]), "group %d" % g
            used[b] |= (15 << (4 * nib)) if w == 4 else 255
            if w == 16:
                used[b + 1] |= 255
        assert not np.any(image & ~used), "bytes outside the declared fields"
    else:
        assert rows.size == 0
        stored = gb != 0
        assert np.array_equal(ops.device_storage(booster, "sp_ptr"), np.concatenate([[0], np.cumsum(stored.sum(1))]))
        assert np.array_equal(ops.device_storage(booster, "sp_bin"), (gb + bound[:-1])[stored])
        if np.all(bound[1:] - bound[:-1] <= 64) and n > 1:  # (narrow features: zero is their bin 0)
            assert stored[0].sum() == 0 and stored[1].all()
    cols = ops.device_storage(booster, "columns", data_idx)
    if cols.size:
        assert cols.size == n * int((lay["width"] == 16).sum() + len(lay["width"]))
        for g, (c, w) in enumerate(zip(lay["column"], lay["width"])):
            col = np.frombuffer(cols[c:c + 2 * n].tobytes(), "<u2") if w == 16 else cols[c:c + n]
            assert np.array_equal(col, gb[:, g]), "column %d" % g


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_built_storage_equals_host_and_group_bins(name, monkeypatch):
    kinds, n, env, what = CASES[name]
    if what == "windows":  # a budget that leaves a window 800 of the 5-byte column rows beside the 8-byte rows
        budget = 4 * (4096 + 5 * 800) + n * 8
        plan = (ctypes.c_int64 * 6)()
        call("LGBM_AMD_StoragePlan", ctypes.c_int64(n), ctypes.c_int64(5), ctypes.c_int64(8), ctypes.c_int64(budget),
             ctypes.c_int(0), plan)
        assert plan[5] == 3
        monkeypatch.setenv("LGBM_AMD_STORAGE_BUDGET", str(budget))
    X, train, (host, dev) = _boosters(kinds, n, env, monkeypatch, what == "empty")
    sets = [(0, train)]
    if what == "valid":
        valid = lgb.Dataset(X[S:S + T + 1], np.zeros(T + 1), reference=train).construct()
        for b, branch in ((host, "0"), (dev, "1")):
            monkeypatch.setenv("LGBM_AMD_DEVICE_STORAGE", branch)
            b.add_valid(valid, "valid")
        sets.append((1, valid))
    for data_idx, ds in sets:
        for which in ("rows", "columns", "sp_ptr", "sp_bin"):
            a, b = ops.device_storage(host, which, data_idx), ops.device_storage(dev, which, data_idx)
            assert a.shape == b.shape and np.array_equal(a, b), which
        _check_reading(dev, ds, data_idx)
    if "SPARSE_ROWS" in "".join(env):
        assert ops.device_storage(dev, "layout")["sparse_rows"]


def test_training_on_device_built_storage_gives_the_same_model(monkeypatch):
    before = (ctypes.c_int64(0), ctypes.c_int64(0))
    call("LGBM_AMD_DeviceStorageStats", ctypes.byref(before[0]), ctypes.byref(before[1]))
    _, _, boosters = _boosters("nnwnn", M, {}, monkeypatch)
    texts = []
    for b in boosters:
        for _ in range(5):
            b.update()
        texts.append(b.model_to_string())
    assert texts[0] == texts[1] and boosters[0].num_trees() == 5
    after = (ctypes.c_int64(0), ctypes.c_int64(0))
    call("LGBM_AMD_DeviceStorageStats", ctypes.byref(after[0]), ctypes.byref(after[1]))
    assert after[0].value == before[0].value + 1 and after[1].value == before[1].value + 1
