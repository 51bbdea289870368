"""The rule of Booster.predict_device (src/device/tensor_predict.h) without a GPU: the plan
(LGBM_AMD_TensorPredictPlan) against a literal table, and the tile and packed-node walk evaluated
on host matrices (LGBM_AMD_TensorPredictOnHost) against the walker of tests/helpers/forest_ref.py.

The table.  A tile of S slots has 256 rows and takes S * pitch * elem bytes, pitch = 258 elements
for 2-byte and 257 for 4- and 8-byte elements; the plan takes the tile route while that is within
53248 bytes (52 KiB: the thresholds that profiles/r21_tensor_predict.md measured), the slots route
beyond: 516, 1028 and 2056 bytes per slot, so 103, 51 and 25 slots are the last that fit.
"""
import ctypes

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from lightgbmv1_amd import ops
from helpers import forest_ref as fr

TILE, SLOTS = 0, 1
RAW, LEAF, CONTRIB = nat.PREDICT_RAW_SCORE, nat.PREDICT_LEAF_INDEX, nat.PREDICT_CONTRIB

# (slots, element bytes, most leaves, predict type) -> (route, rows)
PLAN = [
    ((103, 2, 63, RAW), (TILE, 256)), ((104, 2, 63, RAW), (SLOTS, 256)),
    ((51, 4, 63, RAW), (TILE, 256)), ((52, 4, 63, RAW), (SLOTS, 256)),
    ((25, 8, 63, RAW), (TILE, 256)), ((26, 8, 63, RAW), (SLOTS, 256)),
    ((0, 4, 1, nat.PREDICT_NORMAL), (TILE, 256)), ((10, 4, 63, LEAF), (TILE, 256)),
    ((10, 4, 32768, RAW), (TILE, 256)), ((10, 4, 32769, RAW), (SLOTS, 256)), ((10, 4, 32769, LEAF), (SLOTS, 256)),
    ((0, 8, 1, CONTRIB), (SLOTS, 256)), ((1, 2, 2, CONTRIB), (SLOTS, 256)), ((51, 4, 63, CONTRIB), (SLOTS, 256)),
]


@pytest.mark.parametrize("args,want", PLAN)
def test_plan_table(args, want):
    out = (ctypes.c_int32 * 2)()
    nat.call("LGBM_AMD_TensorPredictPlan", ctypes.c_int32(args[0]), ctypes.c_int32(args[1]), ctypes.c_int32(args[2]),
             nat.c_int(args[3]), out)
    assert (out[0], out[1]) == want


def test_launch_info_is_the_tables():
    assert ops.tensor_predict_launch_info() == {"ladder": [256], "lds_bytes": 53248, "max_leaves": 32768}


def elements(X, dtype):
    """(the array the evaluator reads, its C API code, its values as float64) of float64 X as dtype;
    bfloat16 is the upper half of a float32, kept as uint16"""
    with np.errstate(over="ignore"):
        if dtype == "bfloat16":
            bits = (X.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
            return bits, nat.DTYPE_BFLOAT16, (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        a = X.astype(dtype)
    code = {"float16": nat.DTYPE_FLOAT16, "float32": nat.DTYPE_FLOAT32, "float64": nat.DTYPE_FLOAT64}[dtype]
    return a, code, a.astype(np.float64)


def on_host(bst, a, code, ptype, start, num):
    n, ncol = a.shape
    width = ctypes.c_int64(0)
    nat.call("LGBM_BoosterCalcNumPredict", bst.handle, nat.c_int(1), nat.c_int(ptype), nat.c_int(start), nat.c_int(num),
             ctypes.byref(width))
    out = np.full((n, width.value), np.nan)
    nat.call("LGBM_AMD_TensorPredictOnHost", bst.handle, ctypes.c_void_p(a.ctypes.data), nat.c_int(code),
             ctypes.c_int64(n), ctypes.c_int32(ncol), ctypes.c_int64(a.strides[0] // a.itemsize),
             ctypes.c_int64(a.strides[1] // a.itemsize), nat.c_int(ptype), nat.c_int(start), nat.c_int(num),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int64(out.size))
    return out


@pytest.mark.parametrize("route", ["plan", "slots"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32", "float64"])
@pytest.mark.parametrize("name", fr.DEVICE_FORESTS)
def test_evaluator_equals_the_walker(name, dtype, route, monkeypatch):
    """257 rows: a full tile of 256 and a tile of one row; contiguous, and a view with both strides
    non-unit"""
    if route == "slots":
        monkeypatch.setenv("LGBM_AMD_TENSOR_PREDICT_SLOTS", "1")
    f = fr.FORESTS[name]
    bst = lgb.Booster(model_str=f.text)
    a, code, values = elements(f.tiled(257), dtype)
    raw, leaf = fr.walk(f.text, values, f.start, f.num)
    base = np.zeros((2 * a.shape[0], 3 * a.shape[1]), dtype=a.dtype)
    base[::2, ::3] = a
    for what, m in (("contiguous", a), ("strided", base[::2, ::3])):
        assert np.array_equal(on_host(bst, m, code, RAW, f.start, f.num), raw), (what, "raw")
        assert np.array_equal(on_host(bst, m, code, LEAF, f.start, f.num), leaf), (what, "leaf")
