"""The objective output transforms behind custom metrics on GPU tensors, without a GPU.

* LGBM_AMD_ConvertScores -- the host evaluator of src/device/score_convert.h, the rule the export
  kernel applies -- against float64 NumPy formulas for every kind, over the edge values of
  tests/helpers/convert_cases.py (0, +-tiny, +-700, +-inf, ...) and 2, 3 and 17 classes, within
  the bound derived there; kinds 0 and 2 bit for bit.
* Against the host objectives themselves: what LGBM_BoosterGetPredict returns for a CPU booster
  must be the evaluator applied to its raw scores bit for bit (the same arithmetic in the same
  order); the raw scores are read again after the objective was reset to none.
* lightgbmv1_amd.on_device marks a callable; a marked fobj / feval on a booster without a device
  learner raises and names device_type=gpu; the device entry points of the C API fail with a
  message for such a booster, and LGBM_AMD_BoosterDeviceId gives -1.
"""
import ctypes

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from lightgbmv1_amd.basic import _load_lib

from helpers import convert_cases as cc


def _convert(kind, param, scores):
    s = np.ascontiguousarray(scores, dtype=np.float64)
    out = np.empty_like(s)
    nat.call("LGBM_AMD_ConvertScores", ctypes.c_int(kind), ctypes.c_double(param), ctypes.c_int(s.shape[0]),
             ctypes.c_int64(s.shape[1]), s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return out


@pytest.mark.parametrize("kind,param,num_class", [(0, 0.0, 1), (0, 0.0, 3), (1, 1.0, 1), (1, 2.5, 1), (2, 0.0, 1),
                                                  (3, 0.0, 1), (4, 0.0, 2), (4, 0.0, 3), (4, 0.0, 17), (5, 0.7, 3),
                                                  (5, 1.0, 17)])
def test_evaluator_against_numpy(kind, param, num_class):
    scores = cc.edge_scores(num_class)
    got = _convert(kind, param, scores)
    cc.assert_within_bound(got, cc.reference(kind, param, scores), kind, num_class, "host evaluator")


def test_softmax_rows_sum_to_one():
    for k in (2, 3, 17):
        scores = cc.edge_scores(k)
        p = _convert(4, 0.0, scores)
        total = np.zeros(p.shape[1])
        for c in range(k):
            total = total + p[c]
        ok = np.isfinite(total)
        assert ok.sum() > 300
        assert np.max(np.abs(total[ok] - 1.0)) <= cc.softmax_row_sum_bound(k)


def test_evaluator_in_place_and_bad_kind():
    scores = cc.edge_scores(3)
    want = _convert(4, 0.0, scores)
    buf = scores.copy()
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    nat.call("LGBM_AMD_ConvertScores", ctypes.c_int(4), ctypes.c_double(0.0), ctypes.c_int(3),
             ctypes.c_int64(buf.shape[1]), p, p)
    assert np.array_equal(buf.view(np.uint64), want.view(np.uint64))
    with pytest.raises(lgb.LightGBMError, match="kind"):
        _convert(6, 0.0, scores)


def _data(n=500, classes=0, seed=3):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, 5)
    if classes:
        y = (np.argmax(X[:, :classes], axis=1)).astype(np.float64)
    else:
        y = (X[:, 0] + 0.3 * X[:, 1] > 0).astype(np.float64)
    return X, y


def _get_predict(booster, n_total):
    out = np.empty(n_total, dtype=np.float64)
    got = ctypes.c_int64(0)
    nat.call("LGBM_BoosterGetPredict", booster.handle, ctypes.c_int(0), ctypes.byref(got),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert got.value == n_total
    return out


OBJECTIVES = [
    ("binary", {"objective": "binary", "sigmoid": 1.7}, 0, 1, 1.7),
    ("multiclass", {"objective": "multiclass", "num_class": 3}, 3, 4, 0.0),
    ("multiclassova", {"objective": "multiclassova", "num_class": 3, "sigmoid": 0.8}, 3, 5, 0.8),
    ("poisson", {"objective": "poisson"}, 0, 3, 0.0),
    ("reg_sqrt", {"objective": "regression", "reg_sqrt": True}, 0, 2, 0.0),
    ("cross_entropy", {"objective": "cross_entropy"}, 0, 1, 1.0),
]


@pytest.mark.parametrize("name,params,classes,kind,param", OBJECTIVES, ids=[o[0] for o in OBJECTIVES])
def test_evaluator_is_the_host_objective_bit_for_bit(name, params, classes, kind, param):
    X, y = _data(classes=classes)
    params = dict(params, device_type="cpu", num_leaves=7, min_data_in_leaf=5, verbose=-1, num_threads=1)
    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    for _ in range(4):
        booster.update()
    k = max(1, classes)
    converted = _get_predict(booster, len(y) * k)
    booster.reset_parameter({"objective": "none"})
    raw = _get_predict(booster, len(y) * k)
    assert not np.array_equal(raw, converted)
    got = _convert(kind, param, raw.reshape(k, len(y)))
    assert np.array_equal(got.reshape(-1).view(np.uint64), converted.view(np.uint64)), \
        "%s: %d of %d values differ" % (name, int(np.sum(got.reshape(-1) != converted)), got.size)


# ---------------------------------------------------------------- the mark, and boosters without a device learner
def test_on_device_marks_and_returns_the_callable():
    def f(preds, data):
        return preds, preds

    assert lgb.on_device(f) is f
    assert "on_device" in lgb.__all__

    @lgb.on_device
    def g(preds, data):
        return "m", 0.0, False

    assert g(None, None) == ("m", 0.0, False)

    class Callable:
        def __call__(self, preds, data):
            return None

    c = Callable()
    assert lgb.on_device(c) is c


def _cpu_booster():
    X, y = _data(200)
    params = {"objective": "binary", "device_type": "cpu", "num_leaves": 4, "verbose": -1, "num_threads": 1}
    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    booster.update()
    return booster, X, y


def test_marked_callables_need_a_device_learner():
    booster, X, y = _cpu_booster()
    called = []

    @lgb.on_device
    def fobj(preds, data):
        called.append(type(preds))
        return preds, preds

    @lgb.on_device
    def feval(preds, data):
        called.append(type(preds))
        return "m", 0.0, False

    with pytest.raises(lgb.LightGBMError, match="device_type=gpu"):
        booster.update(fobj=fobj)
    with pytest.raises(lgb.LightGBMError, match="device_type=gpu"):
        booster.eval_train(feval)
    with pytest.raises(lgb.LightGBMError, match="device_type=gpu"):
        booster.device_scores()
    assert not called  # (nothing was handed NumPy instead)
    # the booster still trains with its own objective and with an unmarked callable
    booster.update()
    booster.update(fobj=lambda preds, data: (preds - data.get_label(), np.ones_like(preds)))
    assert booster.current_iteration() == 3


def test_c_entry_points_refuse_a_cpu_booster():
    booster, X, y = _cpu_booster()
    lib = _load_lib()
    lib.LGBM_GetLastError.restype = ctypes.c_char_p
    dev = ctypes.c_int(7)
    assert lib.LGBM_AMD_BoosterDeviceId(booster.handle, ctypes.byref(dev)) == 0 and dev.value == -1
    n = len(y)
    assert lib.LGBM_AMD_BoosterGetPredictDevice(booster.handle, ctypes.c_int(0), ctypes.c_int(1), ctypes.c_void_p(0),
                                                ctypes.c_int64(n)) == -1
    assert b"device_type=gpu" in lib.LGBM_GetLastError()
    fin = ctypes.c_int(0)
    g = np.zeros(n, dtype=np.float32)  # (never read: the call fails on the booster)
    p = ctypes.c_void_p(g.ctypes.data)
    assert lib.LGBM_AMD_BoosterUpdateOneIterCustomDevice(booster.handle, p, p, ctypes.c_int(0), ctypes.c_int64(n),
                                                         ctypes.byref(fin)) == -1
    assert b"device_type=gpu" in lib.LGBM_GetLastError()
    assert booster.current_iteration() == 1
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.LGBM_AMD_DeviceCustomStats(ctypes.byref(a), ctypes.byref(b)) == 0
    assert a.value >= 0 and b.value >= 0
