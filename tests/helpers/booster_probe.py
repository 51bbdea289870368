"""Reading a booster's state through the C API: the gradients of its last iteration and its
training scores (shared by tests/test_gpu_learner.py and tests/test_rank_refs_host.py)."""
import ctypes

import numpy as np


def last_gradients(bst):
    """(grad, hess) of the booster's last iteration (LGBM_AMD_BoosterLastGradients)"""
    from lightgbmv1_amd.basic import _load_lib, _safe_call
    _LIB = _load_lib()
    n = ctypes.c_int64(0)
    _safe_call(_LIB.LGBM_AMD_BoosterLastGradients(bst.handle, None, None, ctypes.byref(n)))
    g = np.zeros(n.value, dtype=np.float32)
    h = np.zeros(n.value, dtype=np.float32)
    _safe_call(_LIB.LGBM_AMD_BoosterLastGradients(bst.handle, g.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                  h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(n)))
    return g, h


def train_scores(bst, n):
    """the booster's training scores (LGBM_BoosterGetPredict, data 0)"""
    from lightgbmv1_amd.basic import _load_lib, _safe_call
    buf = np.zeros(n, dtype=np.float64)
    got = ctypes.c_int64(0)
    _safe_call(_load_lib().LGBM_BoosterGetPredict(bst.handle, ctypes.c_int(0), ctypes.byref(got),
                                                  buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    assert got.value == n
    return buf
