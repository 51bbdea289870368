"""The compact matrix of device CSR prediction, evaluated on the host (LGBM_AMD_CsrToSlots: the
rule of a stored entry in src/device/csr_slots.h, shared with src/device/csr_kernels.hip) against
NumPy: the used features are the sorted split features of the window's trees, and the matrix is
X.toarray()[:, used] -- absent entries 0, stored zeros and NaN kept, columns the model does not
have ignored, and of two stored entries on one column of a row the last one.  Needs no GPU.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from helpers import contrib_cases as cc

NCOL = 200
INFORMATIVE = [3, 17, 42, 99, 150, 199]


@pytest.fixture(scope="module")
def booster():
    rng = np.random.RandomState(21)
    X = np.zeros((600, NCOL))
    X[:, INFORMATIVE] = rng.randn(600, len(INFORMATIVE))  # (the other columns are constant: never split on)
    y = X[:, 3] - X[:, 42] * X[:, 150] + np.sin(X[:, 199]) + 0.5 * X[:, 17] + 0.3 * X[:, 99] + 0.1 * rng.randn(600)
    p = {"objective": "regression", "num_leaves": 7, "min_data_in_leaf": 5, "verbose": -1, "num_threads": 2, "seed": 1}
    return lgb.train(p, lgb.Dataset(X, y, params=p), num_boost_round=12)


def _split_features(booster, start=0, num=-1):
    trees = booster.dump_model()["tree_info"]
    stop = len(trees) if num <= 0 else min(len(trees), start + num)
    found = set()

    def walk(node):
        if "split_feature" in node:
            found.add(node["split_feature"])
            walk(node["left_child"])
            walk(node["right_child"])

    for t in trees[start:stop]:
        walk(t["tree_structure"])
    return sorted(found)


def _slots(booster, indptr, indices, data, start=0, num=-1):
    """(used, compact matrix) of LGBM_AMD_CsrToSlots for raw CSR arrays"""
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    p_ptr, p_code = nat.pointer(indptr)
    v_ptr, v_code = nat.pointer(data)
    common = (booster.handle, p_ptr, nat.c_int(p_code), indices.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v_ptr,
              nat.c_int(v_code), ctypes.c_int64(len(indptr)), ctypes.c_int64(len(data)), nat.c_int(start),
              nat.c_int(num))
    n = ctypes.c_int32(-1)
    used = np.full(booster.num_feature(), -1, dtype=np.int32)
    nat.call("LGBM_AMD_CsrToSlots", *common, ctypes.byref(n), used.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None)
    used = used[:n.value]
    mat = np.full((len(indptr) - 1, n.value), 7, dtype=data.dtype)
    n2 = ctypes.c_int32(-1)
    nat.call("LGBM_AMD_CsrToSlots", *common, ctypes.byref(n2), None, mat.ctypes.data_as(ctypes.c_void_p))
    assert n2.value == n.value
    return used, mat


def _random_csr(rng, rows, ncol, density, dtype):
    m = sp.random(rows, ncol, density=density, format="csr", random_state=rng, dtype=np.float64)
    m.data = rng.randn(len(m.data))
    return m.astype(dtype)


def test_used_features_are_the_windows_split_features(booster):
    m = _random_csr(np.random.RandomState(0), 5, NCOL, 0.1, np.float64)
    used, _ = _slots(booster, m.indptr, m.indices, m.data)
    want = _split_features(booster)
    assert 0 < len(want) <= len(INFORMATIVE) and set(want) <= set(INFORMATIVE)
    assert used.tolist() == want
    # a window of the first trees only: (possibly) fewer features, from those trees alone
    for start, num in ((0, 1), (2, 3), (11, 1)):
        used_w, mat = _slots(booster, m.indptr, m.indices, m.data, start, num)
        assert used_w.tolist() == _split_features(booster, start, num)
        assert np.array_equal(mat, m.toarray()[:, used_w])


@pytest.mark.parametrize("ptr_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_canonical_and_shuffled_rows(booster, dtype, ptr_dtype):
    rng = np.random.RandomState(3)
    m = _random_csr(rng, 300, NCOL, 0.15, dtype)
    m.data[::11] = np.nan  # (a stored NaN is a value)
    m.data[::7] = 0.0      # (so is a stored zero)
    indptr = m.indptr.astype(ptr_dtype)
    want = m.toarray()
    used, mat = _slots(booster, indptr, m.indices, m.data)
    assert mat.dtype == dtype and mat.shape == (300, len(used)) and len(used) > 0
    assert np.array_equal(mat, want[:, used], equal_nan=True)
    assert np.isnan(mat).any() and np.isnan(want[:, used]).sum() == np.isnan(mat).sum()
    # the same entries in another order within each row (has_sorted_indices == False is legal)
    indices, data = m.indices.copy(), m.data.copy()
    for r in range(300):
        perm = rng.permutation(indptr[r + 1] - indptr[r]) + indptr[r]
        indices[indptr[r]:indptr[r + 1]] = indices[perm]
        data[indptr[r]:indptr[r + 1]] = data[perm]
    assert not np.array_equal(indices, m.indices)
    _, mat_s = _slots(booster, indptr, indices, data)
    assert np.array_equal(mat_s, want[:, used], equal_nan=True)


def test_duplicates_empty_rows_and_foreign_columns(booster):
    used = _split_features(booster)
    u0, u1 = used[0], used[-1]
    unused = next(c for c in range(NCOL) if c not in used)
    rows = [
        ([u0, unused, u0], [1.0, 2.0, 3.0]),              # one column twice: the last stored entry wins
        ([], []),                                          # an empty row
        ([u1, u0, u1, u1], [4.0, 5.0, 0.0, -6.0]),         # three times, a stored zero in between
        ([NCOL, u0, NCOL + 1000, 2 ** 31 - 1], [9.0, 8.0, 9.0, 9.0]),  # columns the model does not have
        ([], []),
        ([u1, u1], [7.0, 0.0]),                            # the last one is a stored zero
        ([-1, u1], [5.0, 2.5]),                            # (a negative column is no feature either)
    ]
    indptr = np.cumsum([0] + [len(c) for c, _ in rows])
    indices = np.array([c for cs, _ in rows for c in cs], dtype=np.int32)
    data = np.array([v for _, vs in rows for v in vs], dtype=np.float64)
    want = np.zeros((len(rows), NCOL))
    want[0, u0], want[2, u1], want[2, u0], want[3, u0], want[5, u1], want[6, u1] = 3.0, -6.0, 5.0, 8.0, 0.0, 2.5
    for ptr_dtype in (np.int32, np.int64):
        for dtype in (np.float32, np.float64):
            got_used, mat = _slots(booster, indptr.astype(ptr_dtype), indices, data.astype(dtype))
            assert got_used.tolist() == used
            assert np.array_equal(mat, want[:, used].astype(dtype))
    # a matrix of empty rows only
    _, mat = _slots(booster, np.zeros(5, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    assert mat.shape == (4, len(used)) and not mat.any()


def test_single_leaf_model_uses_no_feature():
    c = cc.case("single_leaf")
    m = sp.csr_matrix(c.X[:50])
    used, mat = _slots(c.booster, m.indptr, m.indices, m.data)
    assert used.size == 0 and mat.shape == (50, 0)
