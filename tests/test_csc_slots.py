"""The compact matrix of device CSC prediction, evaluated on the host (LGBM_AMD_CscToSlots: the
rule of a stored entry in src/device/csc_slots.h, shared with src/device/csc_kernels.hip) against
NumPy: the used features are the sorted split features of the window's trees, and the matrix is
csc_meaning(...)[row0:row0 + rows, used] (tests/helpers/csc_cases.py) -- absent entries 0, stored
zeros and NaN kept, columns the model does not have ignored, entries whose row is outside the
window dropped, and of several stored entries on one cell the last stored one.  Needs no GPU.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from helpers import contrib_cases as cc
from helpers import csc_cases as csc

NCOL = 200
INFORMATIVE = [3, 17, 42, 99, 150, 199]


@pytest.fixture(scope="module")
def booster():
    """(the booster of tests/test_csr_slots.py)"""
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


def _slots(booster, col_ptr, indices, data, num_row, row0=0, rows=None, start=0, num=-1, nelem=None):
    """(used, compact matrix) of LGBM_AMD_CscToSlots for raw CSC arrays and a window of rows"""
    rows = num_row - row0 if rows is None else rows
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    p_ptr, p_code = nat.pointer(col_ptr)
    v_ptr, v_code = nat.pointer(data)
    common = (booster.handle, p_ptr, nat.c_int(p_code), indices.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v_ptr,
              nat.c_int(v_code), ctypes.c_int64(len(col_ptr)), ctypes.c_int64(len(data) if nelem is None else nelem),
              ctypes.c_int64(num_row), ctypes.c_int64(row0), ctypes.c_int64(rows), nat.c_int(start), nat.c_int(num))
    n = ctypes.c_int32(-1)
    used = np.full(booster.num_feature(), -1, dtype=np.int32)
    nat.call("LGBM_AMD_CscToSlots", *common, ctypes.byref(n), used.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None)
    used = used[:n.value]
    guard = 3  # (rows after the matrix that the call must leave alone)
    mat = np.full((rows + guard, n.value), 7, dtype=data.dtype)
    n2 = ctypes.c_int32(-1)
    nat.call("LGBM_AMD_CscToSlots", *common, ctypes.byref(n2), None, mat.ctypes.data_as(ctypes.c_void_p))
    assert n2.value == n.value and np.all(mat[rows:] == 7)
    return used, mat[:rows]


def _random_csc(rng, rows, ncol, density, dtype):
    m = sp.random(rows, ncol, density=density, format="csc", random_state=rng, dtype=np.float64)
    m.data = rng.randn(len(m.data))
    return m.astype(dtype)


def test_used_features_are_the_windows_split_features(booster):
    m = _random_csc(np.random.RandomState(0), 5, NCOL, 0.1, np.float64)
    used, _ = _slots(booster, m.indptr, m.indices, m.data, 5)
    want = _split_features(booster)
    assert 3 <= len(want) <= len(INFORMATIVE) and set(want) <= set(INFORMATIVE)
    assert used.tolist() == want
    # a window of the first trees only: (possibly) fewer features, from those trees alone
    for start, num in ((0, 1), (2, 3), (11, 1)):
        used_w, mat = _slots(booster, m.indptr, m.indices, m.data, 5, start=start, num=num)
        assert used_w.tolist() == _split_features(booster, start, num)
        assert np.array_equal(mat, m.toarray()[:, used_w])


@pytest.mark.parametrize("ptr_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_canonical_and_shuffled_columns(booster, dtype, ptr_dtype):
    rng = np.random.RandomState(3)
    m = _random_csc(rng, 300, NCOL, 0.15, dtype)
    m.data[::11] = np.nan  # (a stored NaN is a value)
    m.data[::7] = 0.0      # (so is a stored zero)
    col_ptr = m.indptr.astype(ptr_dtype)
    want = m.toarray()     # (canonical: no cell twice)
    assert np.array_equal(want, csc.csc_meaning(col_ptr, m.indices, m.data, 300, NCOL), equal_nan=True)
    used, mat = _slots(booster, col_ptr, m.indices, m.data, 300)
    assert mat.dtype == dtype and mat.shape == (300, len(used)) and len(used) > 0
    assert np.array_equal(mat, want[:, used], equal_nan=True)
    assert np.isnan(mat).any() and np.isnan(want[:, used]).sum() == np.isnan(mat).sum()
    # the same entries in another order within each column (has_sorted_indices == False is legal)
    indices, data = csc.shuffled_within_columns(rng, col_ptr, m.indices, m.data)
    assert not np.array_equal(indices, m.indices)
    _, mat_s = _slots(booster, col_ptr, indices, data, 300)
    assert np.array_equal(mat_s, want[:, used], equal_nan=True)


def test_repeated_cells_empty_and_foreign_columns_and_rows_outside_the_matrix(booster):
    used = _split_features(booster)
    unused = next(c for c in range(NCOL) if c not in used)
    num_row = 12
    columns, want = csc.hostile(used, unused, NCOL, num_row)
    for ptr_dtype in (np.int32, np.int64):
        for dtype in (np.float32, np.float64):
            col_ptr, indices, data = csc.from_columns(columns, dtype, ptr_dtype)
            assert indices.min() == -1 and indices.max() == 2 ** 31 - 1 and num_row in indices
            assert np.array_equal(csc.csc_meaning(col_ptr, indices, data, num_row, NCOL), want.astype(dtype), equal_nan=True)
            got_used, mat = _slots(booster, col_ptr, indices, data, num_row)
            assert got_used.tolist() == used
            assert np.array_equal(mat, want[:, used].astype(dtype), equal_nan=True)
    # a matrix of empty columns only
    _, mat = _slots(booster, np.zeros(NCOL + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32), 4)
    assert mat.shape == (4, len(used)) and not mat.any()


def test_matrix_narrower_than_the_model(booster):
    used = _split_features(booster)
    ncol = used[-2] + 1  # (the last used feature, at least, is no column of the matrix)
    m = _random_csc(np.random.RandomState(5), 40, ncol, 0.3, np.float64)
    got_used, mat = _slots(booster, m.indptr, m.indices, m.data, 40)
    assert got_used.tolist() == used
    want = np.zeros((40, NCOL))
    want[:, :ncol] = m.toarray()
    assert np.array_equal(mat, want[:, used]) and not mat[:, -1].any() and mat[:, :-1].any()


def test_row_windows_are_slices_of_the_whole(booster):
    rng = np.random.RandomState(6)
    m = _random_csc(rng, 97, NCOL, 0.2, np.float32)
    indices, data = csc.shuffled_within_columns(rng, m.indptr, m.indices, m.data, INFORMATIVE[::2])
    n, k = 97, 31
    _, whole = _slots(booster, m.indptr, indices, data, n, 0, n)
    assert whole.any() and np.array_equal(whole, m.toarray()[:, _split_features(booster)])
    for row0, rows in ((k, 1), (k, n - k), (0, k), (n - 1, 1), (k, 0)):
        _, part = _slots(booster, m.indptr, indices, data, n, row0, rows)
        assert part.shape[0] == rows and np.array_equal(part, whole[row0:row0 + rows])


def test_pointer_past_the_entries_is_clamped(booster):
    m = _random_csc(np.random.RandomState(7), 50, NCOL, 0.2, np.float64)
    nelem = int(m.indptr[INFORMATIVE[3]]) + 2  # (ends inside a used column)
    assert nelem < m.nnz
    used, mat = _slots(booster, m.indptr, m.indices, m.data, 50, nelem=nelem)
    col_ptr = np.minimum(m.indptr, nelem)
    want = csc.csc_meaning(col_ptr, m.indices[:nelem], m.data[:nelem], 50, NCOL)
    assert np.array_equal(mat, want[:, used]) and not np.array_equal(mat, m.toarray()[:, used])


def test_single_leaf_model_uses_no_feature():
    c = cc.case("single_leaf")
    m = sp.csc_matrix(c.X[:50])
    used, mat = _slots(c.booster, m.indptr, m.indices, m.data, 50)
    assert used.size == 0 and mat.shape == (50, 0)


def test_prediction_and_binning_walk_columns_with_one_set_of_constants():
    """Both CSC paths walk a column by src/device/stored_order.h: a segment length or a workgroup
    size of its own on either side would fork the walk again."""
    from lightgbmv1_amd import ops
    predict, binning = ops.csc_launch_info(), ops.csc_bin_launch_info()
    for key in ("segment_entries", "block", "batch"):
        assert predict[key] == binning[key], key


def test_pack_column_runs_native_driver(tmp_path):
    """PackColumnRuns (include/lgbm_amd/sparse_ptr.h), which both CSC paths upload their columns
    by, has no entry point of its own: tests/native/csc_slots_driver.cpp checks its runs and every
    column's place against a direct computation (adjacent columns, an empty column between two
    used ones, a gap, columns past the matrix's width, a single column).  The plain build of the
    program; tests/test_csc_slots_sanitized.py has the sanitized one."""
    import os
    import shutil
    import subprocess
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = tmp_path / "csc_slots_driver"
    build = subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(root, "tests", "native", "csc_slots_driver.cpp"),
                            "-o", str(driver)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    out = subprocess.run([str(driver)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "csc slots driver ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
