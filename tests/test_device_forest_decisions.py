"""Device prediction against the walker of tests/helpers/forest_ref.py, which applies the decision
rule of a node as that module writes it down and shares no code with the project
(tests/test_forest_ref_host.py holds the host predictor to the same walker without a GPU).  The
hand-written forests meet every edge value of a split: NaN at a categorical node, values in
(-1, 0), categories past the bitset, +-1e-35, a float32 just beyond a float64 threshold, 16
trees per iteration.  Raw scores (k_predict_forest) and leaf indices (k_predict_leaf) must equal
the walker's; contributions (k_shap_forest) are within cc.tolerance of the host's and their rows
sum to the walker's raw score within (F + 1) times that.  Routes: ops.forest_predict on dense and
sparse_csr GPU tensors, Booster.predict on row-major, column-major and CSR host matrices in one
and in two chunks.  LGBM_AMD_DevicePredictCount is asserted on every call.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch  # (before the native library loads, as in tests/test_ops.py: one HIP runtime for both)

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from lightgbmv1_amd import ops
from helpers import contrib_cases as cc
from helpers import forest_ref as fr

pytestmark = pytest.mark.gpu

GPU = {"device_type": "gpu"}
DTYPES = [np.float32, np.float64]
KINDS = {"raw": {"raw_score": True}, "leaf": {"pred_leaf": True}, "contrib": {"pred_contrib": True}}
CODES = {"raw": nat.PREDICT_RAW_SCORE, "leaf": nat.PREDICT_LEAF_INDEX, "contrib": nat.PREDICT_CONTRIB}


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    pass


def _device_calls():
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DevicePredictCount", ctypes.byref(out))
    return out.value


def _dense(pred):
    if isinstance(pred, list):
        return np.hstack([p.toarray() for p in pred])
    return pred.toarray() if sp.issparse(pred) else pred


def _device(booster, X, **kw):
    before = _device_calls()
    out = _dense(booster.predict(X, **kw, **GPU))
    assert _device_calls() == before + 1, "the prediction did not run on the device"
    return np.asarray(out, dtype=np.float64).reshape(X.shape[0], -1)


def cast(X, dtype):
    with np.errstate(over="ignore"):  # (1e300 is inf as float32: the walker takes what the cast gives)
        return np.ascontiguousarray(np.asarray(X).astype(dtype))


@functools.lru_cache(maxsize=None)
def case_of(name):
    f = fr.FORESTS[name]
    return cc.Case(lgb.Booster(model_str=f.text), f.rows, f.start, f.num)


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(raw, leaf) of the walker and the host predictor's contributions for the forest's probing
    rows as `dtype`, computed once; a test takes the rows it predicts with take()"""
    f, c = fr.FORESTS[name], case_of(name)
    X = cast(f.rows, dtype)
    raw, leaf = fr.walk(f.text, X, f.start, f.num)
    before = _device_calls()
    contrib = c.booster.predict(X, pred_contrib=True, **c.window)  # (no device_type: the host predictor)
    assert _device_calls() == before
    return raw, leaf, np.asarray(contrib, dtype=np.float64).reshape(len(X), -1)


def take(name, dtype, n):
    idx = np.arange(n) % len(fr.FORESTS[name].rows)
    return {k: v[idx] for k, v in zip(("raw", "leaf", "contrib"), reference(name, dtype))}


def check(got, want, name, what):
    """got / want: dicts of raw, leaf, contrib"""
    for k in ("raw", "leaf"):
        assert got[k].shape == want[k].shape, (what, k)
        bad = np.nonzero((got[k] != want[k]).any(axis=1))[0]
        assert bad.size == 0, "%s: %s of rows %s differ from the walker" % (what, k, bad[:8])
    cc.check_contrib(got["contrib"], want["contrib"], want["raw"], case_of(name), what)


def mixed_csr(X, index_dtype=np.int32):
    """(indptr, indices, data, columns) of the rows of X with, by turns, the zeros absent or stored,
    one column stored twice (a decoy first: the last stored entry is the value), an entry on a
    column past the model's, a stored NaN and a stored 1e-36; and the dense matrix that this means
    (where the column stored twice holds an absent zero, the decoy is its only entry, and the value)"""
    X = X.copy()
    n, f = X.shape
    X[1::7, 0] = np.nan
    X[2::7, f - 1] = 1e-36
    indptr, indices, data = [0], [], []
    for r in range(n):
        if r % 3 == 0:
            indices.append(r % f)
            data.append(5.0)
        if r % 4 == 0:
            indices.append(f)
            data.append(3.0)
        for j in range(f):
            if X[r, j] != 0 or r % 2 == 1:  # (NaN != 0: stored)
                indices.append(j)
                data.append(X[r, j])
        indptr.append(len(indices))
    indptr, indices = np.array(indptr, dtype=index_dtype), np.array(indices, dtype=np.int32)
    data = np.array(data, dtype=X.dtype)
    twice = [r for r in range(n) if len(set(indices[indptr[r]:indptr[r + 1]])) < indptr[r + 1] - indptr[r]]
    assert twice and np.isnan(data).any() and (data == 0).any() and (indices == f).any() and (np.diff(indptr) < f).any()
    return (indptr, indices, data, f + 1), fr.csr_meaning(indptr, indices, data, f)


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
@pytest.mark.parametrize("name", fr.DEVICE_FORESTS)
def test_ops_on_dense_tensors(name, rows):
    f, c = fr.FORESTS[name], case_of(name)
    for dtype in DTYPES:
        Xd = torch.tensor(cast(f.tiled(rows), dtype), device="cuda")
        before = _device_calls()
        got = {k: ops.forest_predict(c.booster, Xd, kind=k, start_iteration=f.start, num_iteration=f.num)
               for k in KINDS}
        assert _device_calls() == before + 3
        assert all(t.is_cuda and t.dtype == torch.float64 for t in got.values())
        check({k: t.cpu().numpy() for k, t in got.items()}, take(name, dtype, rows), name,
              "ops %s %d rows %s" % (name, rows, np.dtype(dtype).name))


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", fr.DEVICE_FORESTS)
def test_ops_on_sparse_csr_tensors(name, index_dtype):
    f, c = fr.FORESTS[name], case_of(name)
    for dtype in DTYPES:
        (indptr, indices, data, cols), X = mixed_csr(cast(f.tiled(257), dtype))
        Xs = torch.sparse_csr_tensor(torch.tensor(indptr).to(index_dtype), torch.tensor(indices).to(index_dtype),
                                     torch.tensor(data), size=(257, cols), device="cuda", check_invariants=False)
        assert Xs.crow_indices().dtype == index_dtype and Xs.values().dtype == torch.tensor(data).dtype
        raw, leaf = fr.walk(f.text, X, f.start, f.num)
        contrib = c.booster.predict(X, pred_contrib=True, **c.window).reshape(257, -1)  # (the host predictor)
        before = _device_calls()
        got = {k: ops.forest_predict(c.booster, Xs, kind=k, start_iteration=f.start, num_iteration=f.num).cpu().numpy()
               for k in KINDS}
        assert _device_calls() == before + 3
        check(got, {"raw": raw, "leaf": leaf, "contrib": contrib}, name,
              "ops csr %s %s %s" % (name, index_dtype, np.dtype(dtype).name))


def _for_mat(booster, X, kind, width, start, num, params="device_type=gpu"):
    """LGBM_BoosterPredictForMat on X in the layout it has (row- or column-major)"""
    row_major = X.flags["C_CONTIGUOUS"]
    assert row_major or X.flags["F_CONTIGUOUS"]
    out = np.empty((X.shape[0], width))
    got = ctypes.c_int64(0)
    nat.call("LGBM_BoosterPredictForMat", booster.handle, X.ctypes.data_as(ctypes.c_void_p),
             nat.c_int(nat.DTYPE_FLOAT32 if X.dtype == np.float32 else nat.DTYPE_FLOAT64),
             ctypes.c_int32(X.shape[0]), ctypes.c_int32(X.shape[1]), nat.c_int(1 if row_major else 0),
             nat.c_int(CODES[kind]), nat.c_int(start), nat.c_int(num), nat.cstr(params), ctypes.byref(got),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert got.value == out.size
    return out


@pytest.mark.parametrize("rows,chunk", [(1024, None), (1025, None), (1025, "1024")])
@pytest.mark.parametrize("name", fr.DEVICE_FORESTS)
def test_booster_predict_on_dense_matrices(name, rows, chunk, monkeypatch):
    """1025 rows in chunks of 1024: the last chunk is one row"""
    f, c = fr.FORESTS[name], case_of(name)
    if chunk:
        monkeypatch.setenv("LGBM_AMD_PREDICT_CHUNK_ROWS", chunk)
    for dtype in DTYPES:
        X = cast(f.tiled(rows), dtype)
        want = take(name, dtype, rows)
        check({k: _device(c.booster, X, **kw, **c.window) for k, kw in KINDS.items()}, want, name,
              "%s %d rows %s" % (name, rows, np.dtype(dtype).name))
        Xf = np.asfortranarray(X)
        before = _device_calls()
        got = {k: _for_mat(c.booster, Xf, k, want[k].shape[1], f.start, f.num) for k in KINDS}
        assert _device_calls() == before + 3
        check(got, want, name, "%s %d rows %s column-major" % (name, rows, np.dtype(dtype).name))


@pytest.mark.parametrize("name", fr.DEVICE_FORESTS)
def test_booster_predict_on_csr_matrices(name):
    f, c = fr.FORESTS[name], case_of(name)
    for dtype in DTYPES:
        (indptr, indices, data, cols), X = mixed_csr(cast(f.tiled(1024), dtype))
        m = sp.csr_matrix((data, indices, indptr), shape=(1024, cols))
        assert m.dtype == dtype and m.nnz == len(data)
        raw, leaf = fr.walk(f.text, X, f.start, f.num)
        contrib = c.booster.predict(X, pred_contrib=True, **c.window).reshape(1024, -1)  # (the host predictor)
        kw = dict(c.window, predict_disable_shape_check=True)  # (one column more than the model has)
        got = {k: _device(c.booster, m, **KINDS[k], **kw) for k in ("raw", "leaf")}
        # (Booster.predict returns a sparse input's contributions in the input's type: the doubles
        # come from LGBM_BoosterPredictForCSR)
        p_ptr, p_code = nat.pointer(m.indptr)
        v_ptr, v_code = nat.pointer(m.data)
        got["contrib"] = np.empty_like(contrib)
        n_out = ctypes.c_int64(0)
        before = _device_calls()
        nat.call("LGBM_BoosterPredictForCSR", c.booster.handle, p_ptr, ctypes.c_int32(p_code),
                 m.indices.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v_ptr, nat.c_int(v_code),
                 ctypes.c_int64(len(m.indptr)), ctypes.c_int64(len(m.data)), ctypes.c_int64(cols),
                 nat.c_int(nat.PREDICT_CONTRIB), nat.c_int(f.start), nat.c_int(f.num),
                 nat.cstr("device_type=gpu predict_disable_shape_check=true"), ctypes.byref(n_out),
                 got["contrib"].ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert n_out.value == contrib.size and _device_calls() == before + 1
        check(got, {"raw": raw, "leaf": leaf, "contrib": contrib}, name, "%s csr %s" % (name, np.dtype(dtype).name))


def test_seventeen_trees_per_iteration_stay_on_the_host():
    f = fr.FORESTS["classes17"]
    bst = lgb.Booster(model_str=f.text)
    X = f.tiled(1024)
    raw, leaf = fr.walk(f.text, X)
    before = _device_calls()
    assert np.array_equal(bst.predict(X, raw_score=True, **GPU), raw)
    assert np.array_equal(bst.predict(X, pred_leaf=True, **GPU), leaf)
    assert np.array_equal(bst.predict(sp.csr_matrix(X), raw_score=True, **GPU), raw)
    assert _device_calls() == before, "17 trees per iteration do not fit the kernel's accumulators"
    Xd = torch.tensor(X[:64], device="cuda")
    for kind in KINDS:
        with pytest.raises(lgb.LightGBMError):
            ops.forest_predict(bst, Xd, kind=kind)
        with pytest.raises(lgb.LightGBMError):
            ops.forest_predict(bst, Xd.to_sparse_csr(), kind=kind)


@pytest.mark.parametrize("name", ["table", "offsets", "classes16"])
def test_matrices_narrower_and_wider_than_the_model(name):
    """predict_disable_shape_check: the host predicts a narrower dense matrix (the kernels index a
    row by the model's features) and reads its absent columns as 0; a wider one runs on the device"""
    f, c = fr.FORESTS[name], case_of(name)
    wide = np.concatenate([f.tiled(1024), np.full((1024, 3), 7.0)], axis=1)
    off = {"predict_disable_shape_check": True}
    for dtype in DTYPES:
        for cols in (1, 2, f.num_features - 1):
            X = cast(wide[:, :cols], dtype)
            raw, leaf = fr.walk(f.text, X)
            before = _device_calls()
            got_raw = c.booster.predict(X, raw_score=True, **off, **GPU).reshape(1024, -1)
            got_leaf = c.booster.predict(X, pred_leaf=True, **off, **GPU)
            got_for_mat = _for_mat(c.booster, np.asfortranarray(X), "raw", raw.shape[1], 0, -1,
                                   "device_type=gpu predict_disable_shape_check=true")
            assert _device_calls() == before, "a matrix of %d columns went to the device" % cols
            assert np.array_equal(got_raw, raw) and np.array_equal(got_leaf, leaf) and np.array_equal(got_for_mat, raw)
        X = cast(wide, dtype)
        want = take(name, dtype, 1024)
        before = _device_calls()
        with pytest.raises(lgb.LightGBMError):  # (the host path reports the mismatch)
            c.booster.predict(X, raw_score=True, **GPU)
        assert _device_calls() == before
        check({k: _device(c.booster, X, **kw, **off) for k, kw in KINDS.items()}, want, name,
              "%s %d columns %s" % (name, X.shape[1], np.dtype(dtype).name))
