"""CSC inputs predicted on the device (src/device/csc_kernels.hip scatters the stored entries of
the columns the trees split on into the compact matrix; the forest kernels walk it) against the
host predictor (LGBM_AMD_HOST_PREDICT=1), the device CSR path on m.tocsr() and the dense device
path: through Booster.predict / LGBM_BoosterPredictForCSC / LGBM_BoosterPredictSparseOutput (row
gate, row chunks, shape check) and through lightgbmv1_amd.ops.forest_predict on torch.sparse_csc
GPU tensors.  Raw scores and leaf indices must be equal; contributions are held to the tolerance
of tests/helpers/contrib_cases.py and are bit-equal to the device CSR path's (same compact matrix,
same kernel); in forced chunks the four host layouts (row-major, column-major, CSR, CSC) give the
same doubles for every kind.  What a matrix with repeated cells means comes from csc_meaning
(tests/helpers/csc_cases.py), never from toarray(), which sums them.
LGBM_AMD_DevicePredictCount is asserted on every call, so a silent host fallback fails.
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
from helpers import csc_cases as csc
from helpers import forest_ref as fr

pytestmark = pytest.mark.gpu

GPU = {"device_type": "gpu"}
KINDS = ({"raw_score": True}, {"pred_leaf": True}, {"pred_contrib": True})
OPS_KINDS = ("raw", "leaf", "contrib")


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    pass


def _device_calls():
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DevicePredictCount", ctypes.byref(out))
    return out.value


def _dense(pred):
    """contributions of a sparse input come back sparse (a list of matrices for several classes)"""
    if isinstance(pred, list):
        return np.hstack([p.toarray() for p in pred])
    return pred.toarray() if sp.issparse(pred) else pred


def _host(monkeypatch, booster, X, **kw):
    monkeypatch.setenv("LGBM_AMD_HOST_PREDICT", "1")
    before = _device_calls()
    out = _dense(booster.predict(X, **kw, **GPU))
    assert _device_calls() == before
    monkeypatch.delenv("LGBM_AMD_HOST_PREDICT")
    return out


def _device(booster, X, **kw):
    before = _device_calls()
    out = _dense(booster.predict(X, **kw, **GPU))
    assert _device_calls() == before + 1, "the prediction did not run on the device"
    return out


def _capi(booster, m, kind=nat.PREDICT_CONTRIB, start_iteration=0, num_iteration=-1, ptr_dtype=None,
          params="device_type=gpu"):
    """doubles from LGBM_BoosterPredictForCSC / ForCSR by the matrix's format (Booster.predict gives the
    contributions of a sparse input in the input's type: float32 for a float32 matrix)"""
    indptr = m.indptr if ptr_dtype is None else m.indptr.astype(ptr_dtype)
    p_ptr, p_code = nat.pointer(indptr)
    v_ptr, v_code = nat.pointer(m.data)
    is_csc = sp.isspmatrix_csc(m)
    width = ctypes.c_int64(0)
    nat.call("LGBM_BoosterCalcNumPredict", booster.handle, nat.c_int(1), nat.c_int(kind), nat.c_int(start_iteration),
             nat.c_int(num_iteration), ctypes.byref(width))
    out = np.empty((m.shape[0], width.value))
    got = ctypes.c_int64(0)
    nat.call("LGBM_BoosterPredictForCSC" if is_csc else "LGBM_BoosterPredictForCSR", booster.handle, p_ptr,
             ctypes.c_int32(p_code), m.indices.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v_ptr, nat.c_int(v_code),
             ctypes.c_int64(len(indptr)), ctypes.c_int64(len(m.data)), ctypes.c_int64(m.shape[0 if is_csc else 1]),
             nat.c_int(kind), nat.c_int(start_iteration), nat.c_int(num_iteration), nat.cstr(params), ctypes.byref(got),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert got.value == out.size
    return out


def _compare_with_host(monkeypatch, booster, m, case_, what, **window):
    """device CSC against host CSC for the three kinds; returns the device's (raw, leaf, contrib).
    The contributions are compared as the doubles of LGBM_BoosterPredictForCSC; the sparse output
    of Booster.predict must be csc matrices holding the same values in the matrix's type."""
    assert sp.isspmatrix_csc(m) and m.indices.dtype == np.int32
    raw_d = _device(booster, m, raw_score=True, **window)
    leaf_d = _device(booster, m, pred_leaf=True, **window)
    before = _device_calls()
    contrib_d = _capi(booster, m, **window)
    assert _device_calls() == before + 1, "the contributions did not come from the device"
    raw_h = _host(monkeypatch, booster, m, raw_score=True, **window)
    leaf_h = _host(monkeypatch, booster, m, pred_leaf=True, **window)
    monkeypatch.setenv("LGBM_AMD_HOST_PREDICT", "1")
    contrib_h = _capi(booster, m, **window)
    assert _device_calls() == before + 1
    monkeypatch.delenv("LGBM_AMD_HOST_PREDICT")
    assert raw_d.shape == raw_h.shape and np.array_equal(raw_d, raw_h), what
    assert leaf_d.shape == leaf_h.shape and np.array_equal(leaf_d, leaf_h), what
    cc.check_contrib(contrib_d, contrib_h, raw_d, case_, what)
    before = _device_calls()
    sparse_out = booster.predict(m, pred_contrib=True, **window, **GPU)
    assert _device_calls() == before + 1, "the sparse contributions did not come from the device"
    parts = sparse_out if isinstance(sparse_out, list) else [sparse_out]
    assert len(parts) == (case_.num_class if case_.num_class > 1 else 1)
    assert all(sp.isspmatrix_csc(p) and p.dtype == m.dtype for p in parts), what
    assert np.array_equal(_dense(sparse_out), contrib_d.astype(m.dtype)), what
    return raw_d, leaf_d, contrib_d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", cc.CASES)
def test_model_cases_match_the_host_the_csr_path_and_the_dense_path(name, dtype, monkeypatch):
    c = cc.case(name)
    X = np.ascontiguousarray(c.X.astype(dtype))
    m = sp.csc_matrix(X)  # (drops the zeros, keeps the NaN)
    assert m.dtype == dtype and m.has_sorted_indices
    raw_d, leaf_d, contrib_d = _compare_with_host(monkeypatch, c.booster, m, c,
                                                  "%s %s" % (name, np.dtype(dtype).name), **c.window)
    r = m.tocsr()
    assert np.array_equal(raw_d, _device(c.booster, r, raw_score=True, **c.window))
    assert np.array_equal(leaf_d, _device(c.booster, r, pred_leaf=True, **c.window))
    assert np.array_equal(raw_d, _device(c.booster, X, raw_score=True, **c.window))
    assert np.array_equal(leaf_d, _device(c.booster, X, pred_leaf=True, **c.window))
    before = _device_calls()
    assert np.array_equal(contrib_d, _capi(c.booster, r, **c.window)), "contributions differ from the CSR path's"
    assert _device_calls() == before + 1


@pytest.fixture(scope="module")
def wide():
    (col_ptr, indices, data), dense = csc.wide_matrix()
    inf = csc.WIDE_INFORMATIVE
    y = dense[:, inf] @ np.linspace(1.0, 2.0, len(inf)) + np.sin(3 * dense[:, 7])
    p = {"objective": "regression", "num_leaves": 15, "min_data_in_leaf": 5, "verbose": -1, "num_threads": 4, "seed": 2}
    bst = lgb.train(p, lgb.Dataset(dense, y, params=p), num_boost_round=10)
    m = sp.csc_matrix((data, indices, col_ptr), shape=dense.shape)
    return bst, m, dense


def test_wide_sparse_matrix(wide, monkeypatch):
    bst, m, dense = wide
    counts = np.diff(m.indptr)
    assert counts[:6].tolist() == csc.WIDE_COUNTS and (m.data == 0.0).any()
    assert 0.005 < m.nnz / (csc.WIDE_ROWS * csc.WIDE_COLS) < 0.015
    used = np.nonzero(bst.feature_importance())[0]
    assert 3 <= len(used) <= len(csc.WIDE_INFORMATIVE) + 5
    inf = csc.WIDE_INFORMATIVE

    def column(c):
        return m.indices[m.indptr[c]:m.indptr[c + 1]]

    # what the matrix holds: a shuffled column, a cell three times over more than 64 entries, repeats
    # inside the batch of entries 64 .. 127; all of them columns the trees split on
    assert set(inf[:4]) <= set(used.tolist())
    assert (np.diff(column(inf[0])) < 0).any() and (np.diff(column(inf[3])) < 0).any()
    three = column(inf[1])
    assert three[3] == three[200] == three[500] and np.count_nonzero(three == three[3]) == 3
    batch = column(inf[2])[64:128]
    assert len(set(batch.tolist())) <= 64 - 4
    assert not np.array_equal(m.toarray(), dense), "toarray() sums the repeated cells"
    c = cc.Case(bst, dense)
    raw_d, leaf_d, contrib_d = _compare_with_host(monkeypatch, bst, m, c, "wide")
    # the repeated cells hold their last stored entry: the dense matrix built that way agrees
    assert np.array_equal(raw_d, _device(bst, dense, raw_score=True))
    assert np.array_equal(leaf_d, _device(bst, dense, pred_leaf=True))
    cc.check_contrib(contrib_d, _device(bst, dense, pred_contrib=True), raw_d, c, "wide against dense")
    unused = np.setdiff1d(np.arange(csc.WIDE_COLS), used)
    assert np.all(contrib_d[:, unused] == 0.0)
    # a second run is the first one, bit for bit
    assert np.array_equal(raw_d, _device(bst, m, raw_score=True))
    assert np.array_equal(leaf_d, _device(bst, m, pred_leaf=True))
    before = _device_calls()
    assert np.array_equal(contrib_d, _capi(bst, m))
    assert _device_calls() == before + 1


def test_wide_sparse_matrix_in_chunks(wide, monkeypatch):
    """chunks of 192 rows: every column's entries spread over all of them, and the compact
    matrix's column stride changes with the last chunk"""
    bst, m, dense = wide
    want = {k: _device(bst, m, **{k: True}) for k in ("raw_score", "pred_leaf", "pred_contrib")}
    leaf_h = _host(monkeypatch, bst, m, pred_leaf=True)
    monkeypatch.setenv("LGBM_AMD_PREDICT_CHUNK_ROWS", "192")
    for k, w in want.items():
        assert np.array_equal(_device(bst, m, **{k: True}), w), k
    assert np.array_equal(want["pred_leaf"], leaf_h)
    assert np.array_equal(want["pred_leaf"], _device(bst, dense, pred_leaf=True))


def _three_chunks():
    c = cc.case("multiclass3")
    X = np.concatenate([c.X, c.X[::-1]])  # 3000 rows: two chunks of 1024 and one of 952
    X[[1023, 1024, 2047, 2999]] = 0.0     # all-zero rows on the chunk boundaries
    return c, X


def _for_mat(booster, X, kind):
    """doubles from LGBM_BoosterPredictForMat on X in the layout it has (row- or column-major)"""
    row_major = X.flags["C_CONTIGUOUS"]
    assert X.dtype == np.float64 and (row_major or X.flags["F_CONTIGUOUS"])
    width = ctypes.c_int64(0)
    nat.call("LGBM_BoosterCalcNumPredict", booster.handle, nat.c_int(1), nat.c_int(kind), nat.c_int(0), nat.c_int(-1),
             ctypes.byref(width))
    out = np.empty((X.shape[0], width.value))
    got = ctypes.c_int64(0)
    nat.call("LGBM_BoosterPredictForMat", booster.handle, X.ctypes.data_as(ctypes.c_void_p), nat.c_int(nat.DTYPE_FLOAT64),
             ctypes.c_int32(X.shape[0]), ctypes.c_int32(X.shape[1]), nat.c_int(1 if row_major else 0), nat.c_int(kind),
             nat.c_int(0), nat.c_int(-1), nat.cstr("device_type=gpu"), ctypes.byref(got),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert got.value == out.size
    return out


@pytest.mark.parametrize("kind", [nat.PREDICT_RAW_SCORE, nat.PREDICT_NORMAL, nat.PREDICT_LEAF_INDEX, nat.PREDICT_CONTRIB],
                         ids=["raw", "normal", "leaf", "contrib"])
def test_the_four_layouts_agree_in_chunks(kind, monkeypatch):
    """one loop stages, runs and copies back the chunks of every layout: 3000 rows in chunks of
    1024 give the same doubles as row-major, column-major, CSR and CSC input, one device call each,
    and (but for contributions, which the host computes by another algorithm) the host's"""
    c, X = _three_chunks()
    m = sp.csc_matrix(X)
    monkeypatch.setenv("LGBM_AMD_PREDICT_CHUNK_ROWS", "1024")
    got = {}
    for layout, predict in [("row-major", lambda: _for_mat(c.booster, X, kind)),
                            ("column-major", lambda: _for_mat(c.booster, np.asfortranarray(X), kind)),
                            ("csr", lambda: _capi(c.booster, m.tocsr(), kind)),
                            ("csc", lambda: _capi(c.booster, m, kind))]:
        before = _device_calls()
        got[layout] = predict()
        assert _device_calls() == before + 1, "%s did not take one device call" % layout
    for layout, out in got.items():
        assert out.shape == got["row-major"].shape and np.array_equal(out, got["row-major"]), layout
    if kind != nat.PREDICT_CONTRIB:
        monkeypatch.setenv("LGBM_AMD_HOST_PREDICT", "1")
        before = _device_calls()
        host = _for_mat(c.booster, X, kind)
        assert _device_calls() == before
        assert np.array_equal(got["row-major"], host)


def test_chunked_rows_are_bit_equal(monkeypatch):
    c, X = _three_chunks()
    m = sp.csc_matrix(X)
    assert not np.isin(m.indices, [1023, 1024, 2047, 2999]).any()
    for kw in KINDS:
        whole = _device(c.booster, m, **kw)
        monkeypatch.setenv("LGBM_AMD_PREDICT_CHUNK_ROWS", "1024")
        chunked = _device(c.booster, m, **kw)
        monkeypatch.delenv("LGBM_AMD_PREDICT_CHUNK_ROWS")
        assert whole.shape[0] == 3000 and np.array_equal(whole, chunked)
    monkeypatch.setenv("LGBM_AMD_PREDICT_CHUNK_ROWS", "1024")
    assert np.array_equal(_device(c.booster, m, pred_leaf=True), _host(monkeypatch, c.booster, m, pred_leaf=True))


def test_c_api_with_int64_col_ptr(wide):
    bst, m, _ = wide
    want = _device(bst, m, raw_score=True)
    before = _device_calls()
    out = _capi(bst, m, kind=nat.PREDICT_RAW_SCORE, ptr_dtype=np.int64)
    assert _device_calls() == before + 1
    assert np.array_equal(out.reshape(-1), want)


def test_row_gate_and_early_stop(monkeypatch):
    c = cc.case("window")
    m = sp.csc_matrix(c.X)
    for kw in KINDS:
        before = _device_calls()
        below = _dense(c.booster.predict(m[:1023], **kw, **GPU))
        assert _device_calls() == before, "1023 rows stay on the host"
        at = _device(c.booster, m[:1024], **kw)
        want = _host(monkeypatch, c.booster, m[:1024], **kw)
        assert np.array_equal(below, want[:1023])
        if "pred_contrib" in kw:
            cc.check_contrib(at, want, _device(c.booster, m[:1024], raw_score=True), cc.Case(c.booster, c.X), "1024 rows")
        else:
            assert np.array_equal(at, want)
    before = _device_calls()
    stopped = c.booster.predict(m, pred_early_stop=True, **GPU)
    assert _device_calls() == before, "early stopping stays on the host"
    assert stopped.shape == (len(c.X),)


def test_matrix_without_stored_entries(monkeypatch):
    c = cc.case("repeat3")
    m = sp.csc_matrix((1200, c.num_features))
    assert m.nnz == 0
    zero_row = np.zeros((1, c.num_features))
    for kw in KINDS:
        got = _device(c.booster, m, **kw)
        one = _host(monkeypatch, c.booster, zero_row, **kw).reshape(1, -1)
        got = got.reshape(1200, -1)
        if "pred_contrib" in kw:
            assert np.max(np.abs(got - one)) <= cc.tolerance(c.booster)
            assert np.array_equal(got, np.repeat(got[:1], 1200, axis=0))
        else:
            assert np.array_equal(got, np.repeat(one, 1200, axis=0))


def test_shape_check(wide, monkeypatch):
    bst, m, _ = wide
    grown = sp.csc_matrix((m.data, m.indices, np.concatenate([m.indptr, [m.indptr[-1]] * 3])),
                          shape=(csc.WIDE_ROWS, csc.WIDE_COLS + 3))
    for cols in (csc.WIDE_COLS - 3, csc.WIDE_COLS + 3):
        other = grown[:, :cols]
        assert other.shape[1] == cols and sp.isspmatrix_csc(other)
        before = _device_calls()
        with pytest.raises(lgb.LightGBMError):  # (the host path reports the mismatch)
            bst.predict(other, raw_score=True, **GPU)
        assert _device_calls() == before
        for kw in ({"raw_score": True}, {"pred_leaf": True}):
            got = _device(bst, other, predict_disable_shape_check=True, **kw)
            want = _host(monkeypatch, bst, other, predict_disable_shape_check=True, **kw)
            assert np.array_equal(got, want)


def _csc_tensor(col_ptr, indices, data, shape, index_dtype):
    return torch.sparse_csc_tensor(torch.as_tensor(np.asarray(col_ptr)).to(index_dtype),
                                   torch.as_tensor(np.asarray(indices)).to(index_dtype), torch.as_tensor(np.asarray(data)),
                                   size=shape, device="cuda", check_invariants=False)


@pytest.mark.filterwarnings("ignore:Sparse C:UserWarning")
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_ops_forest_predict_on_sparse_csc_tensors(index_dtype):
    c = cc.case("multiclass3")
    rows = 70  # (below the C API's row gate: the op has none)
    for dtype in (torch.float32, torch.float64):
        Xd = torch.tensor(c.X[:rows], dtype=dtype, device="cuda")
        Xd[3] = 0.0  # an empty row
        m = sp.csc_matrix(Xd.cpu().numpy())
        Xs = _csc_tensor(m.indptr, m.indices, m.data, m.shape, index_dtype)
        assert Xs.layout == torch.sparse_csc and Xs.ccol_indices().dtype == index_dtype
        assert Xs.row_indices().dtype == index_dtype and Xs.values().dtype == dtype
        for kind in OPS_KINDS:
            before = _device_calls()
            got = ops.forest_predict(c.booster, Xs, kind=kind)
            want = ops.forest_predict(c.booster, Xd, kind=kind)
            assert _device_calls() == before + 2
            assert got.is_cuda and got.dtype == torch.float64 and got.shape == want.shape
            if kind == "contrib":
                raw = ops.forest_predict(c.booster, Xs, kind="raw").cpu().numpy()
                cc.check_contrib(got.cpu().numpy(), want.cpu().numpy(), raw, c, "ops %s %s" % (index_dtype, dtype))
            else:
                assert torch.equal(got, want)
    win = ops.forest_predict(c.booster, Xs, kind="leaf", start_iteration=2, num_iteration=3)
    assert tuple(win.shape) == (rows, 9)
    with pytest.raises(lgb.LightGBMError):
        ops.forest_predict(c.booster, Xs, kind="normal")
    # (what to_sparse_csc() builds is taken as well)
    assert torch.equal(ops.forest_predict(c.booster, Xd.to_sparse_csc(), kind="leaf"),
                       ops.forest_predict(c.booster, Xd, kind="leaf"))


@pytest.mark.filterwarnings("ignore:Sparse C:UserWarning")
def test_columns_on_the_segment_boundaries():
    """strictly ascending columns of epw - 1, epw, epw + 1 and 2 * epw + 1 stored entries, epw the
    entries of a column that one wave takes: one segment short of full, exactly full, one entry
    into a second, and one entry into a third"""
    info = ops.csc_launch_info()
    epw = info["segment_entries"]
    assert epw >= info["batch"] >= 1 and info["block"] % info["batch"] == 0
    c = cc.case("multiclass3")
    used = np.nonzero(c.booster.feature_importance())[0]
    lengths = [epw - 1, epw, epw + 1, 2 * epw + 1]
    assert len(used) >= len(lengths)
    rows = 2 * epw + 2
    rng = np.random.RandomState(4)
    dense = np.zeros((rows, c.num_features))
    for f, n in zip(used, lengths):
        at = np.sort(rng.choice(rows, size=n, replace=False))
        dense[at, f] = rng.randn(n) + 3.0  # (no zeros among the stored values)
    m = sp.csc_matrix(dense)
    assert np.diff(m.indptr)[used[:4]].tolist() == lengths and m.has_canonical_format
    Xs = _csc_tensor(m.indptr, m.indices, m.data, m.shape, torch.int64)
    Xd = torch.tensor(dense, device="cuda")
    assert Xs.values().dtype == torch.float64 and tuple(Xs.shape) == (rows, c.num_features)
    for kind in OPS_KINDS:
        before = _device_calls()
        got = ops.forest_predict(c.booster, Xs, kind=kind)
        want = ops.forest_predict(c.booster, Xd, kind=kind)
        assert _device_calls() == before + 2
        print("segments %s: max |diff| = %.3e" % (kind, float((got - want).abs().max())))
        assert torch.equal(got, want), kind


@functools.lru_cache(maxsize=None)
def _forest_case(name):
    f = fr.FORESTS[name]
    return cc.Case(lgb.Booster(model_str=f.text), f.rows, f.start, f.num)


def _cast(X, dtype):
    with np.errstate(over="ignore"):  # (1e300 becomes inf as float32, on purpose)
        return X.astype(dtype)


def _check_forest(got, want, name, what):
    for k in ("raw", "leaf"):
        assert got[k].shape == want[k].shape, (what, k)
        bad = np.nonzero((got[k] != want[k]).any(axis=1))[0]
        assert bad.size == 0, "%s: %s of rows %s differ from the walker" % (what, k, bad[:8])
    cc.check_contrib(got["contrib"], want["contrib"], want["raw"], _forest_case(name), what)


@pytest.mark.filterwarnings("ignore:Sparse C:UserWarning")
@pytest.mark.parametrize("name", fr.DEVICE_FORESTS)
def test_hand_written_forests_through_ops(name):
    f, c = fr.FORESTS[name], _forest_case(name)
    for dtype, index_dtype in ((np.float32, torch.int64), (np.float64, torch.int32)):
        (col_ptr, indices, data, cols), X = csc.mixed_csc(_cast(f.tiled(257), dtype))
        Xs = _csc_tensor(col_ptr, indices, data, (257, cols), index_dtype)
        assert Xs.values().dtype == torch.as_tensor(data).dtype and X.dtype == dtype
        raw, leaf = fr.walk(f.text, X, f.start, f.num)
        contrib = c.booster.predict(X, pred_contrib=True, **c.window).reshape(257, -1)  # (the host predictor)
        before = _device_calls()
        got = {k: ops.forest_predict(c.booster, Xs, kind=k, start_iteration=f.start, num_iteration=f.num).cpu().numpy()
               for k in OPS_KINDS}
        assert _device_calls() == before + 3
        _check_forest(got, {"raw": raw, "leaf": leaf, "contrib": contrib}, name,
                      "ops csc %s %s" % (name, np.dtype(dtype).name))


@pytest.mark.parametrize("name", fr.DEVICE_FORESTS)
def test_hand_written_forests_through_booster_predict(name):
    f, c = fr.FORESTS[name], _forest_case(name)
    for dtype in (np.float32, np.float64):
        (col_ptr, indices, data, cols), X = csc.mixed_csc(_cast(f.tiled(1024), dtype))
        m = sp.csc_matrix((data, indices, col_ptr), shape=(1024, cols))
        assert m.dtype == dtype and m.nnz == len(data)
        raw, leaf = fr.walk(f.text, X, f.start, f.num)
        contrib = c.booster.predict(X, pred_contrib=True, **c.window).reshape(1024, -1)  # (the host predictor)
        kw = dict(c.window, predict_disable_shape_check=True)  # (one column more than the model has)
        got = {"raw": _device(c.booster, m, raw_score=True, **kw).reshape(1024, -1),
               "leaf": _device(c.booster, m, pred_leaf=True, **kw).reshape(1024, -1)}
        before = _device_calls()
        got["contrib"] = _capi(c.booster, m, start_iteration=f.start, num_iteration=f.num,
                               params="device_type=gpu predict_disable_shape_check=true")
        assert _device_calls() == before + 1
        _check_forest(got, {"raw": raw, "leaf": leaf, "contrib": contrib}, name,
                      "%s csc %s" % (name, np.dtype(dtype).name))
