"""CSC matrices binned on the device when a Dataset is constructed (src/device/csc_bin_kernels.hip).

Kernel against evaluator: ops.csc_group_bins (the kernels under a Dataset's bin mappers) must equal
LGBM_AMD_CscToGroupBins, the shared rule of src/device/csc_bins.h on the host, which
tests/test_csc_bins.py holds to the host path -- on the edge matrix of
tests/helpers/csc_bin_cases.py (with rows outside the matrix and a pointer past the entries) and on
columns placed on the kernels' launch shape (0, 1, S - 1, S, S + 1 and 2S + 1 entries for a segment
of S, a cell stored twice inside a segment and across two, a shuffled column longer than a segment,
more push-zeros features than a wave has lanes, tile - 1 / tile / tile + 1 rows).

Dataset path: a Dataset built with LGBM_AMD_DEVICE_BINNING=1 saves the same binary file, byte for
byte, as one built with =0 and as the device CSR build of m.tocsr(), and LGBM_AMD_DeviceBinCscStats
shows the CSC path ran once per device build, so a silent host fallback fails.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from lightgbmv1_amd import ops
from lightgbmv1_amd._native import LightGBMError
from helpers import csc_bin_cases as cc
from helpers import csr_bin_cases as cb

pytestmark = pytest.mark.gpu

N = 3000
WIDE = 90       # columns of the wide matrix
WIDE_PZ = 70    # its first columns hold 1.0 in 85 % of the rows: their zeros are pushed
WIDE_ROWS = 1400


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    pass


def _csc_tensor(col_ptr, indices, data, num_row):
    ccol = torch.from_numpy(np.ascontiguousarray(col_ptr)).cuda()
    row = torch.from_numpy(np.ascontiguousarray(indices)).to(ccol.dtype).cuda()
    return torch.sparse_csc_tensor(ccol, row, torch.from_numpy(np.ascontiguousarray(data)).cuda(),
                                   size=(num_row, len(col_ptr) - 1), check_invariants=False)


def _kernel_equals_rule(ds, arrays, num_row):
    rule = ds.eval_group_bins(*arrays, num_row)
    got = ops.csc_group_bins(ds, _csc_tensor(*arrays, num_row)).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == rule.shape
    bad = np.argwhere(got != rule)
    assert bad.shape[0] == 0, (bad[:8], got[got != rule][:8], rule[got != rule][:8])
    return rule


@pytest.fixture(scope="module")
def edge():
    clean = cc.columns_of(cb.base_rows(N))
    cols, _ = cc.edge_columns(clean, N)
    return clean, cc.with_bad_rows(cols, N)


@pytest.mark.parametrize("ptype", [np.int32, np.int64], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("vtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("setting", [{}, {"use_missing": False}, {"zero_as_missing": True},
                                     {"categorical_feature": "9,14"}, {"enable_bundle": False}],
                         ids=["default", "no_missing", "zero_as_missing", "categorical", "no_bundle"])
def test_kernel_equals_rule_on_the_edge_matrix(monkeypatch, edge, setting, vtype, ptype):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    clean, cols = edge
    train = cc.NativeCscDataset(*cc.flatten(clean, vtype, ptype), N, dict(cc.PARAMS, **setting))
    arrays = cc.flatten(cols, vtype, ptype)
    rule = _kernel_equals_rule(train, arrays, N)
    assert ((rule == -1).all(axis=0).any()) == ("categorical_feature" in setting)
    assert (rule > 0).any(axis=0).sum() >= 2
    over = arrays[0].copy()
    over[-1] += 7  # (a pointer past the entries)
    assert np.array_equal(_kernel_equals_rule(train, (over, arrays[1], arrays[2]), N), rule)


@pytest.fixture(scope="module")
def wide():
    """the columns of the wide training matrix: WIDE_PZ push-zeros columns, the rest sparse"""
    rng = np.random.RandomState(11)
    cols = []
    for c in range(WIDE):
        if c < WIDE_PZ:
            u = rng.rand(WIDE_ROWS)
            cols.append([(r, 1.0 if u[r] < 0.85 else float(2 + c % 3)) for r in range(WIDE_ROWS) if u[r] < 0.92])
        else:
            cols.append([(int(r), float(rng.randn()) + 2.0) for r in np.flatnonzero(rng.rand(WIDE_ROWS) < 0.05)])
    return cols


def _column(rng, c, length, twice=(), shuffle=False):
    """`length` entries of column c on distinct ascending rows; twice: (i, j) pairs of positions, the
    entry at j repeating the row of the entry at i with another value"""
    rows = np.sort(rng.permutation(WIDE_ROWS)[:length])
    if shuffle:
        rows = rng.permutation(rows)
    col = []
    for r in rows:
        v = rng.choice([1.0, 2.0, 3.0, 0.0]) if c < WIDE_PZ else rng.choice([rng.randn() + 2.0, 0.0, float("nan")])
        col.append((int(r), float(v)))
    for i, j in twice:
        col[j] = (col[i][0], col[i][1] + 1.0 if j % 2 else 0.0 if c >= WIDE_PZ else 1.0)
    return col


@pytest.mark.parametrize("ptype", [np.int32, np.int64], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("vtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_kernel_equals_rule_on_the_launch_shape(monkeypatch, wide, vtype, ptype):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    info = ops.csc_bin_launch_info()
    S, B, tile = info["segment_entries"], info["batch"], info["tile_rows"]
    assert 2 * S + 1 <= WIDE_ROWS and B < WIDE_PZ <= info["max_push_zero_features"] and tile + 1 < WIDE_ROWS
    train = cc.NativeCscDataset(*cc.flatten(wide, vtype, ptype), WIDE_ROWS, cc.PARAMS)
    rng = np.random.RandomState(12)
    cols = [list(c) for c in wide]
    # on push-zeros columns and on sparse ones: the segment's edges
    for c, n in zip((0, 1, 2, 3, 4, 5, 70, 71, 72, 73, 74, 75), (0, 1, S - 1, S, S + 1, 2 * S + 1) * 2):
        cols[c] = _column(rng, c, n)
    for c in (6, 76):
        cols[c] = _column(rng, c, S + 16, twice=[(10, 20), (30, B + 3)])      # twice inside a segment
        cols[c + 1] = _column(rng, c + 1, S + 16, twice=[(11, S + 7)])          # ... across two segments
        cols[c + 2] = _column(rng, c + 2, 2 * S + 1, shuffle=True)              # unsorted, longer than a segment
        cols[c + 3] = _column(rng, c + 3, 2 * S + 1, twice=[(3, 40), (40, S + 3), (S + 3, 2 * S)])  # four times
    arrays = cc.flatten(cols, vtype, ptype)
    rule = _kernel_equals_rule(train, arrays, WIDE_ROWS)
    assert ((rule != 0).sum(axis=1) >= 1).all()  # (column 0 is empty: every row holds its pushed zero bin)
    # the tile's row edge (the entries on later rows are dropped)
    for n in (tile - 1, tile, tile + 1, 1):
        _kernel_equals_rule(train, arrays, n)


# ---- Dataset path

def _matrix(n, seed, dense_cols=(0, 1), ncol=40, density=0.05, dtype=np.float64):
    rng = np.random.RandomState(seed)
    X = np.zeros((n, ncol))
    mask = rng.rand(n, ncol) < density
    X[mask] = rng.randn(int(mask.sum())) + 2.0
    for c in dense_cols:
        X[:, c] = rng.randn(n)
    X[rng.rand(n) < 0.02, 3] = np.nan
    m = sp.csc_matrix(X.astype(dtype))
    y = (X[:, 0] + np.nan_to_num(X[:, 3]) + X[:, 5] > 0.5).astype(np.float32)
    return m, y


def _num_groups(ds):
    ng = ctypes.c_int(0)
    nat.call("LGBM_AMD_DatasetGetGroupBins", ds.construct().handle, None, None, ctypes.byref(ng))
    return ng.value


def _build_all(monkeypatch, tmp_path, make, name="d"):
    """the binary files of make("csc") built on the host and on the device, and of make("csr") (the
    same matrices converted) on the device: all equal; the device builds must take the CSC / CSR
    path once per Dataset"""
    files = []
    for mode, layout in (("0", "csc"), ("1", "csc"), ("1", "csr")):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cc.csc_stats()[0], cb.bin_stats()[1]
        sets = make(layout)
        for k, ds in enumerate(sets):
            ds.construct()
            f = tmp_path / ("%s_%s_%s_%d.bin" % (name, mode, layout, k))
            ds.save_binary(str(f))
            files.append(f.read_bytes())
        assert cc.csc_stats()[0] - before[0] == (len(sets) if (mode, layout) == ("1", "csc") else 0)
        assert cb.bin_stats()[1] - before[1] == (len(sets) if (mode, layout) == ("1", "csr") else 0)
    n = len(files) // 3
    for k in range(n):
        assert len(files[k]) > 100 and files[k] == files[n + k], k
        assert files[k] == files[2 * n + k], k
    return n


def _as(layout, m):
    return m if layout == "csc" else m.tocsr()


PARAMS = {"objective": "binary", "max_bin": 63, "verbose": -1, "device_type": "gpu"}


@pytest.mark.parametrize("host_sparse", [None, "0", "1"])
def test_dataset_files_equal_host_build(monkeypatch, tmp_path, host_sparse):
    if host_sparse is None:
        monkeypatch.delenv("LGBM_AMD_HOST_SPARSE", raising=False)
    else:
        monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", host_sparse)
    m, y = _matrix(30011, 1)
    _build_all(monkeypatch, tmp_path, lambda layout: [lgb.Dataset(_as(layout, m), y, params=PARAMS)])


@pytest.mark.parametrize("case", ["float32_int64", "categorical", "no_bundle", "last_window_one_group",
                                  "unsorted_and_twice"])
def test_dataset_files_equal_host_build_variants(monkeypatch, tmp_path, case):
    m, y = _matrix(4097, 2, dtype=np.float32 if case == "float32_int64" else np.float64)
    params, cat = dict(PARAMS), "auto"
    if case == "float32_int64":
        m.indptr = m.indptr.astype(np.int64)
    if case == "categorical":
        m = sp.csc_matrix(np.hstack([m.toarray(), np.random.RandomState(3).randint(0, 6, size=(m.shape[0], 2))]))
        cat = [40, 41]
    if case == "no_bundle":
        params["enable_bundle"] = False
    if case == "last_window_one_group":
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
        ng = _num_groups(lgb.Dataset(m, y, params=params))
        k = next(k for k in range(2, ng) if ng % k == 1)  # (at least two windows, the last of one group)
        monkeypatch.setenv("LGBM_AMD_BIN_CHUNK_GROUPS", str(k))
    if case == "unsorted_and_twice":
        indptr, indices, data = m.indptr.copy(), m.indices.copy(), m.data.copy()
        s, e = indptr[5], indptr[6]
        order = np.random.RandomState(4).permutation(e - s)
        indices[s:e], data[s:e] = indices[s:e][order], data[s:e][order]
        at = indptr[8]  # column 7's last cell again, with another value
        indices, data = np.insert(indices, at, indices[at - 1]), np.insert(data, at, data[at - 1] + 1.5)
        indptr[8:] += 1
        m = sp.csc_matrix((data, indices, indptr), shape=m.shape)
        assert not m.has_sorted_indices
    _build_all(monkeypatch, tmp_path, lambda layout: [lgb.Dataset(_as(layout, m), y, params=params, categorical_feature=cat)])


@pytest.mark.parametrize("width", [38, 40, 43], ids=["narrower", "equal", "wider"])
def test_reference_sets_of_other_widths(monkeypatch, tmp_path, width):
    m, y = _matrix(5000, 4)
    v, vy = _matrix(2000, 7, ncol=width)

    def make(layout):
        tr = lgb.Dataset(_as(layout, m), y, params=PARAMS)
        return [tr, lgb.Dataset(_as(layout, v), vy, reference=tr)]
    assert _build_all(monkeypatch, tmp_path, make) == 2


def test_tile_edges_and_empty_sparse_group(monkeypatch, tmp_path):
    """a validation set whose sparse column 7 is stored at rows 255 and 256 of the compaction tiles
    only, and whose sparse column 8 has no stored row"""
    tile = ops.csc_bin_launch_info()["tile_rows"]
    monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", "1")
    m, y = _matrix(5000, 4)
    v = m[:3 * tile + 5].toarray()
    v[:, 7] = 0.0
    v[:, 8] = 0.0
    for r in (tile - 1, tile, 2 * tile - 1, 2 * tile, 3 * tile + 4):
        v[r, 7] = 2.5
    vm = sp.csc_matrix(v)

    def make(layout):
        tr = lgb.Dataset(_as(layout, m), y, params=PARAMS)
        return [tr, lgb.Dataset(_as(layout, vm), y[:vm.shape[0]], reference=tr)]
    assert _build_all(monkeypatch, tmp_path, make) == 2


def test_validation_set_trains_the_same_model(monkeypatch):
    m, y = _matrix(20000, 5)
    vm, vy = _matrix(6000, 6)
    texts = []
    for mode in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cc.csc_stats()[0]
        tr = lgb.Dataset(m, y, params=PARAMS)
        va = lgb.Dataset(vm, vy, reference=tr)
        evals = {}
        bst = lgb.train(dict(PARAMS, num_leaves=15, metric="binary_logloss"), tr, num_boost_round=3, valid_sets=[va],
                        callbacks=[lgb.record_evaluation(evals)])
        assert cc.csc_stats()[0] - before == (2 if mode == "1" else 0)
        texts.append((bst.model_to_string(), evals))
    assert texts[0][0] == texts[1][0] and texts[0][1] == texts[1][1]
    assert texts[0][0].count("Tree=") == 3


def test_gate_without_the_knob(monkeypatch):
    """LGBM_AMD_DEVICE_BINNING unset: device_type=gpu and enough stored entries take the device"""
    monkeypatch.delenv("LGBM_AMD_DEVICE_BINNING", raising=False)
    rng = np.random.RandomState(8)
    n, per_row = 12000, 10   # 120K stored entries: the gate (kCscBinMinEntries)
    big = sp.csr_matrix((rng.randn(n * per_row), (rng.randint(0, 4, size=(n, per_row)) + 4 * np.arange(per_row)).ravel(),
                         np.arange(n + 1) * per_row), shape=(n, 40)).tocsc()
    assert big.nnz == 120000
    small = big[:n - 1]  # (one row, ten entries, below it)
    for m, params, expect in ((big, PARAMS, 1), (big, dict(PARAMS, device_type="cpu"), 0), (small, PARAMS, 0)):
        before = cc.csc_stats()[0]
        lgb.Dataset(m, params=params).construct()
        assert cc.csc_stats()[0] - before == expect


def test_too_many_push_zero_features_stay_on_the_host(monkeypatch, tmp_path):
    """one feature more than the cap: the whole matrix takes the host path, and the op refuses
    instead of running the kernels"""
    cap = ops.csc_bin_launch_info()["max_push_zero_features"]
    rng = np.random.RandomState(13)
    m = sp.csc_matrix((rng.rand(300, cap + 1) < 0.85).astype(np.float32))  # 1.0 is every column's most frequent value
    y = rng.rand(300).astype(np.float32)
    files = []
    for mode in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cc.csc_stats()[0]
        ds = lgb.Dataset(m, y, params=PARAMS).construct()
        assert cc.csc_stats()[0] == before
        f = tmp_path / ("pz_%s.bin" % mode)
        ds.save_binary(str(f))
        files.append(f.read_bytes())
    assert files[0] == files[1]
    with pytest.raises(LightGBMError, match="zeros pushed"):
        ops.csc_group_bins(ds, _csc_tensor(m.indptr[:5], m.indices[:m.indptr[4]], m.data[:m.indptr[4]], 300))


def test_malformed_col_ptr_never_reaches_the_device(monkeypatch):
    """a col_ptr that descends is refused before any upload: the matrix goes to the host path and
    builds what it builds with device binning off"""
    cols = cc.columns_of(cb.base_rows(600))
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    train = cc.NativeCscDataset(*cc.flatten(cols), 600, cc.PARAMS)
    col_ptr, indices, data = cc.flatten(cols)
    col_ptr = col_ptr.copy()
    col_ptr[12] = col_ptr[13] + 2
    outcomes = []
    for mode in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cc.csc_stats()[0]
        try:
            outcomes.append(cc.NativeCscDataset(col_ptr, indices, data, 600, cc.PARAMS, reference=train).group_bins()[0])
        except LightGBMError as e:
            outcomes.append(str(e))
        assert cc.csc_stats()[0] == before
    assert type(outcomes[0]) is type(outcomes[1]) and np.array_equal(outcomes[0], outcomes[1])
    # (and the well-formed matrix does go through the device with the same reference)
    before = cc.csc_stats()[0]
    valid = cc.NativeCscDataset(*cc.flatten(cols), 600, cc.PARAMS, reference=train)
    assert cc.csc_stats()[0] == before + 1
    assert np.array_equal(valid.group_bins()[0], train.group_bins()[0])
