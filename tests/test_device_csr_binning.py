"""CSR matrices binned on the device when a Dataset is constructed (src/device/csr_bin_kernels.hip).

Kernel against evaluator: ops.csr_group_bins (k_csr_to_group_bins under a Dataset's bin mappers)
must equal LGBM_AMD_CsrToGroupBins, the shared rule of src/device/csr_bins.h on the host, which
tests/test_csr_bins.py holds to the host push -- on the edge rows of tests/helpers/csr_bin_cases.py
and on rows placed on the kernel's launch shape (rows of 0, 1, 63, 64, 65 and 129 entries, one
column twice across and inside a batch, 3 / 4 / 5 rows, more push-zeros features than a batch).

Dataset path: a Dataset built with LGBM_AMD_DEVICE_BINNING=1 saves the same binary file, byte for
byte, as one built with =0, and LGBM_AMD_DeviceBinStats shows the CSR path ran once per device
build, so a silent host fallback fails.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import lightgbmv1_amd as lgb
from lightgbmv1_amd import ops
from lightgbmv1_amd._native import LightGBMError
from helpers import csr_bin_cases as cb

pytestmark = pytest.mark.gpu

WIDE = 200      # columns of the wide matrix
WIDE_PZ = 70    # its first columns hold 1.0 in 85 % of the rows: more push-zeros features than a batch


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    pass


def _csr_tensor(indptr, indices, data, ncol):
    crow = torch.from_numpy(np.ascontiguousarray(indptr)).cuda()
    col = torch.from_numpy(np.ascontiguousarray(indices)).to(crow.dtype).cuda()
    return torch.sparse_csr_tensor(crow, col, torch.from_numpy(np.ascontiguousarray(data)).cuda(),
                                   size=(len(indptr) - 1, ncol), check_invariants=False)


def _kernel_equals_rule(ds, arrays, ncol):
    rule = ds.eval_group_bins(*arrays)
    got = ops.csr_group_bins(ds, _csr_tensor(*arrays, ncol)).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == rule.shape
    bad = np.argwhere(got != rule)
    assert bad.shape[0] == 0, (bad[:8], got[got != rule][:8], rule[got != rule][:8])
    return rule


@pytest.fixture(scope="module")
def edge():
    clean = cb.base_rows()
    rows, at = cb.edge_rows(clean)
    rows[at["column_past_end"]].append((-1, 2.0))  # (dropped by the rule; the host push is not asked)
    return clean, rows


@pytest.mark.parametrize("ptype", [np.int32, np.int64], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("vtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("setting", [{}, {"use_missing": False}, {"zero_as_missing": True},
                                     {"categorical_feature": "9,14"}, {"enable_bundle": False}],
                         ids=["default", "no_missing", "zero_as_missing", "categorical", "no_bundle"])
def test_kernel_equals_rule_on_edge_rows(monkeypatch, edge, setting, vtype, ptype):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    clean, rows = edge
    train = cb.NativeDataset(*cb.flatten(clean, vtype, ptype), cb.NCOL, dict(cb.PARAMS, **setting))
    rule = _kernel_equals_rule(train, cb.flatten(rows, vtype, ptype), 1000001)
    assert ((rule == -1).all(axis=0).any()) == ("categorical_feature" in setting)
    assert (rule > 0).any(axis=0).sum() >= 2


@pytest.fixture(scope="module")
def wide():
    """the rows of the wide training matrix: WIDE_PZ push-zeros columns, the rest sparse"""
    rng = np.random.RandomState(11)
    n = 1500
    rows = []
    for r in range(n):
        u = rng.rand(WIDE_PZ)
        row = [(c, 1.0 if u[c] < 0.85 else float(2 + c % 3)) for c in range(WIDE_PZ) if u[c] < 0.92]
        row += [(int(c), float(rng.randn()) + 2.0) for c in np.flatnonzero(rng.rand(WIDE - WIDE_PZ) < 0.05) + WIDE_PZ]
        rows.append(row)
    return rows


def _wide_row(rng, length, twice=()):
    """a row of `length` entries on distinct columns in random order; twice: (i, j) pairs of
    positions, the entry at j repeating the column of the entry at i with another value"""
    cols = rng.permutation(WIDE)[:length]
    row = []
    for c in cols:
        v = rng.choice([1.0, 2.0, 3.0, 0.0]) if c < WIDE_PZ else rng.choice([rng.randn() + 2.0, 0.0, float("nan")])
        row.append((int(c), float(v)))
    for i, j in twice:
        row[j] = (row[i][0], row[i][1] + 1.0 if j % 2 else 0.0 if row[i][0] >= WIDE_PZ else 1.0)
    return row


@pytest.mark.parametrize("ptype", [np.int32, np.int64], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("vtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_kernel_equals_rule_on_the_launch_shape(monkeypatch, wide, vtype, ptype):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    info = ops.csr_bin_launch_info()
    B, W = info["batch"], info["rows_per_block"]
    assert 2 * B + 1 <= WIDE and WIDE_PZ > B and WIDE_PZ <= info["max_push_zero_features"]
    train = cb.NativeDataset(*cb.flatten(wide, vtype, ptype), WIDE, cb.PARAMS)
    rng = np.random.RandomState(12)
    rows = [_wide_row(rng, n) for n in (0, 1, B - 1, B, B + 1, 2 * B + 1)]
    rows.append(_wide_row(rng, B + 16, twice=[(10, B + 6)]))            # one column across two batches
    rows.append(_wide_row(rng, B + 16, twice=[(11, B + 7)]))
    rows.append(_wide_row(rng, B, twice=[(5, 20), (6, 21), (30, 63)]))  # ... twice inside one batch
    rows.append(_wide_row(rng, 2 * B + 1, twice=[(3, 40), (40, B + 3), (B + 3, 2 * B)]))  # ... four times
    rows += [_wide_row(rng, int(n)) for n in rng.randint(0, WIDE, size=40)]
    rows += wide[:64]
    rule = _kernel_equals_rule(train, cb.flatten(rows, vtype, ptype), WIDE)
    assert (rule[0] != 0).sum() >= B  # (the empty row: every push-zeros group holds its zero bin)
    for n in (W - 1, W, W + 1, 1):    # the workgroup's row edge
        _kernel_equals_rule(train, cb.flatten(rows[6:6 + n], vtype, ptype), WIDE)


# ---- Dataset path

def _matrix(n, seed, dense_cols=(0, 1), ncol=40, density=0.05, dtype=np.float64):
    rng = np.random.RandomState(seed)
    X = np.zeros((n, ncol))
    mask = rng.rand(n, ncol) < density
    X[mask] = rng.randn(int(mask.sum())) + 2.0
    for c in dense_cols:
        X[:, c] = rng.randn(n)
    X[rng.rand(n) < 0.02, 3] = np.nan
    m = sp.csr_matrix(X.astype(dtype))
    y = (X[:, 0] + np.nan_to_num(X[:, 3]) + X[:, 5] > 0.5).astype(np.float32)
    return m, y


def _build_both(monkeypatch, tmp_path, make, name="d"):
    """the binary files of make() built on the host and on the device; the device build must
    take the CSR path once per Dataset"""
    files = []
    for mode in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cb.bin_stats()[1]
        sets = make()
        for k, ds in enumerate(sets):
            ds.construct()
            f = tmp_path / ("%s_%s_%d.bin" % (name, mode, k))
            ds.save_binary(str(f))
            files.append(f.read_bytes())
        assert cb.bin_stats()[1] - before == (len(sets) if mode == "1" else 0)
    n = len(files) // 2
    for k in range(n):
        assert len(files[k]) > 100 and files[k] == files[n + k], k
    return n


PARAMS = {"objective": "binary", "max_bin": 63, "verbose": -1, "device_type": "gpu"}


@pytest.mark.parametrize("host_sparse", [None, "0", "1"])
def test_dataset_files_equal_host_build(monkeypatch, tmp_path, host_sparse):
    if host_sparse is None:
        monkeypatch.delenv("LGBM_AMD_HOST_SPARSE", raising=False)
    else:
        monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", host_sparse)
    m, y = _matrix(30011, 1)
    _build_both(monkeypatch, tmp_path, lambda: [lgb.Dataset(m, y, params=PARAMS)])


@pytest.mark.parametrize("case", ["float32_int64", "categorical", "no_bundle", "last_chunk_one_row"])
def test_dataset_files_equal_host_build_variants(monkeypatch, tmp_path, case):
    m, y = _matrix(4097, 2, dtype=np.float32 if case == "float32_int64" else np.float64)
    params, cat = dict(PARAMS), "auto"
    if case == "float32_int64":
        m.indptr = m.indptr.astype(np.int64)
    if case == "categorical":
        m = sp.csr_matrix(np.hstack([m.toarray(), np.random.RandomState(3).randint(0, 6, size=(m.shape[0], 2))]))
        cat = [40, 41]
    if case == "no_bundle":
        params["enable_bundle"] = False
    if case == "last_chunk_one_row":
        monkeypatch.setenv("LGBM_AMD_BIN_CHUNK_ROWS", "1024")
    _build_both(monkeypatch, tmp_path, lambda: [lgb.Dataset(m, y, params=params, categorical_feature=cat)])


def test_tile_edges_and_empty_sparse_group(monkeypatch, tmp_path):
    """a validation set whose sparse column 7 is stored at rows 255 and 256 of the compaction tiles
    only, and whose sparse column 8 has no stored row"""
    tile = ops.csr_bin_launch_info()["tile_rows"]
    monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", "1")
    m, y = _matrix(5000, 4)
    v = m[:3 * tile + 5].toarray()
    v[:, 7] = 0.0
    v[:, 8] = 0.0
    for r in (tile - 1, tile, 2 * tile - 1, 2 * tile, 3 * tile + 4):
        v[r, 7] = 2.5
    vm = sp.csr_matrix(v)

    def make():
        tr = lgb.Dataset(m, y, params=PARAMS)
        return [tr, lgb.Dataset(vm, y[:vm.shape[0]], reference=tr)]
    assert _build_both(monkeypatch, tmp_path, make) == 2


def test_validation_set_trains_the_same_model(monkeypatch):
    m, y = _matrix(20000, 5)
    vm, vy = _matrix(6000, 6)
    texts = []
    for mode in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cb.bin_stats()[1]
        tr = lgb.Dataset(m, y, params=PARAMS)
        va = lgb.Dataset(vm, vy, reference=tr)
        evals = {}
        bst = lgb.train(dict(PARAMS, num_leaves=15, metric="binary_logloss"), tr, num_boost_round=3, valid_sets=[va],
                        callbacks=[lgb.record_evaluation(evals)])
        assert cb.bin_stats()[1] - before == (2 if mode == "1" else 0)
        texts.append((bst.model_to_string(), evals))
    assert texts[0][0] == texts[1][0] and texts[0][1] == texts[1][1]
    assert texts[0][0].count("Tree=") == 3


def test_gate_without_the_knob(monkeypatch):
    """LGBM_AMD_DEVICE_BINNING unset: device_type=gpu and enough stored entries take the device"""
    monkeypatch.delenv("LGBM_AMD_DEVICE_BINNING", raising=False)
    rng = np.random.RandomState(8)
    n, per_row = 110000, 10   # 1.1M stored entries: over the gate of 2^20
    big = sp.csr_matrix((rng.randn(n * per_row), (rng.randint(0, 4, size=(n, per_row)) + 4 * np.arange(per_row)).ravel(),
                         np.arange(n + 1) * per_row), shape=(n, 40))
    small, _ = _matrix(3000, 9)
    for m, params, expect in ((big, PARAMS, 1), (big, dict(PARAMS, device_type="cpu"), 0), (small, PARAMS, 0)):
        before = cb.bin_stats()[1]
        lgb.Dataset(m, params=params).construct()
        assert cb.bin_stats()[1] - before == expect


def test_too_many_push_zero_features_stay_on_the_host(monkeypatch, tmp_path):
    """one feature more than the kernel's flag bitset holds: the whole matrix takes the host path,
    and the op refuses instead of running the kernel"""
    cap = ops.csr_bin_launch_info()["max_push_zero_features"]
    rng = np.random.RandomState(13)
    m = sp.csr_matrix((rng.rand(300, cap + 1) < 0.85).astype(np.float32))  # 1.0 is every column's most frequent value
    y = rng.rand(300).astype(np.float32)
    files = []
    for mode in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cb.bin_stats()[1]
        ds = lgb.Dataset(m, y, params=PARAMS).construct()
        assert cb.bin_stats()[1] == before
        f = tmp_path / ("pz_%s.bin" % mode)
        ds.save_binary(str(f))
        files.append(f.read_bytes())
    assert files[0] == files[1]
    with pytest.raises(LightGBMError, match="zeros pushed"):
        ops.csr_group_bins(ds, _csr_tensor(m.indptr[:5], m.indices[:m.indptr[4]], m.data[:m.indptr[4]], cap + 1))


def test_malformed_indptr_never_reaches_the_device(monkeypatch):
    """an indptr that descends is refused before any upload: the matrix goes to the host path,
    whose row reader raises on it -- the same error with device binning on and off"""
    rows = cb.base_rows(600)
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    train = cb.NativeDataset(*cb.flatten(rows), cb.NCOL, cb.PARAMS)
    indptr, indices, data = cb.flatten(rows)
    indptr = indptr.copy()
    indptr[300] = indptr[301] + 2
    errors = []
    for mode in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", mode)
        before = cb.bin_stats()[1]
        with pytest.raises(LightGBMError) as e:
            cb.NativeDataset(indptr, indices, data, cb.NCOL, cb.PARAMS, reference=train)
        errors.append(str(e.value))
        assert cb.bin_stats()[1] == before
    assert errors[0] == errors[1]
    # (and the well-formed matrix does go through the device with the same reference)
    before = cb.bin_stats()[1]
    arrays = cb.flatten(rows)
    valid = cb.NativeDataset(*arrays, cb.NCOL, cb.PARAMS, reference=train)
    assert cb.bin_stats()[1] == before + 1
    assert np.array_equal(valid.group_bins()[0], train.group_bins()[0])
