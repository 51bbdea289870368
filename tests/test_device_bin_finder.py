"""The first step of the bin finder on the device (src/device/bin_find_kernels.hip):
``ops.sample_distinct`` against the NumPy reference of tests/test_sample_distinct_host.py, bit for
bit, on the sample sizes at which the kernel's loops turn over, in every element type and layout and
on the edge columns; and a training Dataset of a GPU tensor built with the device bin finder forced
and with it off: the same binary file.
"""
import numpy as np
import pytest
import torch

import lightgbmv1_amd as lgb
from lightgbmv1_amd import ops
from test_sample_distinct_host import assert_same, edge_columns, edge_matrix, reference
from test_tensor_bins_host import CATS, matrix

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    pass


def sizes():
    info = ops.bin_find_launch_info()
    t = info["tile"]
    out = [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]
    for s in info["size_thresholds"]:
        out += [s - 1, s, s + 1]
    return sorted(set(out))


def values(n, ncol, seed):
    """columns by turns: few values with repeats and zeros, all different, NaNs and zeros among halves"""
    rng = np.random.RandomState(seed)
    X = rng.randn(n, ncol)
    X[:, 0::3] = X[:, 0::3].round(1)
    X[:, 2::3] = np.where(rng.rand(n, len(range(2, ncol, 3))) < 0.3, np.nan, (X[:, 2::3] * 2).round() / 2)
    return X


def laid_out(X, dtype, layout):
    t = torch.from_numpy(X).to(dtype).cuda()
    if layout == "column_major":
        t = t.t().contiguous().t()
    if layout == "view":  # non-unit strides in both dimensions
        base = torch.full((2 * t.shape[0], 3 * t.shape[1] + 1), 7.0, dtype=dtype, device="cuda")
        base[::2, 1::3] = t
        t = base[::2, 1::3]
        assert t.stride(1) == 3 and t.stride(0) == 2 * base.shape[1]
    return t


def check(t, rows=None):
    wide = t.to(torch.float64).cpu().numpy()
    if rows is not None:
        wide = wide[rows]
    before = ops.tensor_bin_stats(bin_find=True)
    got = ops.sample_distinct(t, rows)
    assert ops.tensor_bin_stats(bin_find=True) == before + 1
    assert_same(got, [reference(wide[:, c]) for c in range(wide.shape[1])], (tuple(t.shape), t.dtype))


@pytest.mark.parametrize("ncol", [1, 33])
@pytest.mark.parametrize("n", sizes())
def test_sample_sizes(n, ncol):
    assert ops.tensor_bin_launch_info()["gather_tile"] == 32
    check(laid_out(values(n, ncol, n), torch.float64, "contiguous"))


@pytest.mark.parametrize("layout", ["contiguous", "column_major", "view"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_dtypes_and_layouts(dtype, layout):
    n = ops.bin_find_launch_info()["tile"] + 1
    t = laid_out(values(n + 40, 33, 2) * 3, DTYPES[dtype], layout)
    check(t, np.random.RandomState(4).permutation(n + 40)[:n].astype(np.int32))
    # column 1 holds both signs: the passes over the zero low bits of the narrower types are skipped
    # (a double's 64 bits less the 29, 42 and 45 mantissa bits that float32, float16 and bfloat16
    # leave zero, in digits of 8)
    assert ops.sample_distinct(t, sort_passes=True)[1][3] == {"f16": 3, "bf16": 3, "f32": 5, "f64": 8}[dtype]


def test_more_than_one_pass_of_columns():
    """33 columns of a sample long enough that the 256 MiB rule takes 32 and then 1; the last
    column alone has more runs than the 32 before it together"""
    n = 210000
    X = np.random.RandomState(6).randint(-20, 21, (n, 33)) * 0.25
    X[:, 32] = np.random.RandomState(7).randn(n)
    check(laid_out(X, torch.float64, "contiguous"))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_edge_columns(dtype):
    """every edge column in one launch; the float64-only columns collapse in the narrower types"""
    t = laid_out(edge_matrix(), DTYPES[dtype], "contiguous")
    if dtype == "f64":
        got = dict(zip(edge_columns(), ops.sample_distinct(t)))
        assert got["ulp_chain"][1].tolist() == [3, 1] and got["every_byte"][0].size == 9
        assert got["all_zero"][0].size == 0 and got["all_nan"][2] == 7 and got["nans"][2] == 4
    check(t)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_dataset_with_the_device_bin_finder(monkeypatch, tmp_path, dtype):
    """two categorical columns (10, 11), sparse columns (6-9) and max_bin_by_feature"""
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "1")
    t = laid_out(matrix(3000, 9), DTYPES[dtype], "contiguous")
    params = {"objective": "binary", "max_bin": 63, "min_data_in_bin": 1, "min_data_in_leaf": 1, "verbose": -1,
              "device_type": "gpu", "max_bin_by_feature": [9 + 5 * c for c in range(12)]}
    files = []
    for knob, moved in (("0", 0), ("1", 1)):
        monkeypatch.setenv("LGBM_AMD_DEVICE_BIN_FIND", knob)
        before = ops.tensor_bin_stats(bin_find=True)
        ds = lgb.Dataset(t, np.zeros(3000, dtype=np.float32), params=params, categorical_feature=CATS)
        ds.construct().save_binary(str(tmp_path / (knob + ".bin")))
        files.append((tmp_path / (knob + ".bin")).read_bytes())
        assert ops.tensor_bin_stats(bin_find=True) - before == moved
    assert len(files[0]) > 1000 and files[0] == files[1]
