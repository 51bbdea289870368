"""SHAP contributions of small batches by the leaves-on-lanes kernel (src/device/shap_leaf_kernels.hip),
forced with ops.forest_predict(..., shap_kernel="leaves"), against the host predictor's float64
recursion (Booster.predict without a device).  The bound is the one of tests/helpers/contrib_cases.py
for the per-leaf form, 64 * 2**-52 * S per entry (S: the sum over trees of the largest |leaf
value|); each row's contributions also sum to its raw score within it.

The models put a tree on every edge of the kernel: 2 leaves; 63, 64, 65 and 130 leaves (the lane
stride of leaves, and of internal nodes at 64 / 65); a single-leaf tree between two others; 1, W and
W + 1 trees per class of 3 classes (the batch edge); 300 features (the accumulator is wider than
the workgroup) and 7,000 (it leaves LDS for a global tile); a repeated split feature on a path (the
six-feature models, the hand-written tree); a categorical split with NaNs in numerical and
categorical columns.  Rows 1, 5 and 65.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch  # (before the native library loads, as in tests/test_ops.py: one HIP runtime for both)

import lightgbmv1_amd as lgb
from lightgbmv1_amd import _native as nat
from lightgbmv1_amd import ops
from helpers import contrib_cases as cc
from helpers import forest_ref as fr

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 65)
MODELS = ["leaves2", "leaves63", "leaves64", "leaves65", "leaves130", "single_leaf_between", "classes_1",
          "classes_w", "classes_w1", "wide300", "wide7000", "special_values"]
LAYOUTS = ["float32", "float64", "sparse_csr", "sparse_csc"]


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    pass


def _train(params, X, y, rounds):
    params = dict(params, verbose=-1, num_threads=4, seed=1, deterministic=True, min_data_in_leaf=1)
    return lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=rounds)


@functools.lru_cache(maxsize=None)
def model(name):
    """(booster, 65 float64 rows that are float32 numbers) of a case"""
    rng = np.random.RandomState(MODELS.index(name) + 3)
    wide = ops.shap_launch_info()["wave_ladder"][0]
    if name.startswith("leaves"):  # six features: every deep path repeats some
        leaves = int(name[6:])
        X = rng.randn(3000, 6)
        y = np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + np.abs(X[:, 3]) + 0.1 * rng.randn(3000)
        bst = _train({"objective": "regression", "num_leaves": leaves}, X, y, 3)
        assert bst.dump_model()["tree_info"][0]["num_leaves"] == leaves
    elif name.startswith("classes"):
        rounds = {"classes_1": 1, "classes_w": wide, "classes_w1": wide + 1}[name]
        X = rng.randn(600, 6)
        y = np.argmax(X[:, :3] + 0.3 * rng.randn(600, 3), axis=1).astype(np.float64)
        bst = _train({"objective": "multiclass", "num_class": 3, "num_leaves": 15}, X, y, rounds)
    elif name.startswith("wide"):  # (7,001 doubles of accumulator do not fit in LDS beside four waves: a global tile)
        features = int(name[4:])
        X = rng.randn(600, features)
        y = X[:, ::features // 10].sum(axis=1) + 0.1 * rng.randn(600)
        bst = _train({"objective": "regression", "num_leaves": 15}, X, y, 5)
    elif name == "single_leaf_between":  # the last tree splits feature 2 twice on the path to leaves 2, 3
        trees = [fr.tree([fr.num(0, 0.0, 0, False, ~0, ~1)], [0.5, -0.25], [5, 11]),
                 fr.tree([], [0.125]),
                 fr.tree([fr.num(2, 0.5, 2, True, 1, 2), fr.cat(1, [1, 3], 0, ~0, ~1),
                          fr.num(2, 1.5, 0, False, ~2, ~3)], [1.0, -2.0, 0.75, 3.0], [3, 6, 4, 9])]
        bst = lgb.Booster(model_str=fr.model_text(trees, 4))
        X = rng.randn(65, 4)
        X[:, 1] = rng.randint(0, 5, 65)
        X[::7, 2] = np.nan
    else:  # the rows of tests/test_device_contrib.py's NaN case, and a NaN in a numerical column
        c = cc.case("categorical_zero_missing")
        bst, X = c.booster, c.X[:65].copy()
        X[::3, 1] = np.nan
        X[1::4, 3] = np.nan
        X[2::5, 0] = np.nan
    return bst, X[:65].astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def host(name):
    """the reference, once per model: contributions and raw scores of the 65 rows, and the bound"""
    bst, X = model(name)
    width = bst.num_model_per_iteration() * (bst.num_feature() + 1)
    return (bst.predict(X, pred_contrib=True).reshape(65, width),
            bst.predict(X, raw_score=True).reshape(65, -1), cc.tolerance(bst))


def tensor(X, layout):
    if layout in ("float32", "float64"):
        return torch.tensor(X, dtype=getattr(torch, layout), device="cuda")
    dense = torch.tensor(X, dtype=torch.float64 if layout == "sparse_csr" else torch.float32, device="cuda")
    return dense.to_sparse_csr() if layout == "sparse_csr" else dense.to_sparse_csc()


def _device_calls():
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DevicePredictCount", ctypes.byref(out))
    return out.value


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", MODELS)
def test_leaves_kernel_matches_the_host(name, layout):
    bst, X = model(name)
    want, raw, tol = host(name)
    classes = raw.shape[1]
    for n in ROWS:
        got = ops.forest_predict(bst, tensor(X[:n], layout), kind="contrib", shap_kernel="leaves").cpu().numpy()
        assert got.shape == (n, want.shape[1]) and np.all(np.isfinite(got))
        err = np.max(np.abs(got - want[:n]))
        add = np.max(np.abs(got.reshape(n, classes, -1).sum(axis=2) - raw[:n]))
        print("%s %s %d rows: |diff| %.3e, additivity %.3e, bound %.3e" % (name, layout, n, err, add, tol))
        assert err <= tol and add <= tol


def test_two_runs_give_the_same_bits():
    bst, X = model("leaves130")
    Xd = tensor(X, "float64")
    assert torch.equal(ops.forest_predict(bst, Xd, kind="contrib", shap_kernel="leaves"),
                       ops.forest_predict(bst, Xd, kind="contrib", shap_kernel="leaves"))


def test_small_batches_are_routed_to_the_kernel():
    bst, X = model("leaves63")
    want, _, tol = host("leaves63")
    before = _device_calls()
    got = bst.predict(X[:64], pred_contrib=True, device_type="gpu")
    assert _device_calls() == before + 1, "64 rows of contributions did not run on the device"
    assert np.max(np.abs(got - want[:64])) <= tol
    Xd = tensor(X[:5], "float32")
    assert torch.equal(bst.predict_device(Xd, pred_contrib=True),
                       ops.forest_predict(bst, Xd, kind="contrib", shap_kernel="leaves"))


def test_leaves_raises_where_the_plan_cannot_serve():
    """a chain of 119 distinct features: one wave's path weights and terms are over the LDS budget,
    so "auto" runs rows-on-lanes and "leaves" is an error"""
    bst = lgb.Booster(model_str=cc.chain_model_text(119))
    Xd = torch.tensor(cc.chain_rows(119, n=5), device="cuda")
    assert ops.forest_predict(bst, Xd, kind="contrib").shape == (5, 120)
    with pytest.raises(lgb.LightGBMError):
        ops.forest_predict(bst, Xd, kind="contrib", shap_kernel="leaves")
