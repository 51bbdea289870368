"""Refit on the device (GBDT::RefitTree with a device learner; src/device/refit_kernels.hip).

* `ops.leaf_sums` / `ops.add_leaf_values`: the two per-tree kernels on caller-owned tensors,
  against the host evaluator of the same fixed-point rule (bit-identical), against exact sums
  within the rounding bound of tests/test_refit_sums_host.py, and against NumPy float64.
* Staging of the leaf matrix: windows, the uint16 and int32 column forms, and the validation of
  every entry before anything uses it.
* Whole refits: a teacher-forced replay of the device's arithmetic with a derived bound, the CPU
  learner's refit with measured tolerances (profiles/r09_device_refit.md), LGBM_AMD_HOST_REFIT,
  the CLI, and run-to-run determinism.
"""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import lightgbmv1_amd as lgb
import lightgbmv1_amd.ops  # noqa: F401  (lgb.ops)
from lightgbmv1_amd import _native as nat
from test_refit_sums_host import K_EPSILON, check_against_exact, columns, host_leaf_sums, trees_only

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(lgb.__file__), "lib", "lightgbm")
ROWS = [1, 63, 64, 65, 255, 256, 257, 1025]


@pytest.fixture(scope="module")
def info(gpu_available):
    return lgb.ops.refit_launch_info()


def _wrap_rows(info):
    """one row more than a full pass of the leaf-sum launch covers: every thread's loop runs again"""
    return info["max_grid"] * info["block"] * info["unroll"] + 1


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_leaf_sums(leaf, grad, hess, num_leaves):
    sg, sh, cnt, exps = lgb.ops.leaf_sums(_gpu(leaf), _gpu(grad), _gpu(hess), num_leaves)
    return sg.cpu().numpy(), sh.cpu().numpy(), cnt.cpu().numpy(), np.array(exps, dtype=np.int32)


def _leaf_counts(info):
    # 1, 2, 64; the LDS limit and one past it (the global-table path); 70000: int32 columns
    return [1, 2, 64, info["lds_leaves"], info["lds_leaves"] + 1, 70000]


def _check_leaf_sums(leaf, grad, hess, num_leaves):
    dev = _device_leaf_sums(leaf, grad, hess, num_leaves)
    host = host_leaf_sums(leaf, grad, hess, num_leaves)
    for d, h in zip(dev, host):  # the same integer rule: bit-identical
        assert np.array_equal(d.view(np.int64) if d.dtype == np.float64 else d,
                              h.view(np.int64) if h.dtype == np.float64 else h)
    check_against_exact(leaf, grad, hess, num_leaves, dev)
    again = _device_leaf_sums(leaf, grad, hess, num_leaves)
    for d, a in zip(dev, again):  # run-to-run bitwise
        assert d.tobytes() == a.tobytes()


@pytest.mark.parametrize("n", ROWS)
def test_leaf_sums_equal_host_rule_and_exact_sums(info, n):
    for num_leaves in _leaf_counts(info):
        rs, grad, hess = columns(n, 7 * n + num_leaves)
        _check_leaf_sums(rs.randint(0, num_leaves, n).astype(np.int32), grad, hess, num_leaves)


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4, 5])
def test_leaf_sums_when_the_grid_stride_loop_wraps(info, which):
    num_leaves = _leaf_counts(info)[which]
    n = _wrap_rows(info)
    rs, grad, hess = columns(n, 900 + which)
    _check_leaf_sums(rs.randint(0, num_leaves, n).astype(np.int32), grad, hess, num_leaves)


@pytest.mark.parametrize("n", [1, 65, 1025])
def test_leaf_sums_one_leaf_and_last_leaf_only(info, n):
    rs, grad, hess = columns(n, 50 + n)
    for num_leaves in _leaf_counts(info)[2:]:
        for only in (0, num_leaves - 1):
            _check_leaf_sums(np.full(n, only, dtype=np.int32), grad, hess, num_leaves)


def test_leaf_sums_all_zero_gradients(info):
    leaf = (np.arange(300) % 7).astype(np.int32)
    z = np.zeros(300, dtype=np.float32)
    sg, sh, cnt, exps = _device_leaf_sums(leaf, z, z, 7)
    assert np.all(sg == 0.0) and np.all(sh == 0.0) and np.array_equal(cnt, np.bincount(leaf, minlength=7))
    assert np.array_equal(exps, host_leaf_sums(leaf, z, z, 7)[3])


def test_ops_reject_a_leaf_id_outside_the_tree(info):
    one = np.ones(100, dtype=np.float32)
    for bad in (5, -1):
        leaf = np.zeros(100, dtype=np.int32)
        leaf[37] = bad
        with pytest.raises(lgb.basic.LightGBMError):
            _device_leaf_sums(leaf, one, one, 5)
        score = torch.zeros(100, dtype=torch.float64).cuda()
        with pytest.raises(lgb.basic.LightGBMError):
            lgb.ops.add_leaf_values(score, _gpu(leaf), torch.ones(5, dtype=torch.float64).cuda())
        assert torch.all(score == 0.0)


@pytest.mark.parametrize("n", ROWS + ["wrap"])
def test_add_leaf_values_is_one_double_add_per_row(info, n):
    n = _wrap_rows(info) if n == "wrap" else n
    for num_leaves in (1, 64, info["value_lds_leaves"], info["value_lds_leaves"] + 1, 70000):
        rs = np.random.RandomState(n % 1000 + num_leaves)
        score = rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)
        values = rs.randn(num_leaves)
        leaf = rs.randint(0, num_leaves, n).astype(np.int32)
        leaf[-1] = num_leaves - 1
        out = lgb.ops.add_leaf_values(_gpu(score), _gpu(leaf), _gpu(values)).cpu().numpy()
        assert out.tobytes() == (score + values[leaf]).tobytes()


# ---------------------------------------------------------------- whole refits
def _data(seed, n, f=10):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, f)
    y = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + np.sin(X[:, 3]) + 0.1 * rs.randn(n)
    return rs, X, y.astype(np.float32).astype(np.float64)


def _refit(base, X, y, params, decay=0.9, weight=None, group=None, leaves=None):
    """Booster.refit with a weight / group on the new data and an optional leaf matrix of the
    caller's: the refitted booster (LGBM_BoosterRefit)"""
    if leaves is None:
        leaves = base.predict(X, pred_leaf=True).reshape(len(X), -1)
    leaves = np.ascontiguousarray(leaves, dtype=np.int32)
    p = dict(params, refit_decay_rate=decay, verbose=-1)
    out = lgb.Booster(p, lgb.Dataset(X, y, weight=weight, group=group, params=p))
    nat.call("LGBM_BoosterMerge", out.handle, base._to_predictor().handle)
    nat.call("LGBM_BoosterRefit", out.handle, leaves.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
             ctypes.c_int32(leaves.shape[0]), ctypes.c_int32(leaves.shape[1]))
    return out


def _leaf_values(bst):
    """per tree, the leaf values of the model text (17 significant digits: the doubles themselves)"""
    return [np.array(ln.split("=")[1].split(), dtype=np.float64)
            for ln in bst.model_to_string().split("\n") if ln.startswith("leaf_value=")]


@pytest.fixture(scope="module")
def regression_model(gpu_available):
    """8 trees of 15 leaves on 3000 x 10, trained on the CPU; a second sample to refit on"""
    _, X, y = _data(1, 3000)
    params = dict(objective="regression", num_leaves=15, verbose=-1, device_type="cpu", min_data_in_leaf=20)
    base = lgb.train(params, lgb.Dataset(X, y), num_boost_round=8)
    _, X2, y2 = _data(2, 3000)
    return base, X2, y2


STAGING = dict(objective="regression", device_type="gpu")


def test_windows_and_column_widths_give_one_model(regression_model, monkeypatch):
    """n = 1025 rows and 7 trees: no multiple of the transpose tile either way"""
    base, X2, y2 = regression_model
    X, y = X2[:1025], y2[:1025]
    leaves = base.predict(X, pred_leaf=True).reshape(1025, -1)[:, :7]
    seven = lgb.Booster(model_str=base.model_to_string(num_iteration=7), silent=True)
    texts = {}
    for name, env in (("default", {}), ("window1", {"LGBM_AMD_REFIT_WINDOW": "1"}),
                      ("window3", {"LGBM_AMD_REFIT_WINDOW": "3"}), ("wide", {"LGBM_AMD_REFIT_WIDE": "1"}),
                      ("wide_window3", {"LGBM_AMD_REFIT_WIDE": "1", "LGBM_AMD_REFIT_WINDOW": "3"})):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            texts[name] = trees_only(_refit(seven, X, y, STAGING, leaves=leaves).model_to_string())
    assert len(texts["default"]) > 1000
    for name, text in texts.items():
        assert text == texts["default"], name
    cpu = _refit(seven, X, y, dict(STAGING, device_type="cpu"), leaves=leaves)
    for a, b in zip(_leaf_values(cpu), _leaf_values(lgb.Booster(model_str=texts["default"], silent=True))):
        np.testing.assert_allclose(b, a, rtol=1e-6, atol=1e-9)  # (not the seven old trees again)


@pytest.mark.parametrize("window", [None, "1"])
def test_an_entry_outside_its_tree_is_rejected_and_changes_nothing(regression_model, monkeypatch, window):
    base, X2, y2 = regression_model
    X, y = X2[:1025], y2[:1025]
    good = base.predict(X, pred_leaf=True).reshape(1025, -1)
    bad = good.copy()
    bad[700, 6] = len(_leaf_values(base)[6])
    if window is not None:
        monkeypatch.setenv("LGBM_AMD_REFIT_WINDOW", window)
    p = dict(STAGING, refit_decay_rate=0.9, verbose=-1)
    bst = lgb.Booster(p, lgb.Dataset(X, y, params=p))
    nat.call("LGBM_BoosterMerge", bst.handle, base._to_predictor().handle)
    before = bst.model_to_string()

    def call(leaves):
        leaves = np.ascontiguousarray(leaves, dtype=np.int32)
        nat.call("LGBM_BoosterRefit", bst.handle, leaves.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                 ctypes.c_int32(leaves.shape[0]), ctypes.c_int32(leaves.shape[1]))

    with pytest.raises(lgb.basic.LightGBMError, match="tree 6"):
        call(bad)
    assert bst.model_to_string() == before
    # ... the training scores included: the same booster now refits as a fresh one does
    call(good)
    assert trees_only(bst.model_to_string()) == trees_only(_refit(base, X, y, STAGING, leaves=good).model_to_string())


def _scale_exp(max_abs, n):
    """the rule of src/device/refit_quant.h: the largest e with n * max * 2^e < 2^53, taking n up
    to a power of two and max up to the power of two above it"""
    if max_abs == 0.0:
        return 0
    return 53 - (n - 1).bit_length() - math.frexp(max_abs)[1]


@pytest.mark.parametrize("decay,l2", [(0.9, 0.0), (0.0, 1.0)])
def test_teacher_forced_replay_of_a_regression_refit(regression_model, decay, l2):
    """Every iteration of the device refit, replayed in NumPy from the device's own earlier trees.

    The scores before tree t are the init score (0: a refit starts from a fresh booster) plus the
    device-refitted values of trees 0 .. t-1 at each row's leaf, one float64 add per tree in tree
    order: bitwise what the device adds.  Then g = float32(score - label), h = 1, the exact
    per-leaf sums S_g (rational) and S_h = count, and the leaf-output formula
        new = decay * old + (1 - decay) * shrinkage * out,  out = -S_g / (kEps + count + lambda_l2).
    The device sums g in fixed point: each row rounded once to a multiple of 2^-e_g, the integer
    sums exact, so its sum is within count * 2^-(e_g + 1) of S_g; h = 1 is a multiple of 2^-e_h,
    its sum exact.  Through the formula that is at most
        (1 - decay) * shrinkage * count * 2^-(e_g + 1) / (kEps + count + lambda_l2)
    in the leaf value, plus the roundings of the handful of double operations on either side:
    8 * 2^-53 * (|decay * old| + |(1 - decay) * shrinkage * out|).  e_g follows from max |g| and
    the row count by the rule of src/device/refit_quant.h (_scale_exp).

    On the parent of the commit that added the device refit this test fails at tree 1: its score
    update walked the merged trees' zero bin thresholds (profiles/r09_device_refit.md)."""
    base, X2, y2 = regression_model
    params = dict(objective="regression", device_type="gpu", lambda_l2=l2)
    dev = _refit(base, X2, y2, params, decay=decay)
    leaves = base.predict(X2, pred_leaf=True).reshape(len(X2), -1)
    old, new = _leaf_values(base), _leaf_values(dev)
    text = base.model_to_string()
    shrink = [float(ln.split("=")[1]) for ln in text.split("\n") if ln.startswith("shrinkage=")]
    n = len(X2)
    score = np.zeros(n)
    worst = 0.0
    for t in range(8):
        g = (score - y2).astype(np.float32)
        e_g = _scale_exp(float(np.max(np.abs(g))), n)
        units = [int(v) for v in np.ldexp(g.astype(np.float64), 149)]  # exact integers, units of 2^-149
        for leaf in range(len(old[t])):
            rows = np.nonzero(leaves[:, t] == leaf)[0]
            count = len(rows)
            s_g = Fraction(sum(units[i] for i in rows), 1 << 149)
            denom = K_EPSILON + count + l2
            out = float(-s_g / Fraction(denom))
            want = decay * old[t][leaf] + (1.0 - decay) * (out * shrink[t])
            bound = (1.0 - decay) * shrink[t] * count * 2.0 ** -(e_g + 1) / denom \
                + 8 * 2.0 ** -53 * (abs(decay * old[t][leaf]) + abs((1.0 - decay) * shrink[t] * out))
            err = abs(new[t][leaf] - want)
            worst = max(worst, err / bound if bound > 0 else 0.0)
            assert err <= bound, (t, leaf, new[t][leaf], want, err, bound)
        score = score + new[t][leaves[:, t]]
    print("teacher-forced replay decay=%g lambda_l2=%g: largest error / bound = %.3g" % (decay, l2, worst))


# The device's gradient kernels are not bitwise the host's, and a difference feeds forward through
# the scores: the tolerances against the CPU learner's refit are measured, not derived.  Each
# constant is the largest leaf-value difference seen (profiles/r09_device_refit.md, "Against the
# CPU learner"), relative to the model's largest |leaf value|; the test allows 8x, for the leaf
# values and, relative to the largest |raw prediction|, for the predictions -- orders of magnitude
# below the O(1) of a wrong leaf assignment.  The recorded differences are last-bit ones: both
# sides sum the same fp32 gradients, the device exactly and the host in doubles; weighted
# regression, whose gradients need no exp, came out bit-equal (0), and 8 x 0 asks for that again.
CPU_CASES = {
    # objective: (parameters, recorded leaf-value difference)
    "binary": (dict(objective="binary"), 3.67e-17),                         # profiles/r09_device_refit.md
    "multiclass": (dict(objective="multiclass", num_class=3), 1.09e-17),    # profiles/r09_device_refit.md
    "regression_weighted": (dict(objective="regression"), 0.0),             # profiles/r09_device_refit.md
    # (no device gradient kernel: the host's gradients are uploaded and feed the same kernels)
    "multiclassova": (dict(objective="multiclassova", num_class=3), 1.26e-17),  # profiles/r09_device_refit.md
    "lambdarank": (dict(objective="lambdarank", min_data_in_leaf=20), 1.84e-17),  # profiles/r09_device_refit.md
}


def _case_data(name, seed, n=3000):
    rs, X, y = _data(seed, n)
    weight = group = None
    if name == "binary":
        y = (y > 0).astype(np.float64)
    elif name in ("multiclass", "multiclassova"):
        y = np.digitize(y, [-0.7, 0.7]).astype(np.float64)
    elif name == "regression_weighted":
        weight = rs.rand(n) + 0.5
    elif name == "lambdarank":
        y = np.clip(np.round(y + 1.5), 0, 4)
        group = np.full(n // 30, 30)
    return X, y, weight, group


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_device_refit_against_the_cpu_learners(gpu_available, name):
    extra, recorded = CPU_CASES[name]
    params = dict(extra, num_leaves=15, verbose=-1)
    X, y, w, grp = _case_data(name, 21)
    base = lgb.train(dict(params, device_type="cpu"), lgb.Dataset(X, y, weight=w, group=grp), num_boost_round=8)
    X2, y2, w2, grp2 = _case_data(name, 22)
    cpu = _refit(base, X2, y2, dict(params, device_type="cpu"), weight=w2, group=grp2)
    dev = _refit(base, X2, y2, dict(params, device_type="gpu"), weight=w2, group=grp2)
    a, b, o = np.concatenate(_leaf_values(cpu)), np.concatenate(_leaf_values(dev)), np.concatenate(_leaf_values(base))
    assert np.max(np.abs(a - o)) > 1e-3 * np.max(np.abs(o))  # (the refit moved the values)
    leaf_diff = np.max(np.abs(a - b)) / np.max(np.abs(a))
    pa = cpu.predict(X2, raw_score=True, device_type="cpu")
    pb = dev.predict(X2, raw_score=True, device_type="cpu")
    pred_diff = np.max(np.abs(pa - pb)) / np.max(np.abs(pa))
    print("device refit against cpu, %s: leaf values %.3g, predictions %.3g" % (name, leaf_diff, pred_diff))
    assert leaf_diff <= 8 * recorded
    assert pred_diff <= 8 * recorded


def test_host_refit_knob_still_runs(regression_model, monkeypatch):
    base, X2, y2 = regression_model
    monkeypatch.setenv("LGBM_AMD_HOST_REFIT", "1")
    host = _refit(base, X2, y2, dict(objective="regression", device_type="gpu"))
    monkeypatch.delenv("LGBM_AMD_HOST_REFIT")
    dev = _refit(base, X2, y2, dict(objective="regression", device_type="gpu"))
    hv, dv = _leaf_values(host), _leaf_values(dev)
    assert all(np.all(np.isfinite(v)) for v in hv)
    # the first tree is fitted before that branch updates any score: the same sums, host doubles
    np.testing.assert_allclose(hv[0], dv[0], rtol=1e-6, atol=1e-9)


def test_cli_refit_gives_the_python_refit(gpu_available, tmp_path):
    rs = np.random.RandomState(4)
    X = rs.rand(2000, 8)
    y = (X[:, 0] + 0.5 * X[:, 1] + 0.1 * rs.rand(2000) > 0.8).astype(int)
    for name, sl in (("train.tsv", slice(0, 1500)), ("test.tsv", slice(1500, 2000))):
        np.savetxt(str(tmp_path / name), np.column_stack([y[sl], X[sl]]), delimiter="\t", fmt="%.10g")

    def run(args):
        r = subprocess.run([CLI] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode == 0, r.stdout.decode()

    run(["task=train", "objective=binary", "device_type=cpu", "data=train.tsv", "num_trees=5", "num_leaves=15",
         "output_model=model.txt", "verbose=-1"])
    run(["task=refit", "objective=binary", "device_type=gpu", "data=test.tsv", "input_model=model.txt",
         "output_model=refit.txt", "verbose=-1"])
    test = np.loadtxt(str(tmp_path / "test.tsv"))
    base = lgb.Booster(model_file=str(tmp_path / "model.txt"), params=dict(objective="binary", device_type="gpu", verbose=-1))
    py = base.refit(np.ascontiguousarray(test[:, 1:]), test[:, 0]).model_to_string()
    cli = (tmp_path / "refit.txt").read_text()
    assert cli[cli.index("Tree=0"):cli.index("end of trees")] == py[py.index("Tree=0"):py.index("end of trees")]


def test_two_device_refits_give_one_model(regression_model):
    base, X2, y2 = regression_model
    params = dict(objective="regression", device_type="gpu")
    assert _refit(base, X2, y2, params).model_to_string() == _refit(base, X2, y2, params).model_to_string()
