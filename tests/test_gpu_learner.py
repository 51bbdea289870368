"""MI355X learner vs the CPU serial learner (same binned data, same parameters).

Device histograms are exact int64 sums of fixed-point (g, h) (per-tree power-of-two
scales), the host's are fp64 sums, and the device scans evaluate thresholds with parallel
prefix sums, so trees are compared structurally (split features / thresholds of the
first tree) and by metric, not bit for bit.
"""
import json

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from helpers.booster_probe import last_gradients as _last_gradients, train_scores as _train_scores

pytestmark = pytest.mark.gpu


def _data(n=60000, f=16, seed=1):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, f).astype(np.float32)
    X[:, 3] = np.abs(X[:, 3])  # skewed feature
    X[rng.rand(n) < 0.05, 5] = np.nan  # missing values
    X[:, 6] = np.where(rng.rand(n) < 0.6, 0.0, X[:, 6])  # zero-heavy feature (most frequent bin 0)
    X[:, 7] = np.where(rng.rand(n) < 0.7, 2.5, X[:, 7])  # most frequent bin not 0
    logit = X[:, 0] + 0.7 * X[:, 1] * X[:, 2] - 0.5 * X[:, 3] + 0.3 * np.nan_to_num(X[:, 5]) + 0.4 * X[:, 7]
    y = (logit + 0.3 * rng.randn(n) > 0).astype(np.float32)
    return X, y


def _auc(y, p):
    from scipy.stats import rankdata
    r = rankdata(p)
    pos = y > 0.5
    return (r[pos].sum() - pos.sum() * (pos.sum() + 1) / 2) / (pos.sum() * (~pos).sum())


def _train(X, y, device, rounds=20, **extra):
    params = {"objective": "binary", "num_leaves": 31, "max_bin": 63, "learning_rate": 0.1,
              "min_data_in_leaf": 20, "verbose": -1, "device_type": device, "seed": 7}
    params.update(extra)
    ds = lgb.Dataset(X, y, params=params)
    return lgb.train(params, ds, rounds, verbose_eval=False)


def test_first_tree_matches_cpu(gpu_available):
    X, y = _data()
    cpu = _train(X, y, "cpu", rounds=1).dump_model()["tree_info"][0]["tree_structure"]
    gpu = _train(X, y, "gpu", rounds=1).dump_model()["tree_info"][0]["tree_structure"]
    # root and its children split on the same features at the same thresholds
    for path in ([], ["left_child"], ["right_child"]):
        a, b = cpu, gpu
        for k in path:
            a, b = a[k], b[k]
        assert a["split_feature"] == b["split_feature"]
        assert a["threshold"] == pytest.approx(b["threshold"])
        assert a["split_gain"] == pytest.approx(b["split_gain"], rel=1e-3)
        assert a["internal_count"] == b["internal_count"]


def test_auc_parity_with_cpu(gpu_available):
    X, y = _data()
    Xt, yt = _data(20000, seed=2)
    p_cpu = _train(X, y, "cpu", rounds=30).predict(Xt)
    p_gpu = _train(X, y, "gpu", rounds=30).predict(Xt)
    assert abs(_auc(yt, p_cpu) - _auc(yt, p_gpu)) < 2e-3
    assert np.corrcoef(p_cpu, p_gpu)[0, 1] > 0.995


def test_regression_and_bagging_on_device(gpu_available):
    rng = np.random.RandomState(3)
    X = rng.randn(40000, 10).astype(np.float32)
    y = (2 * X[:, 0] + np.sin(3 * X[:, 1]) + 0.1 * rng.randn(40000)).astype(np.float32)
    params = dict(objective="regression", bagging_fraction=0.7, bagging_freq=1, feature_fraction=0.8)
    b_gpu = _train(X, y, "gpu", rounds=40, **params)
    b_cpu = _train(X, y, "cpu", rounds=40, **params)
    mse_gpu = np.mean((b_gpu.predict(X) - y) ** 2)
    mse_cpu = np.mean((b_cpu.predict(X) - y) ** 2)
    assert mse_gpu < 0.2 and abs(mse_gpu - mse_cpu) < 0.05


def test_host_assisted_mode_categorical(gpu_available):
    rng = np.random.RandomState(4)
    X = rng.randn(30000, 6).astype(np.float32)
    X[:, 0] = rng.randint(0, 12, size=30000)
    y = ((X[:, 0] % 3 == 0) * 1.5 + X[:, 1] + 0.2 * rng.randn(30000) > 0.7).astype(np.float32)
    params = {"objective": "binary", "num_leaves": 15, "verbose": -1, "device_type": "gpu"}
    ds = lgb.Dataset(X, y, params=params, categorical_feature=[0])
    b = lgb.train(params, ds, 20, verbose_eval=False)
    assert _auc(y, b.predict(X)) > 0.9
    model = b.dump_model()
    assert any("num_cat" in t and t["num_cat"] > 0 for t in model["tree_info"])


def test_multiclass_on_device(gpu_available):
    rng = np.random.RandomState(5)
    X = rng.randn(30000, 8).astype(np.float32)
    y = np.argmax(X[:, :3] + 0.3 * rng.randn(30000, 3), axis=1).astype(np.float32)
    b = _train(X, y, "gpu", rounds=20, objective="multiclass", num_class=3)
    acc = np.mean(np.argmax(b.predict(X), axis=1) == y)
    assert acc > 0.85


def test_rccl_comm_single_rank(gpu_available):
    """The RCCL device communicator (the multi-GPU histogram all-reduce path) on one rank."""
    import ctypes
    import numpy as np
    from lightgbmv1_amd.basic import _load_lib
    lib = _load_lib()
    size = ctypes.c_int(0)
    assert lib.LGBM_AMD_RcclUniqueIdSize(ctypes.byref(size)) == 0
    uid = np.zeros(size.value, dtype=np.uint8)
    assert lib.LGBM_AMD_RcclGetUniqueId(uid.ctypes.data_as(ctypes.c_char_p)) == 0
    assert lib.LGBM_AMD_RcclInit(ctypes.c_int(1), ctypes.c_int(0), ctypes.c_int(0),
                                 uid.ctypes.data_as(ctypes.c_char_p)) == 0
    ok = ctypes.c_int(0)
    try:
        assert lib.LGBM_AMD_RcclSelfTest(ctypes.byref(ok)) == 0
        assert ok.value == 1
        ok.value = 0
        assert lib.LGBM_AMD_RcclGraphSelfTest(ctypes.byref(ok)) == 0
        assert ok.value == 1
    finally:
        lib.LGBM_AMD_RcclFree()


def _rank_data(nq=300, seed=6):
    rng = np.random.RandomState(seed)
    sizes = rng.randint(5, 60, size=nq)
    n = int(sizes.sum())
    X = rng.randn(n, 12).astype(np.float32)
    rel = X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.randn(n)
    y = np.clip(np.floor(rel + 1.5), 0, 4).astype(np.float32)
    return X, y, sizes


def _ndcg_at(y, p, group, k=10):
    out, start = [], 0
    for g in group:
        yy, pp = y[start:start + g], p[start:start + g]
        start += g
        order = np.argsort(-pp, kind="stable")
        disc = 1.0 / np.log2(np.arange(2, g + 2))
        gain = 2.0 ** yy - 1
        dcg = np.sum(gain[order][:k] * disc[:k])
        idcg = np.sum(np.sort(gain)[::-1][:k] * disc[:k])
        out.append(dcg / idcg if idcg > 0 else 1.0)
    return float(np.mean(out))


@pytest.mark.parametrize("objective", ["lambdarank", "rank_xendcg"])
def test_listwise_gradients_on_device(gpu_available, objective):
    """LambdaRank / XE-NDCG gradients from the per-query HIP kernel: NDCG parity with the CPU learner."""
    X, y, group = _rank_data()
    res = {}
    for device in ("cpu", "gpu"):
        params = {"objective": objective, "num_leaves": 15, "min_data_in_leaf": 5, "learning_rate": 0.1,
                  "verbose": -1, "device_type": device, "seed": 3}
        ds = lgb.Dataset(X, y, group=group, params=params)
        b = lgb.train(params, ds, 30, verbose_eval=False)
        res[device] = _ndcg_at(y, b.predict(X), group)
    assert res["gpu"] > 0.7
    assert abs(res["gpu"] - res["cpu"]) < 0.02


@pytest.mark.parametrize("extra", [{}, {"lambdarank_norm": False}, {"weighted": True}, {"sigmoid": 2.5},
                                   {"big": True}, {"mid": True}, {"no_pairs": True}],
                         ids=["norm", "no_norm", "weighted", "sigmoid", "queries_over_2048_docs",
                              "queries_1600_to_2048_docs", "pair_scratch_over_budget"])
def test_lambdarank_device_gradients_equal_host(gpu_available, extra, monkeypatch):
    """The device LambdaRank kernel replays the reference's accumulation (float sums of each
    document's lower-side pairs in the sorted order of the higher side, the double sum of its
    higher-side pairs added at its own position, the host's sigmoid table; reference
    rank_objective.hpp:139-229): its gradients equal the host objective's bit for bit, from
    random initial scores with ties (so device GOSS samples the host's rows)."""
    X, y, group = _rank_data(nq=200, seed=8)
    extra = dict(extra)
    if extra.pop("big", False):
        # queries longer than the LDS staging (kRankMaxDocs = 2048): the global-scratch kernel
        rng0 = np.random.RandomState(4)
        group = np.array([3000, 40, 2500, 30, 60], dtype=np.int64)
        X = rng0.randn(int(group.sum()), 6).astype(np.float32)
        y = np.clip(np.floor(X[:, 0] + 0.3 * rng0.randn(len(X)) + 1.5), 0, 4).astype(np.float32)
    if extra.pop("mid", False):
        # queries staged in LDS whose staging passes 64 KiB (44 B per document: 1490+ documents)
        rng0 = np.random.RandomState(5)
        group = np.array([1600, 50, 2048, 1900, 20], dtype=np.int64)
        X = rng0.randn(int(group.sum()), 6).astype(np.float32)
        y = np.clip(np.floor(X[:, 0] + 0.3 * rng0.randn(len(X)) + 1.5), 0, 4).astype(np.float32)
    if extra.pop("no_pairs", False):
        # a pair scratch budget of 0: each pair evaluated from both of its documents
        monkeypatch.setenv("LGBM_AMD_RANK_PAIR_MB", "0")
    rng = np.random.RandomState(2)
    init = np.round(rng.randn(len(y)) * 2, 1)  # (rounded: tied scores inside queries)
    weight = None
    if extra.pop("weighted", False):
        weight = np.repeat(rng.choice([0.5, 1.0, 2.0], size=len(group)), group).astype(np.float32)
    out = {}
    for device in ("cpu", "gpu"):
        params = dict({"objective": "lambdarank", "num_leaves": 7, "verbose": -1, "device_type": device}, **extra)
        ds = lgb.Dataset(X, y, group=group, init_score=init, weight=weight, params=params)
        bst = lgb.Booster(params, ds)
        bst.update()
        out[device] = _last_gradients(bst)
    for k in range(2):
        assert np.abs(out["cpu"][k]).sum() > 0
        np.testing.assert_array_equal(out["gpu"][k], out["cpu"][k])


@pytest.mark.parametrize("boosting", ["gbdt", "goss"])
def test_lambdarank_ndcg_equals_cpu_learner(gpu_available, boosting):
    """Config #4's parity at test size: LambdaRank (and LambdaRank + GOSS, with the CPU
    learner's GOSS blocks laid out as the device's: one per 1024 rows) on the device -- fx64
    histograms, chosen by gpu_hist_precision=auto for listwise objectives, and gradients equal
    to the host's bit for bit -- gives the CPU learner's NDCG@10."""
    X, y, group = _rank_data(nq=400, seed=11)
    n = len(y)
    res = {}
    for device in ("cpu", "gpu"):
        params = {"objective": "lambdarank", "num_leaves": 31, "min_data_in_leaf": 5, "learning_rate": 0.1,
                  "max_bin": 63, "verbose": -1, "device_type": device, "seed": 3, "boosting": boosting}
        if boosting == "goss" and device == "cpu":
            params["num_threads"] = (n + 1023) // 1024
        ds = lgb.Dataset(X, y, group=group, params=params)
        b = lgb.train(params, ds, 40, verbose_eval=False)
        res[device] = _ndcg_at(y, b.predict(X), group)
    assert res["gpu"] > 0.7
    assert abs(res["gpu"] - res["cpu"]) < 1e-6, res


def _bag_counts(device, boosting, rounds, fixed_gradients=False, **extra):
    X, y = _data(50000, seed=9)
    params = {"objective": "binary", "num_leaves": 15, "max_bin": 63, "verbose": -1, "device_type": device,
              "boosting": boosting, "seed": 11}
    params.update(extra)
    fobj = None
    if fixed_gradients:  # the sampler's input does not depend on the (device vs host) trees
        rng = np.random.RandomState(0)
        g = rng.randn(len(y)).astype(np.float32)
        h = (rng.rand(len(y)) + 0.5).astype(np.float32)

        def fobj(preds, ds):
            return g, h
    b = lgb.train(params, lgb.Dataset(X, y, params=params), rounds, fobj=fobj, verbose_eval=False)
    out = []
    for t in b.dump_model()["tree_info"]:
        root = t["tree_structure"]
        left = root.get("left_child", {})
        # the root and its left child's row counts depend on exactly which rows are in the bag
        out.append((root.get("internal_count"), left.get("internal_count", left.get("leaf_count"))))
    return out


def test_device_bagging_matches_host_draw(gpu_available):
    """Device bagging uses the reference's per-1024-row generators: the bags are identical."""
    kw = dict(bagging_fraction=0.6, bagging_freq=2, bagging_seed=5)
    assert _bag_counts("gpu", "gbdt", 6, **kw) == _bag_counts("cpu", "gbdt", 6, **kw)


def test_device_bagging_with_poisoned_args(monkeypatch, gpu_available):
    """The learner's gradient and bagging launches set every argument field: with the structs
    poisoned first (LGBM_AMD_POISON_ARGS=1) the bags still equal the host draw."""
    monkeypatch.setenv("LGBM_AMD_POISON_ARGS", "1")
    kw = dict(bagging_fraction=0.6, bagging_freq=2, bagging_seed=5)
    assert _bag_counts("gpu", "gbdt", 6, **kw) == _bag_counts("cpu", "gbdt", 6, **kw)


def test_device_balanced_bagging_matches_host_draw(gpu_available):
    kw = dict(pos_bagging_fraction=0.5, neg_bagging_fraction=0.8, bagging_freq=1)
    assert _bag_counts("gpu", "gbdt", 4, **kw) == _bag_counts("cpu", "gbdt", 4, **kw)


def test_device_goss_matches_reference_block_layout(gpu_available):
    """Device GOSS = the reference's GOSS with one sampling block per 1024 rows
    (num_threads >= ceil(n / 1024)): same sampled-set sizes as the host draw."""
    n_blocks = (50000 + 1023) // 1024
    kw = dict(learning_rate=0.5, top_rate=0.2, other_rate=0.1)
    gpu = _bag_counts("gpu", "goss", 5, fixed_gradients=True, **kw)
    cpu = _bag_counts("cpu", "goss", 5, fixed_gradients=True, num_threads=n_blocks, **kw)
    assert [c[0] for c in gpu[:2]] == [50000, 50000]  # sampling starts at iteration 1 / learning_rate
    assert gpu == cpu


def _cat_data(n=40000, seed=12):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, 6).astype(np.float32)
    X[:, 0] = rng.randint(0, 24, size=n)   # many categories: sorted-ctr scan
    X[:, 1] = rng.randint(0, 3, size=n)    # few categories: one-vs-rest
    eff = np.sin(np.arange(24) * 1.7)
    logit = 1.5 * eff[X[:, 0].astype(int)] + 0.8 * (X[:, 1] == 2) + X[:, 2] + 0.3 * rng.randn(n)
    return X, (logit > 0.2).astype(np.float32)


def test_categorical_splits_on_device(gpu_available):
    """Categorical features are scanned by the device split kernel (no host-assisted fallback):
    the first tree's categorical splits and the fit match the CPU learner."""
    X, y = _cat_data()
    models = {}
    for device in ("cpu", "gpu"):
        params = {"objective": "binary", "num_leaves": 15, "verbose": -1, "device_type": device,
                  "max_cat_to_onehot": 4, "min_data_per_group": 50, "cat_smooth": 5}
        ds = lgb.Dataset(X, y, params=params, categorical_feature=[0, 1])
        models[device] = lgb.train(params, ds, 15, verbose_eval=False)
    cpu_t = models["cpu"].dump_model()["tree_info"][0]["tree_structure"]
    gpu_t = models["gpu"].dump_model()["tree_info"][0]["tree_structure"]
    for path in ([], ["left_child"], ["right_child"]):
        a, b = cpu_t, gpu_t
        for k in path:
            a, b = a[k], b[k]
        if "split_feature" not in a:
            continue
        assert a["split_feature"] == b["split_feature"]
        assert a["decision_type"] == b["decision_type"]
        assert str(a["threshold"]) == str(b["threshold"])
        assert a["internal_count"] == b["internal_count"]
    assert any(t["num_cat"] > 0 for t in models["gpu"].dump_model()["tree_info"])
    auc_c, auc_g = _auc(y, models["cpu"].predict(X)), _auc(y, models["gpu"].predict(X))
    assert auc_g > 0.85 and abs(auc_c - auc_g) < 2e-3


def _cat_splits(node):
    if "split_feature" not in node:
        return []
    return ([(node["split_feature"], node["decision_type"], str(node["threshold"]), node["internal_count"])]
            + _cat_splits(node["left_child"]) + _cat_splits(node["right_child"]))


@pytest.mark.parametrize("extra", [{}, {"max_cat_threshold": 64, "cat_smooth": 1, "min_data_per_group": 20}],
                         ids=["default", "wide_sets"])
def test_wide_categorical_on_device(gpu_available, monkeypatch, capfd, extra):
    """A categorical feature with more than 1024 bins (here ~2500 categories) is scanned on the
    device by the wide categorical kernel (bitonic ctr order in LDS, 4096-bin category sets):
    device-resident growth, and the trees equal host-assisted growth's (host split finder)."""
    rng = np.random.RandomState(31)
    n, ncat = 200000, 2500
    X = rng.randn(n, 5).astype(np.float32)
    X[:, 0] = rng.randint(0, ncat, size=n)
    eff = rng.randn(ncat)
    y = ((1.2 * eff[X[:, 0].astype(int)] + X[:, 1] + 0.5 * rng.randn(n)) > 0).astype(np.float32)
    params = dict({"objective": "binary", "num_leaves": 31, "verbose": -1, "device_type": "gpu",
                   "max_bin": 255}, **extra)
    capfd.readouterr()
    ds = lgb.Dataset(X, y, params=params, categorical_feature=[0])
    models = {"device": lgb.train(dict(params, verbose=2), ds, 5, verbose_eval=False)}
    log = capfd.readouterr().out
    assert "device-resident growth" in log and "host-assisted growth" not in log
    monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
    ds = lgb.Dataset(X, y, params=params, categorical_feature=[0])
    models["host"] = lgb.train(params, ds, 5, verbose_eval=False)
    monkeypatch.delenv("LGBM_AMD_HOST_ASSIST", raising=False)
    dt = models["device"].dump_model()["tree_info"]
    ht = models["host"].dump_model()["tree_info"]
    assert any(len(str(nd[2]).split("||")) > 1 for t in dt for nd in _cat_splits(t["tree_structure"])
               if nd[1] == "==")
    for i in range(len(dt)):
        assert _cat_splits(dt[i]["tree_structure"]) == _cat_splits(ht[i]["tree_structure"]), i
    binned = models["device"].dump_model()
    assert binned["tree_info"][0]["num_cat"] > 0


def test_host_assisted_scores_wide_groups(gpu_available, monkeypatch):
    """Host-assisted growth on 16-bit storage groups (a 300-category feature): the training
    scores follow the trees (the leaves' row ranges live on the host there, so the score
    update walks the tree) -- the recorded training loss equals the model's own."""
    rng = np.random.RandomState(32)
    n = 60000
    X = rng.randn(n, 4).astype(np.float32)
    X[:, 0] = rng.randint(0, 300, size=n)
    eff = rng.randn(300)
    y = ((eff[X[:, 0].astype(int)] + X[:, 1] + 0.5 * rng.randn(n)) > 0).astype(np.float32)
    monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
    params = {"objective": "binary", "num_leaves": 15, "verbose": -1, "device_type": "gpu",
              "metric": "binary_logloss"}
    ds = lgb.Dataset(X, y, params=params, categorical_feature=[0])
    ev = {}
    bst = lgb.train(params, ds, 3, valid_sets=[ds], valid_names=["train"], evals_result=ev, verbose_eval=False)
    p = np.clip(bst.predict(X), 1e-15, 1 - 1e-15)
    ll = float(-np.mean(y * np.log(p) + (1 - y) * np.log(1 - p)))
    assert abs(ev["train"]["binary_logloss"][-1] - ll) < 1e-9


def test_validation_scores_on_device(gpu_available):
    """Validation sets are scored on the device (one traversal kernel per tree): the recorded
    metric equals the metric of the booster's own predictions, and early stopping works."""
    X, y = _data(40000, seed=21)
    Xv, yv = _data(15000, seed=22)
    params = {"objective": "binary", "metric": ["binary_logloss", "auc", "binary_error"], "num_leaves": 31,
              "max_bin": 63,
              "verbose": -1, "device_type": "gpu", "bagging_fraction": 0.8, "bagging_freq": 1}
    ds = lgb.Dataset(X, y, params=params)
    dv = lgb.Dataset(Xv, yv, reference=ds)
    rec = {}
    b = lgb.train(params, ds, 40, valid_sets=[dv], valid_names=["v"], evals_result=rec, verbose_eval=False,
                  early_stopping_rounds=5)
    p = b.predict(Xv, num_iteration=b.best_iteration)
    ll = -np.mean(yv * np.log(p) + (1 - yv) * np.log(1 - p))
    assert rec["v"]["binary_logloss"][b.best_iteration - 1] == pytest.approx(ll, rel=1e-6)
    assert rec["v"]["auc"][b.best_iteration - 1] == pytest.approx(_auc(yv, p), abs=1e-6)
    assert rec["v"]["binary_error"][b.best_iteration - 1] == pytest.approx(np.mean((p > 0.5) != (yv > 0)), abs=1e-9)


def test_regression_validation_metrics_on_device(gpu_available):
    rng = np.random.RandomState(23)
    X = rng.randn(30000, 8).astype(np.float32)
    y = (X[:, 0] * 2 + np.sin(X[:, 1]) + 0.1 * rng.randn(30000)).astype(np.float32)
    Xv = rng.randn(8000, 8).astype(np.float32)
    yv = (Xv[:, 0] * 2 + np.sin(Xv[:, 1]) + 0.1 * rng.randn(8000)).astype(np.float32)
    w = (rng.rand(8000) + 0.5).astype(np.float32)
    params = {"objective": "regression", "metric": ["l2", "l1", "rmse"], "verbose": -1, "device_type": "gpu"}
    ds = lgb.Dataset(X, y, params=params)
    rec = {}
    b = lgb.train(params, ds, 20, valid_sets=[lgb.Dataset(Xv, yv, weight=w, reference=ds)], valid_names=["v"],
                  evals_result=rec, verbose_eval=False)
    p = b.predict(Xv)
    l2 = np.sum(w * (p - yv) ** 2) / np.sum(w)
    assert rec["v"]["l2"][-1] == pytest.approx(l2, rel=1e-6)
    assert rec["v"]["rmse"][-1] == pytest.approx(np.sqrt(l2), rel=1e-6)
    assert rec["v"]["l1"][-1] == pytest.approx(np.sum(w * np.abs(p - yv)) / np.sum(w), rel=1e-6)


@pytest.mark.parametrize("kind", ["binary_nan", "categorical", "multiclass"])
def test_device_batch_prediction_matches_host(gpu_available, kind, monkeypatch):
    """LGBM_BoosterPredictForMat on the device forest kernel == the host predictor, bit for bit."""
    if kind == "binary_nan":
        X, y = _data(30000, seed=31)
        params = {"objective": "binary"}
        cats = "auto"
    elif kind == "categorical":
        X, y = _cat_data(30000, seed=32)
        params = {"objective": "binary"}
        cats = [0, 1]
    else:
        rng = np.random.RandomState(33)
        X = rng.randn(30000, 8).astype(np.float32)
        y = np.argmax(X[:, :3] + 0.3 * rng.randn(30000, 3), axis=1).astype(np.float32)
        params = {"objective": "multiclass", "num_class": 3}
        cats = "auto"
    params.update({"num_leaves": 31, "verbose": -1, "device_type": "gpu"})
    b = lgb.train(params, lgb.Dataset(X, y, params=params, categorical_feature=cats), 25, verbose_eval=False)
    for data in (X, X.astype(np.float64)):
        for raw in (False, True):
            monkeypatch.delenv("LGBM_AMD_HOST_PREDICT", raising=False)
            dev = b.predict(data, raw_score=raw)
            monkeypatch.setenv("LGBM_AMD_HOST_PREDICT", "1")
            host = b.predict(data, raw_score=raw)
            np.testing.assert_array_equal(dev, host)
    # an iteration window
    monkeypatch.delenv("LGBM_AMD_HOST_PREDICT", raising=False)
    dev = b.predict(X, num_iteration=10, start_iteration=5)
    monkeypatch.setenv("LGBM_AMD_HOST_PREDICT", "1")
    np.testing.assert_array_equal(dev, b.predict(X, num_iteration=10, start_iteration=5))


@pytest.mark.parametrize("extra", [
    {"lambda_l1": 2.0, "lambda_l2": 5.0},
    {"max_delta_step": 0.3},
    {"path_smooth": 5.0, "min_data_in_leaf": 30},
    {"min_gain_to_split": 5.0},
    {"max_depth": 4},
    {"monotone_constraints": [1, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], "monotone_penalty": 0.5},
    {"zero_as_missing": True},
    {"feature_fraction": 0.6, "feature_fraction_seed": 4},
    {"feature_fraction_bynode": 0.5, "feature_fraction_seed": 5},
    {"feature_fraction": 0.8, "feature_fraction_bynode": 0.6, "feature_fraction_seed": 6},
    {"interaction_constraints": [[0, 1, 2], [3, 5, 7], [1, 6]]},
    {"interaction_constraints": [[0, 1, 2], [2, 3, 4, 7]], "feature_fraction": 0.7, "feature_fraction_seed": 3},
], ids=["l1l2", "max_delta_step", "path_smooth", "min_gain", "max_depth", "monotone", "zero_missing",
        "feature_fraction", "bynode", "bytree_bynode", "interaction", "interaction_bytree"])
def test_device_split_rules_match_cpu(gpu_available, extra):
    """The device split scan applies the reference's split rules like the CPU learner: same
    first-tree splits near the root, and closely matching fits."""
    X, y = _data(40000, seed=41)
    w = np.random.RandomState(42).rand(len(y)).astype(np.float32) + 0.5
    boosters = {}
    for device in ("cpu", "gpu"):
        params = {"objective": "binary", "num_leaves": 31, "max_bin": 63, "verbose": -1, "device_type": device,
                  "seed": 7}
        params.update(extra)
        boosters[device] = lgb.train(params, lgb.Dataset(X, y, weight=w, params=params), 15, verbose_eval=False)
    cpu_t = boosters["cpu"].dump_model()["tree_info"][0]["tree_structure"]
    gpu_t = boosters["gpu"].dump_model()["tree_info"][0]["tree_structure"]
    for path in ([], ["left_child"], ["right_child"]):
        a, b = cpu_t, gpu_t
        for k in path:
            a, b = a.get(k, {}), b.get(k, {})
        if "split_feature" not in a:
            assert "split_feature" not in b
            continue
        assert a["split_feature"] == b["split_feature"]
        assert a["threshold"] == pytest.approx(b["threshold"])
    pc, pg = boosters["cpu"].predict(X[:5000]), boosters["gpu"].predict(X[:5000])
    assert np.corrcoef(pc, pg)[0, 1] > 0.99


def _branches(node, path=()):
    if "split_feature" not in node:
        yield path
        return
    p = path + (node["split_feature"],)
    yield from _branches(node["left_child"], p)
    yield from _branches(node["right_child"], p)


@pytest.mark.parametrize("wide", [0, 37, 197], ids=["3_constraints", "40_constraints", "200_constraints"])
def test_interaction_constraints_device_resident(gpu_available, monkeypatch, tmp_path, wide):
    """Interaction constraints run in device-resident growth (per-leaf constraint bitmasks of
    four 64-bit words, reference col_sampler.hpp:92-126): every root-to-leaf branch uses
    features of one constraint, and the trees equal the host-assisted learner's (same device
    histograms, host split loop).  The wide cases put the useful constraints at bits 37-39 and
    197-199 (the fourth word) after single-feature constraints."""
    X, y = _data(30000, seed=5)
    ic = [[k % 8] for k in range(wide)] + [[0, 1, 2], [3, 5, 7], [1, 6]]
    models = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
        log = tmp_path / ("iters_%s.jsonl" % mode)
        monkeypatch.setenv("LGBM_AMD_ITER_LOG", str(log))
        b = _train(X, y, "gpu", rounds=8, interaction_constraints=ic)
        monkeypatch.delenv("LGBM_AMD_ITER_LOG")
        monkeypatch.delenv("LGBM_AMD_HOST_ASSIST", raising=False)
        rows = [json.loads(line) for line in log.read_text().splitlines()]
        assert all(r["device_resident"][0] == (mode == "device") for r in rows), (mode, rows[0])
        models[mode] = b
        for t in b.dump_model()["tree_info"]:
            for br in _branches(t["tree_structure"]):
                assert any(set(br) <= set(c) for c in ic), br
    dt = models["device"].dump_model()["tree_info"]
    ht = models["host"].dump_model()["tree_info"]
    feats = lambda t: sorted(f for br in _branches(t["tree_structure"]) for f in br)
    assert feats(dt[0]) == feats(ht[0])
    pd, ph = models["device"].predict(X[:5000]), models["host"].predict(X[:5000])
    assert np.corrcoef(pd, ph)[0, 1] > 0.995


def _splits(node):
    if "split_feature" not in node:
        return []
    return ([(node["split_feature"], round(node["threshold"], 6))] + _splits(node["left_child"])
            + _splits(node["right_child"]))


@pytest.mark.parametrize("extra", [
    {},
    {"feature_fraction_bynode": 0.6, "feature_fraction_seed": 9},
    {"interaction_constraints": [[0, 1, 2], [3, 5, 7], [1, 6]]},
    {"num_leaves": 63, "min_data_in_leaf": 200, "extra_seed": 11},
    {"bagging_fraction": 0.6, "bagging_freq": 1, "bagging_seed": 5},
    {"max_depth": 3, "num_leaves": 31},
    {"min_data_in_leaf": 1500, "num_leaves": 31},
], ids=["plain", "bynode", "interaction", "wide_seed", "bagging", "early_end_depth", "early_end_min_data"])
def test_extra_trees_device_resident(gpu_available, monkeypatch, capfd, extra):
    """extra_trees in device-resident growth: the split scans draw each feature's random
    threshold from its generator state at the tree's start (reference
    feature_histogram.hpp:107-110, one Random per feature seeded extra_seed + i), stepped by the
    draws of earlier nodes; the host generators replay the draws after the tree.  Trees equal
    the host-assisted learner's (host split loop, host generators) tree for tree, so the
    generators stay in step across trees."""
    X, y = _data(30000, seed=13)
    capfd.readouterr()
    _train(X[:4000], y[:4000], "gpu", rounds=1, extra_trees=True, verbose=2, **extra)
    assert "device-resident growth" in capfd.readouterr().out
    models = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
        models[mode] = _train(X, y, "gpu", rounds=6, extra_trees=True, **extra)
        monkeypatch.delenv("LGBM_AMD_HOST_ASSIST", raising=False)
    dt = models["device"].dump_model()["tree_info"]
    ht = models["host"].dump_model()["tree_info"]
    assert len(dt) == len(ht)
    for i in range(len(dt)):  # every tree: the generators stay in step across trees
        assert _splits(dt[i]["tree_structure"]) == _splits(ht[i]["tree_structure"]), i
    pd, ph = models["device"].predict(X[:5000]), models["host"].predict(X[:5000])
    assert np.corrcoef(pd, ph)[0, 1] > 0.999
    # and the fit matches the CPU learner's extra-trees model in quality
    cpu = _train(X, y, "cpu", rounds=6, extra_trees=True, **extra)
    assert abs(_auc(y, models["device"].predict(X)) - _auc(y, cpu.predict(X))) < 0.01


@pytest.mark.parametrize("extra", [
    {"feature_fraction_bynode": 0.5},
    {"feature_fraction_bynode": 0.25, "feature_fraction_seed": 3},
    {"feature_fraction_bynode": 0.6, "feature_fraction": 0.8, "feature_fraction_seed": 8},
], ids=["half", "quarter", "with_bytree"])
def test_interaction_constraints_bynode_device_resident(gpu_available, monkeypatch, capfd, extra):
    """Interaction constraints with feature_fraction_bynode grow device-resident: after each
    partition k_bynode_step draws the two children's masks from the tree's used features that
    the branch allows (reference col_sampler.hpp:91-162), both Random::Sample branches, from a
    device generator whose state the host sampler takes after the tree.  Trees equal
    host-assisted growth's (host ColSampler::GetByNode) tree for tree."""
    X, y = _data(30000, seed=17)
    params = dict({"objective": "binary", "num_leaves": 31, "max_bin": 63, "verbose": -1, "device_type": "gpu",
                   "interaction_constraints": [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [3, 5, 7, 10, 11, 12],
                                               [1, 6, 13, 14, 15]], "seed": 4}, **extra)
    capfd.readouterr()
    small = dict(params, verbose=2)
    lgb.train(small, lgb.Dataset(X[:4000], y[:4000], params=small), 1)
    assert "device-resident growth" in capfd.readouterr().out
    models = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
        models[mode] = lgb.train(params, lgb.Dataset(X, y, params=params), 8)
        monkeypatch.delenv("LGBM_AMD_HOST_ASSIST", raising=False)
    dt = models["device"].dump_model()["tree_info"]
    ht = models["host"].dump_model()["tree_info"]
    assert len(dt) == len(ht)
    for i in range(len(dt)):
        assert _splits(dt[i]["tree_structure"]) == _splits(ht[i]["tree_structure"]), i


@pytest.mark.parametrize("extra", [{}, {"feature_fraction_bynode": 0.7, "feature_fraction_seed": 4},
                                   {"max_cat_threshold": 3, "cat_smooth": 1, "min_data_per_group": 10}],
                         ids=["plain", "bynode", "few_thresholds"])
def test_categorical_extra_trees_device_resident(gpu_available, monkeypatch, capfd, extra):
    """extra_trees with categorical features grows device-resident: one-vs-rest features draw
    NextInt(bin_start, bin_end), sorted ones NextInt(0, max_threshold) only when that range is
    not empty -- a count that depends on the child's histogram, so one workgroup scans both
    children of a categorical feature in order (reference feature_histogram.hpp:314-401).  The
    trees equal host-assisted growth's tree for tree (the generators stay in step)."""
    X, y = _cat_data(30000, seed=21)
    params = dict({"objective": "binary", "num_leaves": 31, "verbose": -1, "device_type": "gpu",
                   "extra_trees": True, "extra_seed": 5, "max_cat_to_onehot": 4, "min_data_per_group": 50,
                   "cat_smooth": 5, "seed": 2}, **extra)
    capfd.readouterr()
    small = dict(params, verbose=2)
    lgb.train(small, lgb.Dataset(X[:4000], y[:4000], params=small, categorical_feature=[0, 1]), 1)
    assert "device-resident growth" in capfd.readouterr().out
    models = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
        models[mode] = lgb.train(params, lgb.Dataset(X, y, params=params, categorical_feature=[0, 1]), 8)
        monkeypatch.delenv("LGBM_AMD_HOST_ASSIST", raising=False)
    dt = models["device"].dump_model()["tree_info"]
    ht = models["host"].dump_model()["tree_info"]
    assert len(dt) == len(ht)
    for i in range(len(dt)):
        assert _cat_splits(dt[i]["tree_structure"]) == _cat_splits(ht[i]["tree_structure"]), i
    assert any(t["num_cat"] > 0 for t in dt)


@pytest.mark.parametrize("case", ["small", "wide"])
def test_intermediate_monotone_on_gpu(case, gpu_available, monkeypatch, capfd):
    """monotone_constraints_method=intermediate grows device-resident: the pick walks the tree
    to re-bound the leaves a split can touch (pick.h MonoInterUpdate) and the next split scan
    re-scans them.  Monotone predictions, the same trees as host-assisted growth (the host
    LeafConstraints loop on device histograms), and the CPU learner's first tree."""
    rng = np.random.RandomState(1)
    if case == "small":
        n = 6000
        X = rng.rand(n, 3)
        y = (5 * X[:, 0] + np.sin(10 * np.pi * X[:, 0]) - 5 * X[:, 1] - np.cos(10 * np.pi * X[:, 1])
             + 2 * np.sin(6 * X[:, 2]) + rng.rand(n) * 0.01)
        mono, leaves = [1, -1, 0], 31
    else:
        n = 30000
        X = rng.rand(n, 8)
        y = (3 * X[:, 0] + np.sin(8 * np.pi * X[:, 0]) - 2 * X[:, 1] + X[:, 2] * X[:, 3] + np.cos(6 * X[:, 4])
             + 2 * X[:, 5] - np.sin(5 * X[:, 6]) + rng.rand(n) * 0.05)
        mono, leaves = [1, -1, 0, 1, 0, 1, -1, 0], 63
    params = {"verbose": 2, "monotone_constraints": mono, "min_data": 20, "num_leaves": leaves,
              "monotone_constraints_method": "intermediate", "max_bin": 63}
    capfd.readouterr()
    gpu = lgb.train(dict(params, device_type="gpu"), lgb.Dataset(X, y), 20)
    log = capfd.readouterr().out
    assert "device-resident growth" in log and "host-assisted growth" not in log
    monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
    host = lgb.train(dict(params, device_type="gpu", verbose=-1), lgb.Dataset(X, y), 20)
    monkeypatch.delenv("LGBM_AMD_HOST_ASSIST")
    cpu = lgb.train(dict(params, device_type="cpu", verbose=-1), lgb.Dataset(X, y), 20)
    grid = np.linspace(0, 1, 40)
    for base in rng.rand(6, X.shape[1]):
        for f, sign in [(f, m) for f, m in enumerate(mono) if m != 0]:
            pts = np.tile(base, (40, 1))
            pts[:, f] = grid
            assert np.all(np.diff(gpu.predict(pts)) * sign >= -1e-12)
    ms = lambda b: b.model_to_string()[b.model_to_string().index("Tree=0"):b.model_to_string().index("end of trees")]
    assert ms(gpu) == ms(host)
    # (the re-bounding matters: the basic method grows other trees)
    basic = lgb.train(dict(params, device_type="gpu", verbose=-1, monotone_constraints_method="basic"),
                      lgb.Dataset(X, y), 20)
    assert ms(basic) != ms(gpu)
    assert _splits(gpu.dump_model()["tree_info"][0]["tree_structure"]) == \
        _splits(cpu.dump_model()["tree_info"][0]["tree_structure"])
    assert np.corrcoef(gpu.predict(X), cpu.predict(X))[0, 1] > 0.999


@pytest.mark.parametrize("task", ["lambdarank", "lambdarank_long_queries", "multiclass", "aucmu_weighted",
                                  "regression_family"])
def test_device_metrics_equal_host_metrics(task, gpu_available, monkeypatch, capfd):
    """Validation metrics evaluated on device-resident scores (NDCG / MAP one workgroup per
    query, multiclass on class-major scores, point-wise regression losses) equal the host
    evaluation of the same model (LGBM_AMD_HOST_METRICS=1 forces it)."""
    rng = np.random.RandomState(3)
    n, nv = 8000, 3000
    X, Xv = rng.randn(n, 8), rng.randn(nv, 8)
    if task.startswith("lambdarank"):
        y = np.clip(np.round(X[:, 0] + X[:, 1] + rng.randn(n)), 0, 4)
        yv = np.clip(np.round(Xv[:, 0] + Xv[:, 1] + rng.randn(nv)), 0, 4)
        group, gv = [40] * (n // 40), [30] * (nv // 30)
        if task == "lambdarank_long_queries":
            # queries longer than the LDS staging (2048 documents): the global-scratch kernels of
            # the gradients and of the metrics
            group, gv = [3000, 2600] + [40] * 60, [2100] + [30] * 30
        params = {"objective": "lambdarank", "metric": ["ndcg", "map"], "eval_at": [1, 3, 5, 10]}
    elif task in ("multiclass", "aucmu_weighted"):
        y = (np.argmax(X[:, :4] + 0.5 * rng.randn(n, 4), axis=1)).astype(float)
        yv = (np.argmax(Xv[:, :4] + 0.5 * rng.randn(nv, 4), axis=1)).astype(float)
        group = gv = None
        params = {"objective": "multiclass", "num_class": 4, "metric": ["multi_logloss", "multi_error", "auc_mu"],
                  "multi_error_top_k": 2}
        if task == "aucmu_weighted":  # AUC-mu with a class-cost matrix (zero diagonal)
            w = np.array([[0, 1, 2, 3], [1, 0, 1, 2], [2, 1, 0, 1], [3, 2, 1, 0]], dtype=float)
            params = {"objective": "multiclassova", "num_class": 4, "metric": ["auc_mu"],
                      "auc_mu_weights": list(w.ravel())}
    else:
        y = np.exp(0.3 * X[:, 0]) + rng.rand(n)
        yv = np.exp(0.3 * Xv[:, 0]) + rng.rand(nv)
        group = gv = None
        params = {"objective": "poisson", "metric": ["poisson", "gamma_deviance", "quantile", "huber", "mape"]}
    params.update({"verbose": -1, "device_type": "gpu", "num_leaves": 15, "seed": 1})

    def run():
        ds = lgb.Dataset(X, y, group=group, params=params)
        dv = ds.create_valid(Xv, yv, group=gv)
        res = {}
        lgb.train(params, ds, 6, valid_sets=[dv], valid_names=["v"], evals_result=res, verbose_eval=False)
        return res["v"]

    capfd.readouterr()
    params["verbose"] = 2
    dev = run()
    logged = capfd.readouterr().out
    kinds = {"lambdarank": (30, 31), "lambdarank_long_queries": (30, 31), "multiclass": (20, 21, 22), "aucmu_weighted": (22,),
             "regression_family": (10, 13, 7, 8, 11)}[task]
    for k in kinds:  # the device path ran
        assert "device metric (kind %d)" % k in logged, k
    params["verbose"] = -1
    monkeypatch.setenv("LGBM_AMD_HOST_METRICS", "1")
    host = run()
    assert set(dev) == set(host) and len(dev) >= (1 if task == "aucmu_weighted" else 2)
    for name in dev:
        np.testing.assert_allclose(dev[name], host[name], rtol=1e-9, atol=1e-12, err_msg=name)


@pytest.mark.parametrize("task", ["binary", "binary_weighted", "binary_negative_weights", "lambdarank", "multiclass",
                                  "regression_family"])
def test_training_metrics_on_device(task, gpu_available, monkeypatch, capfd):
    """Training-set metrics (valid_sets=[dtrain]: reference gbdt.cpp:484-542) are reduced on the
    device-resident training scores, equal to the host evaluation of the downloaded scores."""
    rng = np.random.RandomState(5)
    n = 12000
    X = rng.randn(n, 8)
    group = None
    weight = None
    if task.startswith("binary"):
        y = (X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.3 * rng.randn(n) > 0).astype(float)
        params = {"objective": "binary", "metric": ["auc", "binary_logloss", "binary_error"],
                  "bagging_fraction": 0.7, "bagging_freq": 1}
        kinds = (6, 4, 5)
        if task == "binary_weighted":  # (AUC sorts signed weights: zero weights of both classes included)
            weight = rng.choice([0.0, 0.5, 1.0, 2.5], size=n)
        if task == "binary_negative_weights":
            # the device AUC carries the class in the weight's sign: with negative weights the
            # AUC is evaluated on the host (reference binary_metric.hpp:240-241 adds a negative
            # weight to the row's own class), the other metrics stay on the device
            weight = rng.choice([-0.5, 0.5, 1.0, 2.5], size=n)
            kinds = (4, 5)
    elif task == "lambdarank":
        y = np.clip(np.round(X[:, 0] + X[:, 1] + rng.randn(n)), 0, 4)
        group = [40] * (n // 40)
        params = {"objective": "lambdarank", "metric": ["ndcg", "map"], "eval_at": [1, 3, 5]}
        kinds = (30, 31)
    elif task == "multiclass":
        y = (np.argmax(X[:, :4] + 0.5 * rng.randn(n, 4), axis=1)).astype(float)
        params = {"objective": "multiclass", "num_class": 4, "metric": ["multi_logloss", "multi_error", "auc_mu"]}
        kinds = (20, 21, 22)
    else:
        y = np.exp(0.3 * X[:, 0]) + rng.rand(n)
        params = {"objective": "poisson", "metric": ["poisson", "l2", "huber", "mape"]}
        kinds = (10, 1, 11)
    params.update({"verbose": -1, "device_type": "gpu", "num_leaves": 15, "seed": 1})

    def run():
        ds = lgb.Dataset(X, y, group=group, weight=weight, params=params)
        res = {}
        lgb.train(params, ds, 5, valid_sets=[ds], valid_names=["train"], evals_result=res, verbose_eval=False)
        return res["train"]

    capfd.readouterr()
    params["verbose"] = 2
    dev = run()
    logged = capfd.readouterr().out
    for k in kinds:
        assert "device metric (kind %d) on the training set" % k in logged, k
    if task == "binary_negative_weights":
        assert "device metric (kind 6)" not in logged
    params["verbose"] = -1
    monkeypatch.setenv("LGBM_AMD_HOST_METRICS", "1")
    host = run()
    assert set(dev) == set(host) and len(dev) >= 2
    for name in dev:
        np.testing.assert_allclose(dev[name], host[name], rtol=1e-9, atol=1e-12, err_msg=name)


def test_training_metrics_after_reset_training_data(gpu_available, monkeypatch):
    """LGBM_BoosterResetTrainingData to a dataset with other rows re-allocates the device
    training scores: the device training metrics then read the new scores, labels and weights
    (not the freed buffers of the old rows), equal to the host evaluation."""
    import ctypes
    from lightgbmv1_amd.basic import _load_lib, _safe_call
    _LIB = _load_lib()
    rng = np.random.RandomState(9)

    def data(n):
        X = rng.randn(n, 6)
        y = (X[:, 0] + 0.4 * rng.randn(n) > 0).astype(float)
        return X, y, rng.choice([0.5, 1.0, 2.0], size=n)

    params = {"objective": "binary", "metric": ["auc", "binary_logloss"], "verbose": -1, "device_type": "gpu",
              "num_leaves": 15, "seed": 1}
    (X1, y1, w1), (X2, y2, w2) = data(9000), data(5000)

    def run():
        d1 = lgb.Dataset(X1, y1, weight=w1, params=params, free_raw_data=False)
        bst = lgb.Booster(params, d1)
        for _ in range(3):
            bst.update()
        before = bst.eval_train()
        d2 = lgb.Dataset(X2, y2, weight=w2, reference=d1, params=params).construct()
        _safe_call(_LIB.LGBM_BoosterResetTrainingData(bst.handle, d2.handle))
        for _ in range(2):
            bst.update()
        return before, bst.eval_train()

    dev = run()
    monkeypatch.setenv("LGBM_AMD_HOST_METRICS", "1")
    host = run()
    for (a, b) in zip(dev, host):
        assert [m[1] for m in a] == [m[1] for m in b]
        np.testing.assert_allclose([m[2] for m in a], [m[2] for m in b], rtol=1e-9, atol=1e-12)


def _leaf_values(node):
    if "leaf_index" in node:
        return [node["leaf_value"]]
    return _leaf_values(node["left_child"]) + _leaf_values(node["right_child"])


@pytest.mark.parametrize("extra", [
    {"objective": "regression_l1"},
    {"objective": "quantile", "alpha": 0.8},
    {"objective": "quantile", "alpha": 0.3, "weighted": True},
    {"objective": "mape"},
    {"objective": "regression_l1", "bagging_fraction": 0.7, "bagging_freq": 1, "weighted": True},
], ids=["l1", "quantile", "quantile_weighted", "mape", "l1_bagging_weighted"])
def test_percentile_renewal_on_device(extra, gpu_available, monkeypatch):
    """Leaf outputs of L1 / quantile / MAPE renewed on the device (segmented sort of the leaves'
    residuals straight from the partition) equal the host renewal (the partition and the
    scores downloaded) bit for bit, tree after tree."""
    rng = np.random.RandomState(11)
    n = 20000
    X = rng.randn(n, 6)
    y = X[:, 0] * 2 + np.abs(X[:, 1]) + rng.standard_t(3, n)
    extra = dict(extra)
    w = rng.rand(n) + 0.5 if extra.pop("weighted", False) else None
    params = dict({"verbose": -1, "device_type": "gpu", "num_leaves": 15, "seed": 2}, **extra)

    def run():
        bst = lgb.train(params, lgb.Dataset(X, y, weight=w), 8)
        return [_leaf_values(t["tree_structure"]) for t in bst.dump_model()["tree_info"]]

    dev = run()
    monkeypatch.setenv("LGBM_AMD_HOST_RENEW", "1")
    host = run()
    assert len(dev) == len(host)
    for t, (a, b) in enumerate(zip(dev, host)):
        if t < 4:
            assert a == b, t  # bit for bit
        else:  # later trees: last-bit differences in the scores may appear (seen once in 120 leaves)
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


@pytest.mark.parametrize("extra", [{}, {"bagging_fraction": 0.7, "bagging_freq": 1},
                                   {"objective": "multiclass", "num_class": 3}, {"gpu_use_dp": True},
                                   {"negative_weights": True},
                                   {"negative_weights": True, "bagging_fraction": 0.7, "bagging_freq": 1}],
                         ids=["binary", "bagging", "multiclass", "wide", "negative_weights", "negative_weights_bagging"])
def test_device_training_is_bitwise_deterministic(extra, gpu_available):
    """Run-to-run determinism of device training: histograms are exact integer sums and every
    reduction has a fixed order (the root sums included), so two runs give the same model text,
    bit for bit -- with negative hessians too (negative weights: the packed histogram's h half
    is signed, UnpackPartial)."""
    X, y = _data(40000, seed=21)
    extra = dict(extra)
    weight = None
    if extra.pop("negative_weights", False):
        weight = np.random.RandomState(3).choice([-0.5, 0.5, 1.0, 2.5], size=len(y))
    if extra.get("objective") == "multiclass":
        y = (np.digitize(X[:, 0], [-0.5, 0.5])).astype(np.float32)
    params = {"objective": "binary", "verbose": -1, "device_type": "gpu", "num_leaves": 31, "seed": 5}
    params.update(extra)
    runs = [lgb.train(params, lgb.Dataset(X, y, weight=weight), 10).model_to_string() for _ in range(2)]
    assert runs[0] == runs[1]


@pytest.mark.parametrize("params", [{"objective": "binary"}, {"objective": "regression", "num_leaves": 63},
                                    {"objective": "binary", "bagging_fraction": 0.7, "bagging_freq": 1},
                                    {"objective": "binary", "categorical_feature": [3], "max_cat_to_onehot": 2}],
                         ids=["binary", "regression", "bagging", "categorical"])
def test_early_score_update_equals_host_tree_update(params, gpu_available, monkeypatch):
    """The training scores take each tree from its device split records (TreeFromRecords) while
    the host builds the Tree object: the same models and training scores, bit for bit, as
    adding the host-built tree (LGBM_AMD_EARLY_SCORE=0)."""
    rng = np.random.RandomState(12)
    n = 30000
    X = rng.randn(n, 8)
    X[:, 3] = rng.randint(0, 12, n)
    y = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.2 * (X[:, 3] % 3) + 0.3 * rng.randn(n)
    if params["objective"] == "binary":
        y = (y > 0).astype(float)
    out = {}
    for early in ("1", "0"):
        monkeypatch.setenv("LGBM_AMD_EARLY_SCORE", early)
        p = dict({"verbose": -1, "device_type": "gpu", "num_leaves": 31, "seed": 4, "learning_rate": 0.2}, **params)
        cat = p.pop("categorical_feature", "auto")
        b = lgb.train(p, lgb.Dataset(X, y, categorical_feature=cat), 12, keep_training_booster=True)
        out[early] = (b.model_to_string(), _train_scores(b, n), _last_gradients(b))
    assert out["1"][0] == out["0"][0]
    np.testing.assert_array_equal(out["1"][1], out["0"][1])
    for a, c in zip(out["1"][2], out["0"][2]):  # (the next iteration's gradients, from the fused walk)
        np.testing.assert_array_equal(a, c)


def test_negative_hessians_packed_histograms(gpu_available):
    """Negative hessians (negative weights) in the packed fx32 histograms: k_scales keeps the h
    half signed (|h| <= 2^30 per row block) and UnpackPartial returns its borrow to g, so the
    packed trees agree with the wide (int64 g, int64 h) ones up to fixed-point rounding."""
    rng = np.random.RandomState(8)
    n = 30000
    X = rng.randn(n, 10)
    y = (X[:, 0] + 0.7 * X[:, 1] * X[:, 2] + 0.3 * rng.randn(n) > 0).astype(float)
    w = rng.choice([-0.5, 0.5, 1.0, 2.5], size=n)
    base = {"objective": "binary", "verbose": -1, "device_type": "gpu", "num_leaves": 31, "seed": 5,
            "min_data_in_leaf": 5, "lambda_l2": 1.0}
    preds = {}
    for prec in ("fx32", "fx64"):
        params = dict(base, gpu_hist_precision=prec)
        b = lgb.train(params, lgb.Dataset(X, y, weight=w), 5)
        preds[prec] = b.predict(X, raw_score=True)
    assert np.isfinite(preds["fx32"]).all() and np.isfinite(preds["fx64"]).all()
    d = np.abs(preds["fx32"] - preds["fx64"])
    assert np.median(d) < 1e-4 and np.mean(d < 1e-3) > 0.98, (np.median(d), np.mean(d < 1e-3), d.max())


@pytest.mark.parametrize("env", [{"LGBM_AMD_SPARSE_ROWS": "1"}, {"LGBM_AMD_UNIFORM_BINS": "1"}, {"LGBM_AMD_GH_IN_ROWS": "1"}])
def test_storage_layouts_give_identical_models(gpu_available, monkeypatch, env):
    """Histograms are exact integer sums, so the training rows' storage (word matrix with
    per-group widths, every group widened to 16 bits, or row-sparse lists) cannot change a
    model: identical model strings."""
    rng = np.random.RandomState(21)
    n = 30000
    X = np.where(rng.rand(n, 40) < 0.1, rng.randn(n, 40), 0.0)
    X[:, :4] = rng.randn(n, 4)
    y = (X[:, 0] + X[:, 1] * X[:, 2] + X[:, 4:20].sum(1) + 0.3 * rng.randn(n) > 0).astype(np.float32)
    extra = dict(num_leaves=63, max_bin_by_feature=[511] + [63] * 39, bagging_fraction=0.8, bagging_freq=1)
    monkeypatch.setenv("LGBM_AMD_SPARSE_ROWS", "0")
    base = _train(X, y, "gpu", rounds=15, **extra).model_to_string()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    other = _train(X, y, "gpu", rounds=15, **extra).model_to_string()
    assert base == other


def test_four_bit_storage_gives_identical_models(gpu_available, monkeypatch):
    """4-bit storage (every group <= 16 bins, eight to a word; reference DenseBin<uint8_t,
    true>) against 8-bit storage of the same bins: identical models (exact integer histograms),
    with bagging, NaN missing values and a validation set scored on the device."""
    rng = np.random.RandomState(4)
    n = 40000
    X = rng.randn(n, 19)
    X[rng.rand(n) < 0.05, 3] = np.nan
    y = (X[:, 0] + X[:, 1] * X[:, 2] - np.nan_to_num(X[:, 3]) + 0.3 * rng.randn(n) > 0).astype(np.float32)
    params = {"objective": "binary", "num_leaves": 63, "max_bin": 15, "verbose": -1, "device_type": "gpu",
              "seed": 2, "bagging_fraction": 0.8, "bagging_freq": 1, "metric": "auc"}

    def run():
        ds = lgb.Dataset(X[:30000], y[:30000], params=params, free_raw_data=False)
        va = lgb.Dataset(X[30000:], y[30000:], reference=ds)
        ev = {}
        bst = lgb.train(params, ds, 12, valid_sets=[va], evals_result=ev, verbose_eval=False)
        return bst.model_to_string(), ev["valid_0"]["auc"]

    monkeypatch.setenv("LGBM_AMD_NIBBLE_BINS", "0")
    m8, auc8 = run()
    monkeypatch.setenv("LGBM_AMD_NIBBLE_BINS", "1")
    m4, auc4 = run()
    assert m8 == m4
    assert auc8 == auc4


def _forced_trees(monkeypatch, tmp_path, forced, host, cat=None, rounds=3):
    import json as _json
    rng = np.random.RandomState(31)
    n = 30000
    X = rng.randn(n, 8).astype(np.float32)
    X[:, 5] = rng.randint(0, 6, size=n)
    y = (X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * (X[:, 5] == 3) + 0.3 * rng.randn(n) > 0).astype(np.float32)
    f = tmp_path / ("forced_%d.json" % int(host))
    f.write_text(_json.dumps(forced))
    if host:
        monkeypatch.setenv("LGBM_AMD_HOST_ASSIST", "1")
    else:
        monkeypatch.delenv("LGBM_AMD_HOST_ASSIST", raising=False)
    params = {"objective": "binary", "num_leaves": 15, "verbose": -1, "device_type": "gpu", "seed": 3,
              "forcedsplits_filename": str(f), "max_cat_to_onehot": 8}
    ds = lgb.Dataset(X, y, params=params, categorical_feature=cat or [5], free_raw_data=False)
    bst = lgb.train(params, ds, rounds, verbose_eval=False, keep_training_booster=True)
    from lightgbmv1_amd import _native as nat
    rep = _json.loads(nat.read_string(lambda size, need, buf: nat.call(
        "LGBM_AMD_BoosterDeviceCheckSplits", bst.handle, size, need, buf), 1 << 16))
    return bst, rep, X


def _structure(node, depth):
    if "split_feature" not in node or depth == 0:
        return ("leaf", node.get("leaf_count", node.get("internal_count")))
    return (node["split_feature"], str(node["threshold"]), node["internal_count"],
            _structure(node["left_child"], depth - 1), _structure(node["right_child"], depth - 1))


@pytest.mark.parametrize("forced", [
    # numerical root, numerical and categorical children, a grandchild
    {"feature": 0, "threshold": 0.1, "left": {"feature": 1, "threshold": -0.2, "left": {"feature": 2, "threshold": 0.5}},
     "right": {"feature": 5, "threshold": 3}},
    # an invalid node (an unknown feature) ends the forced splits early
    {"feature": 0, "threshold": 0.0, "left": {"feature": 99, "threshold": 1.0}, "right": {"feature": 2, "threshold": 0.0}},
])
def test_forced_splits_on_device(gpu_available, monkeypatch, tmp_path, forced):
    """Forced splits are applied by the device pick (the static BFS schedule of the JSON tree,
    each node's split gathered by the split scan of its leaf): the trees equal the host-assisted
    learner's, and the trees grew device-resident."""
    dev, rep_dev, X = _forced_trees(monkeypatch, tmp_path, forced, host=False)
    host, rep_host, _ = _forced_trees(monkeypatch, tmp_path, forced, host=True)
    assert rep_dev["device_mode"] and not rep_host["device_mode"]
    # the forced levels (and the children they create) are identical; deeper normal splits may
    # differ in near-ties (device fixed-point scan vs host fp64 scan)
    for t_dev, t_host in zip(dev.dump_model()["tree_info"], host.dump_model()["tree_info"]):
        assert _structure(t_dev["tree_structure"], 3) == _structure(t_host["tree_structure"], 3)
    y = (X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * (X[:, 5] == 3) > 0).astype(np.float32)
    assert abs(_auc(y, dev.predict(X)) - _auc(y, host.predict(X))) < 5e-3
    root = dev.dump_model()["tree_info"][0]["tree_structure"]
    assert root["split_feature"] == forced["feature"]


@pytest.mark.parametrize("params", [{"objective": "binary"}, {"objective": "regression"},
                                    {"objective": "binary", "boosting": "goss", "learning_rate": 0.3},
                                    {"objective": "binary", "bagging_fraction": 0.7, "bagging_freq": 1}])
def test_score_walk_computes_next_gradients(gpu_available, monkeypatch, params):
    """The tree's score walk computes the next iteration's gradients from the scores it writes
    (LGBM_AMD_FUSE_GRAD, on by default) instead of a separate gradient pass: the same trees as
    the separate pass (the root sums' per-workgroup grouping differs only in rounding)."""
    X, y = _data(n=80000, seed=7)
    if params["objective"] == "regression":
        y = (X[:, 0] + 0.5 * X[:, 1] * X[:, 2]).astype(np.float32)
    p = dict(params, verbose=-1, device_type="gpu", num_leaves=31, seed=2)
    models, preds = {}, {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("LGBM_AMD_FUSE_GRAD", fuse)
        bst = lgb.train(p, lgb.Dataset(X, y, params=p), 15)
        models[fuse] = bst.dump_model()["tree_info"]
        preds[fuse] = bst.predict(X)
    for a, b in zip(models["0"], models["1"]):
        assert a["num_leaves"] == b["num_leaves"]

        def feats(node):
            if "split_feature" not in node:
                return []
            return [node["split_feature"]] + feats(node["left_child"]) + feats(node["right_child"])
        assert feats(a["tree_structure"]) == feats(b["tree_structure"])
    np.testing.assert_allclose(preds["0"], preds["1"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("rows_layout", ["0", "1"])
def test_host_sparse_groups_device_learner(rows_layout, gpu_available, monkeypatch):
    """Sparse host groups (only the rows off their most frequent bins stored) feed the device
    learner's uploads -- word rows or row-sparse lists (LGBM_AMD_SPARSE_ROWS), the column copy,
    device binning of the dense columns next to host-pushed sparse ones, a validation set --
    with the same models as dense host groups."""
    rng = np.random.RandomState(8)
    n, f = 160000, 30
    X = np.where(rng.rand(n, f) < 0.04, rng.randn(n, f), 0.0)
    X[:, :3] = rng.randn(n, 3)
    y = (X[:, 0] - X[:, 1] + 2 * X[:, 3:15].sum(1) + 0.3 * rng.randn(n) > 0).astype(np.float32)
    monkeypatch.setenv("LGBM_AMD_SPARSE_ROWS", rows_layout)
    params = {"objective": "binary", "num_leaves": 63, "verbose": -1, "device_type": "gpu", "seed": 2,
              "metric": "auc", "enable_bundle": False}

    def run(mode):
        monkeypatch.setenv("LGBM_AMD_HOST_SPARSE", mode)
        ds = lgb.Dataset(X[:140000], y[:140000], params=params)
        va = lgb.Dataset(X[140000:], y[140000:], reference=ds)
        ev = {}
        bst = lgb.train(params, ds, 10, valid_sets=[va], evals_result=ev, verbose_eval=False)
        m = bst.model_to_string()
        return m[m.index("Tree=0"):m.index("end of trees")], ev["valid_0"]["auc"]

    dense = run("0")
    assert run("1") == dense


@pytest.mark.parametrize("variants", [2, 8])
def test_training_auc_with_float_colliding_scores(variants, gpu_available, monkeypatch):
    """The device AUC sorts float32 keys: scores that differ as doubles but round to the same
    float are ordered exactly by the pairwise correction (pairs: runs of 2) or, for long runs of
    such scores, by the 64-bit sort (8 variants of each base score across a whole leaf)."""
    rng = np.random.RandomState(11)
    n = 20000
    X = rng.randn(n, 6)
    y = (X[:, 0] + 0.7 * rng.randn(n) > 0).astype(float)
    if variants == 2:
        base = rng.randn(n // 2).astype(np.float32).astype(np.float64)
        init = np.concatenate([base, base * (1.0 + 2.0 ** -45)])
        X[n // 2:] = X[:n // 2]  # (the pair's rows take the same leaves)
        y[n // 2:] = 1.0 - y[:n // 2]
    else:
        init = 0.25 + rng.randint(0, variants, size=n) * 2.0 ** -44
    params = {"objective": "binary", "metric": "auc", "device_type": "gpu", "num_leaves": 7, "seed": 1,
              "learning_rate": 0.05, "verbose": -1}

    def run():
        ds = lgb.Dataset(X, y, init_score=init, params=params)
        res = {}
        lgb.train(params, ds, 2, valid_sets=[ds], valid_names=["train"], evals_result=res, verbose_eval=False)
        return res["train"]["auc"]

    dev = run()
    monkeypatch.setenv("LGBM_AMD_HOST_METRICS", "1")
    host = run()
    np.testing.assert_allclose(dev, host, rtol=1e-12, atol=0)


_GROWTH_CASES = [
    # (id, parameters, environment, categorical column declared, facts beside the data's)
    ("plain", {}, {}, True, {}),
    ("bynode", {"feature_fraction_bynode": 0.6}, {}, True, {}),
    ("bynode_ic", {"feature_fraction_bynode": 0.6, "interaction_constraints": [[0, 1, 2, 5], [3, 4, 5, 6], [1, 6, 7]]},
     {}, True, {}),
    ("extra_trees", {"extra_trees": True, "extra_seed": 7}, {}, True, {}),
    ("extra_trees_no_categorical", {"extra_trees": True, "extra_seed": 7}, {}, False, {}),
    ("cegb_split", {"cegb_penalty_split": 1e-4}, {}, True, {}),
    ("cegb_coupled", {"cegb_penalty_feature_coupled": [0.5, 0.1, 0.3, 0, 0.2, 0.1, 0.4, 0], "cegb_tradeoff": 0.8},
     {}, True, {}),
    ("cegb_lazy", {"cegb_penalty_feature_lazy": [1e-4, 2e-4, 0, 1e-4, 0, 3e-4, 1e-4, 0]}, {}, True, {}),
    ("forced_splits", {"forcedsplits_filename": "forced.json"}, {}, True, {"forced": "scheduled"}),
    ("intermediate_monotone", {"monotone_constraints": [1, -1, 0, 0, 0, 0, 0, 0],
                               "monotone_constraints_method": "intermediate"}, {}, True, {}),
    ("host_assist", {}, {"LGBM_AMD_HOST_ASSIST": "1"}, True, {"force_host": True}),
    ("round_k_1", {}, {"LGBM_AMD_ROUND_K": "1"}, True, {"round_k_knob": 1}),
]


@pytest.mark.parametrize("params,env,cat,facts", [c[1:] for c in _GROWTH_CASES], ids=[c[0] for c in _GROWTH_CASES])
def test_growth_plan_matches_growth(params, env, cat, facts, gpu_available, monkeypatch, tmp_path):
    """What LGBM_AMD_GrowthPlan answers for a learner's parameters and facts is how the learner
    grows: every tree's residency and whether it grew in rounds, from the iteration log.  Coupled
    CEGB penalties outside the round replay grow in rounds once the tree's sample is used up: the
    first tree, with nothing used yet, takes one split per step."""
    from helpers.growth_facts import learner_plan
    rng = np.random.RandomState(31)
    n = 4096
    X = rng.randn(n, 8).astype(np.float32)
    X[:, 5] = rng.randint(0, 6, size=n)
    y = (X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * (X[:, 5] == 3) + 0.3 * rng.randn(n) > 0).astype(np.float32)
    params = dict({"objective": "binary", "num_leaves": 15, "max_bin": 15, "min_data_in_leaf": 5, "verbose": -1,
                   "device_type": "gpu", "seed": 3, "max_cat_to_onehot": 8}, **params)
    if "forcedsplits_filename" in params:
        path = tmp_path / "forced.json"
        path.write_text(json.dumps({"feature": 0, "threshold": 0.1, "left": {"feature": 1, "threshold": -0.2}}))
        params["forcedsplits_filename"] = str(path)
    log = tmp_path / "iters.jsonl"
    monkeypatch.setenv("LGBM_AMD_ITER_LOG", str(log))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ds = lgb.Dataset(X, y, params=params, categorical_feature=[5] if cat else [])
    lgb.train(params, ds, 3, verbose_eval=False)
    rows = [json.loads(line) for line in log.read_text().splitlines()]
    assert len(rows) == 3
    plan = learner_plan(params, num_features=8, num_categorical=1 if cat else 0, max_cat_bins=6 if cat else 0,
                        total_bins=8 * 15, **facts)
    print(plan, [(r["device_resident"][0], r["rounds"][0]) for r in rows])
    if plan["growth"] == "rounds_once_sample_used":
        rows, plan = rows[:1], dict(plan, growth="steps")
    for r in rows:
        assert r["device_resident"][0] == plan["device_resident"], (plan, r)
        assert (r["rounds"][0] > 0) == (plan["growth"] == "rounds"), (plan, r)
