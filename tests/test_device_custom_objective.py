"""Custom objectives and metrics on GPU tensors (lightgbmv1_amd.on_device; kernels in
src/device/custom_kernels.hip, learner side in src/treelearner/gpu_learner_scores.cpp).

1. The two kernels through ops.cast_gradients / ops.convert_scores at the sizes where their
   launch changes (ops.custom_launch_info): every dtype bit-equal to tensor.to(float32), the
   transforms against the host evaluator within the bound of tests/helpers/convert_cases.py.
2. Transport does not change the model: objectives written in torch compute the same gradients on
   the GPU whether they get NumPy scores and return NumPy (unmarked) or get and return GPU tensors
   (marked); the models must be the same text for gbdt, bagging, GOSS and DART.
3. The scores tensor equals LGBM_BoosterGetPredict bit for bit at every iteration, after a
   rollback and after an update with a built-in objective.
4. A marked feval gets the converted scores the unmarked one gets, within the bound.
5. LGBM_AMD_DeviceCustomStats counts one export and one ingest per marked iteration.
6. Rejected inputs leave the booster usable; accepted odd ones (a non-contiguous view, NumPy from
   a marked callable) give the model of their plain form.
7. cv with a marked objective.

Where two training runs are compared, both come from this process and this build.
"""
import ctypes

import numpy as np
import pytest

import lightgbmv1_amd as lgb
import lightgbmv1_amd.ops  # noqa: F401  (lgb.ops)
from lightgbmv1_amd import _native as nat

from helpers import convert_cases as cc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, F, ITERS = 3000, 6, 10
DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]


@pytest.fixture(scope="module", autouse=True)
def _leave_the_device_as_found(gpu_available):
    """the tensors of the size cases are tens of megabytes each: give torch's cache (and the
    boosters still waiting for the collector) back before the next module runs in this process"""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 1. kernel sizes
@pytest.fixture(scope="module")
def info(gpu_available):
    return lgb.ops.custom_launch_info()


def _lens(info):
    per_trip = info["block"] * info["per_thread"]
    full = per_trip * info["max_grid"]  # elements of one loop trip of the largest grid
    return [1, 63, 64, 65, 255, 256, 257, per_trip - 1, per_trip + 1, full - 1, full, full + 1, 2 * full + 3]


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _gradient_values(n, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-6, 6, (n,), generator=g).double()
    if dtype == torch.float64:
        # beyond float32's range, its subnormals, ties of the rounding, signed zeros, NaN and +-inf
        sp = torch.tensor([3.5e38, -3.5e38, 1e300, -1e300, 3.4028235677973366e38, 1e-40, -1e-40, 1.4e-45, 7e-46, -7e-46,
                           1e-320, -0.0, 0.0, float("nan"), float("inf"), float("-inf"), 1.0 + 2.0 ** -24,
                           1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50], dtype=torch.float64)
    else:
        sp = torch.tensor([-0.0, 0.0, float("nan"), float("inf"), float("-inf"), 6e-8, -6e-8, 1e-40, 65504.0, 1e-5],
                          dtype=torch.float64)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    return x.to(dtype).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_cast_gradients_equals_torch_conversion_at_every_size(info, dtype):
    for n in _lens(info):
        g = _gradient_values(n, dtype, seed=n % 1000)
        h = torch.flip(g, dims=[0]).contiguous()
        og, oh = lgb.ops.cast_gradients(g, h)
        assert og.dtype == torch.float32 and og.shape == g.shape and og.device == g.device
        assert torch.equal(_bits32(og), _bits32(g.to(torch.float32))), (n, dtype)
        assert torch.equal(_bits32(oh), _bits32(h.to(torch.float32))), (n, dtype)


def test_cast_gradients_views_and_shapes(info):
    # an element-aligned view (storage offset 1) and a [3, n] tensor
    base = _gradient_values(1000, torch.float64, seed=4)
    g, h = base[1:], base[:-1]
    og, oh = lgb.ops.cast_gradients(g.contiguous(), h.contiguous())
    assert torch.equal(_bits32(og), _bits32(g.to(torch.float32)))
    g2 = _gradient_values(3 * 333, torch.float16, seed=5).reshape(3, 333)
    og2, _ = lgb.ops.cast_gradients(g2, g2)
    assert og2.shape == (3, 333) and torch.equal(_bits32(og2), _bits32(g2.to(torch.float32)))
    with pytest.raises(lgb.LightGBMError, match="dtype"):
        lgb.ops.cast_gradients(torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(lgb.LightGBMError, match="same dtype"):
        lgb.ops.cast_gradients(torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda"))


def _host_convert(kind, param, scores):
    s = np.ascontiguousarray(scores, dtype=np.float64)
    out = np.empty_like(s)
    nat.call("LGBM_AMD_ConvertScores", ctypes.c_int(kind), ctypes.c_double(param), ctypes.c_int(s.shape[0]),
             ctypes.c_int64(s.shape[1]), s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return out


def _scores(num_class, n, seed):
    """[num_class, n]: the edge columns of convert_cases first (as many as fit), then random"""
    rng = np.random.RandomState(seed)
    s = rng.normal(0, 4, size=(num_class, n))
    e = cc.edge_scores(num_class, n_random=0)
    k = min(n, e.shape[1])
    s[:, :k] = e[:, :k]
    return np.ascontiguousarray(s)


CONVERT_PARAMS = {
    0: ({"objective": "regression"}, 0.0),
    1: ({"objective": "binary", "sigmoid": 2.5}, 2.5),
    2: ({"objective": "regression", "reg_sqrt": True}, 0.0),
    3: ({"objective": "poisson"}, 0.0),
}


def _check_convert(params, kind, param, scores, what):
    t = torch.from_numpy(scores).cuda()
    one = scores.shape[0] == 1
    got = lgb.ops.convert_scores(params, t[0].contiguous() if one else t)
    assert got.dtype == torch.float64 and tuple(got.shape) == ((scores.shape[1],) if one else scores.shape)
    cc.assert_within_bound(got.cpu().numpy().reshape(scores.shape), _host_convert(kind, param, scores), kind,
                           scores.shape[0], what)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_convert_scores_single_class_at_every_size(info, kind):
    params, param = CONVERT_PARAMS[kind]
    for n in _lens(info):
        _check_convert(params, kind, param, _scores(1, n, seed=kind), "n=%d" % n)


@pytest.mark.parametrize("num_class", [3, 17])
def test_convert_scores_by_class(info, num_class):
    per_trip = info["block"] * info["per_thread"]
    # n is never a multiple of 64; the last makes every thread of the row kernel's largest grid loop
    sizes = [1, 63, 333, per_trip + 1] + ([info["block"] * info["max_grid"] + 77] if num_class == 3 else [4099])
    for n in sizes:
        s = _scores(num_class, n, seed=num_class)
        _check_convert({"objective": "multiclass", "num_class": num_class}, 4, 0.0, s, "softmax n=%d" % n)
        _check_convert({"objective": "multiclassova", "num_class": num_class, "sigmoid": 0.7}, 5, 0.7, s, "ova n=%d" % n)
        _check_convert({"objective": "none"}, 0, 0.0, s, "raw n=%d" % n)
    with pytest.raises(lgb.LightGBMError, match="scores per row"):
        lgb.ops.convert_scores({"objective": "multiclass", "num_class": num_class}, torch.zeros(5, dtype=torch.float64, device="cuda"))
    with pytest.raises(lgb.LightGBMError, match="no device kernel"):
        lgb.ops.convert_scores({"objective": "cross_entropy_lambda"}, torch.zeros(5, dtype=torch.float64, device="cuda"))


# ---------------------------------------------------------------- objectives written in torch
def _data(n=N, classes=0, seed=1):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, F)
    if classes:
        y = np.argmax(X[:, :classes] + 0.3 * rng.randn(n, classes), axis=1).astype(np.float64)
    else:
        y = (X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.2 * rng.randn(n) > 0).astype(np.float64)
    return X, y


def _grad_l2(p, y):
    return p - y, torch.ones_like(p)


def _grad_logloss(p, y):
    q = torch.sigmoid(p)
    return q - y, q * (1.0 - q)


def _grad_softmax(p, y):  # p [3, n], y [n] class ids
    q = torch.softmax(p, dim=0)
    onehot = torch.zeros_like(q).scatter_(0, y.long().unsqueeze(0), 1.0)
    return q - onehot, 2.0 * q * (1.0 - q)


OBJECTIVES = {"l2": (_grad_l2, 0), "logloss": (_grad_logloss, 0), "softmax": (_grad_softmax, 3)}


class _Objective:
    """One torch objective in both transports; the gradients are computed on the GPU, in float64,
    either way, and leave as `out_dtype`."""

    def __init__(self, name, y, out_dtype=torch.float32, shape="flat"):
        self.fn, self.classes = OBJECTIVES[name]
        self.y = torch.from_numpy(y).cuda()
        self.out_dtype = out_dtype
        self.shape = shape
        self.seen = []

    def _compute(self, p):
        k = max(1, self.classes)
        g, h = self.fn(p.reshape(k, -1) if k > 1 else p.reshape(-1), self.y)
        return g.to(self.out_dtype), h.to(self.out_dtype)

    def unmarked(self, preds, ds):
        assert isinstance(preds, np.ndarray)
        g, h = self._compute(torch.from_numpy(preds).cuda())
        return g.reshape(-1).cpu().numpy(), h.reshape(-1).cpu().numpy()

    def marked(self):
        @lgb.on_device
        def fobj(preds, ds):
            assert isinstance(preds, torch.Tensor) and preds.is_cuda and preds.dtype == torch.float64
            self.seen.append(tuple(preds.shape))
            g, h = self._compute(preds)
            if self.shape == "flat":
                return g.reshape(-1), h.reshape(-1)
            if self.shape == "transposed_view":  # a [k, n] view of [n, k] storage
                return g.t().contiguous().t(), h.t().contiguous().t()
            if self.shape == "numpy":
                return g.reshape(-1).cpu().numpy(), h.reshape(-1).cpu().numpy()
            return g, h
        return fobj


def _params(classes=0, **extra):
    p = {"objective": "none", "device_type": "gpu", "num_leaves": 7, "max_bin": 63, "min_data_in_leaf": 5,
         "verbose": -1, "seed": 2}
    if classes:
        p["num_class"] = classes
    p.update(extra)
    return p


def _train(name, fobj_of, iters=ITERS, n=N, **extra):
    classes = OBJECTIVES[name][1]
    X, y = _data(n, classes)
    params = _params(classes, **extra)
    booster = lgb.train(params, lgb.Dataset(X, y, params=params), iters, fobj=fobj_of(y), verbose_eval=False)
    assert booster.num_trees() == iters * max(1, classes)
    return booster.model_to_string()


VARIANTS = {
    "gbdt": {},
    "bagging": {"bagging_fraction": 0.6, "bagging_freq": 1},
    "goss": {"boosting": "goss", "learning_rate": 0.5},  # (sampling starts after 1 / learning_rate iterations)
    "dart": {"boosting": "dart"},
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(OBJECTIVES))
def test_transport_does_not_change_the_model(gpu_available, name, variant):
    extra = VARIANTS[variant]
    a = _train(name, lambda y: _Objective(name, y).unmarked, **extra)
    b = _train(name, lambda y: _Objective(name, y).marked(), **extra)
    assert a == b
    b64 = _train(name, lambda y: _Objective(name, y, out_dtype=torch.float64).marked(), **extra)
    assert b64 == b
    if OBJECTIVES[name][1]:
        assert _train(name, lambda y: _Objective(name, y, shape="matrix").marked(), **extra) == b


# ---------------------------------------------------------------- 3. the scores tensor
def _host_scores(booster, total):
    out = np.empty(total, dtype=np.float64)
    got = ctypes.c_int64(0)
    nat.call("LGBM_BoosterGetPredict", booster.handle, ctypes.c_int(0), ctypes.byref(got),
             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert got.value == total
    return out


def _same_bits(t, host):
    return np.array_equal(t.detach().cpu().numpy().reshape(-1).view(np.uint64), host.view(np.uint64))


@pytest.mark.parametrize("name", ["l2", "softmax"])
def test_scores_tensor_is_the_host_getter(gpu_available, name):
    fn, classes = OBJECTIVES[name]
    k = max(1, classes)
    X, y = _data(N, classes)
    params = _params(classes)
    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    dev = ctypes.c_int(-1)
    nat.call("LGBM_AMD_BoosterDeviceId", booster.handle, ctypes.byref(dev))
    assert dev.value >= 0
    obj = _Objective(name, y)
    inner = obj.marked()
    checked = []

    @lgb.on_device
    def fobj(preds, ds):
        assert preds.dtype == torch.float64 and preds.device == torch.device("cuda", dev.value)
        assert tuple(preds.shape) == ((N,) if k == 1 else (k, N))
        assert _same_bits(preds, _host_scores(booster, N * k))
        checked.append(preds.data_ptr())
        return inner(preds, ds)

    for _ in range(5):
        booster.update(fobj=fobj)
    assert len(checked) == 5 and len(set(checked)) == 1  # (one buffer, overwritten in place)
    t = booster.device_scores()
    assert t.data_ptr() == checked[0] and _same_bits(t, _host_scores(booster, N * k))
    assert booster.device_scores() is t  # (fresh: nothing is fetched again)
    before = t.clone()
    booster.rollback_one_iter()
    t2 = booster.device_scores()
    assert _same_bits(t2, _host_scores(booster, N * k)) and not torch.equal(t2, before)
    assert booster.current_iteration() == 4


def test_scores_tensor_after_a_built_in_update(gpu_available):
    X, y = _data()
    params = _params(objective="binary")
    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    raw0 = booster.device_scores(raw=True).clone()
    booster.update()
    raw1 = booster.device_scores(raw=True)
    assert not torch.equal(raw0, raw1)
    conv = booster.device_scores()
    host = _host_scores(booster, N)  # (converted by the host objective)
    cc.assert_within_bound(conv.cpu().numpy(), host, 1, 1, "binary scores")
    # the raw tensor is what the host transform started from
    assert np.array_equal(_host_convert(1, 1.0, raw1.cpu().numpy().reshape(1, -1)).reshape(-1).view(np.uint64),
                          host.view(np.uint64))
    # the NumPy cache is independent of the tensors
    seen = []
    booster.update(fobj=lambda preds, ds: (seen.append(type(preds)) or _Objective("logloss", y).unmarked(preds, ds)))
    assert seen == [np.ndarray]


# ---------------------------------------------------------------- 4. feval
def _binary_sets(n_valid=1001):
    X, y = _data()
    Xv, yv = _data(n_valid, seed=7)
    params = _params(objective="binary", learning_rate=0.3)
    train = lgb.Dataset(X, y, params=params)
    return params, train, lgb.Dataset(Xv, yv, reference=train), y, yv


def test_marked_feval_gets_the_converted_scores(gpu_available):
    got = {"marked": [], "plain": []}

    @lgb.on_device
    def feval_dev(preds, ds):
        assert isinstance(preds, torch.Tensor) and preds.is_cuda and preds.dtype == torch.float64
        assert tuple(preds.shape) == (ds.num_data(),)
        got["marked"].append(preds.cpu().numpy().copy())
        label = torch.from_numpy(ds.get_label()).to(preds.device)
        return "err", float(((preds > 0.5).double() != label.double()).double().mean().item()), False

    def feval_np(preds, ds):
        assert isinstance(preds, np.ndarray)
        got["plain"].append(preds.copy())
        return "err", float(np.mean((preds > 0.5) != (ds.get_label() > 0.5))), False

    best = {}
    for key, fe in (("marked", feval_dev), ("plain", feval_np)):
        params, train, valid, y, yv = _binary_sets()
        b = lgb.train(dict(params, metric="None"), train, 80, valid_sets=[train, valid], valid_names=["train", "valid"],
                      feval=fe, early_stopping_rounds=5, verbose_eval=False)
        best[key] = (b.best_iteration, b.current_iteration())
    print("early stopping (best iteration, iterations run):", best)
    assert best["marked"] == best["plain"]
    assert 0 < best["marked"][0] < 80  # (the validation error stopped improving: early stopping did stop)
    assert len(got["marked"]) == len(got["plain"]) > 2
    sizes = {a.shape[0] for a in got["marked"]}
    assert sizes == {N, 1001}  # (the training set and the validation set, every iteration)
    for a, b in zip(got["marked"], got["plain"]):
        cc.assert_within_bound(a, b, 1, 1, "feval scores")


def test_marked_feval_and_unmarked_feval_mix(gpu_available):
    params, train, valid, y, yv = _binary_sets()
    kinds = []

    @lgb.on_device
    def fe_dev(preds, ds):
        kinds.append("tensor" if isinstance(preds, torch.Tensor) else "numpy")
        return "d", float(preds.mean().item()), False

    def fe_np(preds, ds):
        kinds.append("tensor" if isinstance(preds, torch.Tensor) else "numpy")
        return "h", float(np.mean(preds)), False

    booster = lgb.Booster(params=params, train_set=train)
    booster.add_valid(valid, "valid")
    booster.update()
    res = booster.eval_valid([fe_dev, fe_np])
    assert kinds == ["tensor", "numpy"]
    vals = {m: v for _, m, v, _ in res}
    assert abs(vals["d"] - vals["h"]) <= 1e-12


def test_multiclass_feval_rows_sum_to_one(gpu_available):
    X, y = _data(N, 3)
    params = _params(3, objective="multiclass")
    rows = []

    @lgb.on_device
    def feval(preds, ds):
        assert tuple(preds.shape) == (3, N) and preds.dtype == torch.float64
        p = preds.cpu().numpy()
        rows.append((p[0] + p[1]) + p[2])
        return "m", 0.0, False

    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    for _ in range(3):
        booster.update()
        booster.eval_train(feval)
    assert len(rows) == 3
    for s in rows:
        assert np.max(np.abs(s - 1.0)) <= cc.softmax_row_sum_bound(3)
    host = _host_scores(booster, 3 * N)
    cc.assert_within_bound(booster.device_scores().cpu().numpy().reshape(-1), host, 4, 3, "multiclass scores")


# ---------------------------------------------------------------- 5. the device path ran
def _stats():
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    nat.call("LGBM_AMD_DeviceCustomStats", ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def test_device_path_is_counted(gpu_available):
    e0, i0 = _stats()
    _train("logloss", lambda y: _Objective("logloss", y).unmarked)
    assert _stats() == (e0, i0)
    _train("logloss", lambda y: _Objective("logloss", y).marked())
    assert _stats() == (e0 + ITERS, i0 + ITERS)
    _train("logloss", lambda y: _Objective("logloss", y, shape="numpy").marked())  # (scores exported, host gradients)
    assert _stats() == (e0 + 2 * ITERS, i0 + ITERS)


# ---------------------------------------------------------------- 6. errors and odd inputs
def _bad(what, n, k):
    g = torch.zeros(k * n, dtype=torch.float32, device="cuda")
    h = torch.ones(k * n, dtype=torch.float32, device="cuda")
    if what == "length":
        return g[:-1], h[:-1]
    if what == "lengths differ":
        return g, h[:-1]
    if what == "dtypes differ":
        return g, h.double()
    if what == "int32":
        return g.int(), h.int()
    if what == "[n, k]":
        return g.reshape(n, k), h.reshape(n, k)
    if what == "one on the host":
        return g, h.cpu()
    raise AssertionError(what)


@pytest.mark.parametrize("what,match", [("length", "gradient has shape"), ("lengths differ", "hessian has shape"),
                                        ("dtypes differ", "same dtype"), ("int32", "gradient has dtype"),
                                        ("[n, k]", "gradient has shape"), ("one on the host", "hessian must be a GPU tensor")])
def test_rejected_gradients_leave_the_booster_usable(gpu_available, what, match):
    X, y = _data(N, 3)
    params = _params(3)
    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    good = _Objective("softmax", y).marked()
    booster.update(fobj=good)
    before = booster.model_to_string()
    e0, i0 = _stats()
    with pytest.raises(ValueError, match=match):
        booster.update(fobj=lgb.on_device(lambda preds, ds: _bad(what, N, 3)))
    assert booster.model_to_string() == before and _stats()[1] == i0
    booster.update(fobj=good)
    assert booster.current_iteration() == 2


def test_gradients_on_another_device_are_rejected(gpu_available):
    if torch.cuda.device_count() < 2:
        return  # (one GPU: there is no other device to put a tensor on)
    X, y = _data()
    params = _params()
    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    other = torch.device("cuda", 1)
    with pytest.raises(ValueError, match="gradient is on"):
        booster.update(fobj=lgb.on_device(lambda preds, ds: (torch.zeros(N, device=other), torch.ones(N, device=other))))
    booster.update(fobj=_Objective("l2", y).marked())
    assert booster.current_iteration() == 1


def test_c_api_rejects_a_wrong_length(gpu_available):
    X, y = _data()
    params = _params()
    booster = lgb.Booster(params=params, train_set=lgb.Dataset(X, y, params=params))
    g = torch.zeros(N, dtype=torch.float32, device="cuda")
    fin = ctypes.c_int(0)
    torch.cuda.synchronize()
    for dtype, length, match in ((0, N - 1, "len is"), (7, N, "dtype 7")):
        with pytest.raises(lgb.LightGBMError, match=match):
            nat.call("LGBM_AMD_BoosterUpdateOneIterCustomDevice", booster.handle, ctypes.c_void_p(g.data_ptr()),
                     ctypes.c_void_p(g.data_ptr()), ctypes.c_int(dtype), ctypes.c_int64(length), ctypes.byref(fin))
    out = torch.empty(N + 1, dtype=torch.float64, device="cuda")
    with pytest.raises(lgb.LightGBMError, match="out_len"):
        nat.call("LGBM_AMD_BoosterGetPredictDevice", booster.handle, ctypes.c_int(0), ctypes.c_int(0),
                 ctypes.c_void_p(out.data_ptr()), ctypes.c_int64(N + 1))
    booster.update(fobj=_Objective("l2", y).marked())
    assert booster.current_iteration() == 1


def test_accepted_odd_inputs_give_the_plain_model(gpu_available):
    plain = _train("softmax", lambda y: _Objective("softmax", y, shape="matrix").marked())
    assert _train("softmax", lambda y: _Objective("softmax", y, shape="transposed_view").marked()) == plain
    assert _train("softmax", lambda y: _Objective("softmax", y, shape="numpy").marked()) == plain
    for dt in (torch.float16, torch.bfloat16):  # the same 16-bit values through either transport
        a = _train("logloss", lambda y: _Objective("logloss", y, out_dtype=dt).marked())

        def via_host(y, dt=dt):
            o = _Objective("logloss", y, out_dtype=dt)
            return lambda preds, ds: tuple(t.float().cpu().numpy() for t in o._compute(torch.from_numpy(preds).cuda()))
        assert a == _train("logloss", via_host)


# ---------------------------------------------------------------- 7. cv
def test_cv_with_a_marked_objective(gpu_available):
    n = 2000
    X, y = _data(n)

    def compute(p, ds):
        # a fold holds a subset of the rows: its labels come from the fold's own dataset
        yy = torch.from_numpy(np.asarray(ds.get_label(), dtype=np.float64)).to(p.device)
        q = torch.sigmoid(p)
        return (q - yy).float(), (q * (1.0 - q)).float()

    @lgb.on_device
    def marked(preds, ds):
        assert isinstance(preds, torch.Tensor) and preds.is_cuda
        return compute(preds, ds)

    def unmarked(preds, ds):
        g, h = compute(torch.from_numpy(preds).cuda(), ds)
        return g.cpu().numpy(), h.cpu().numpy()

    def feval(preds, ds):
        return "err", float(np.mean((preds > 0) != (ds.get_label() > 0.5))), False

    hist = {}
    e0, i0 = _stats()
    for key, fobj in (("marked", marked), ("unmarked", unmarked)):
        params = _params(metric="None")
        hist[key] = lgb.cv(params, lgb.Dataset(X, y, params=params), num_boost_round=5, nfold=2, stratified=False,
                           shuffle=False, fobj=fobj, feval=feval, verbose_eval=False)
    assert _stats()[1] == i0 + 2 * 5  # (two folds, five iterations, the marked run only)
    assert hist["marked"].keys() == hist["unmarked"].keys() and len(hist["marked"]["err-mean"]) == 5
    for k in hist["marked"]:
        assert hist["marked"][k] == hist["unmarked"][k], k
