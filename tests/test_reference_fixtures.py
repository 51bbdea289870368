"""Parity with the reference package's own fixtures.

* ``test_pinned_bounds``: the reference's basic test (tests/python_package_test/test_basic.py:16-61)
  pins the model's lower / upper bound after 20 iterations on scikit-learn's breast-cancer split
  (random_state=2) to -2.9040190126976606 / 3.3182142872462883; also the save/load, text-file
  prediction and prediction early-stopping consistency of the same test.  The GPU variant runs
  the device learner with ``gpu_use_dp`` (wide int64 histograms), as the reference's test does.
* ``test_example_consistency``: the reference's test_consistency.py:67-131 over the bundled
  ``examples/*`` (binary with ``.weight``, multiclass, regression with ``.init``, lambdarank and
  xendcg with ``.query``): predictions from a matrix, from the text file and from the sklearn
  estimator agree, and a Dataset built from the file (side files loaded by name) matches the one
  built from arrays.  The example data are the copies in the repository (the
  ``example_data`` fixture of conftest.py unpacks them).
"""
import os

import numpy as np
import pytest

import lightgbmv1_amd as lgb

LOWER = -2.9040190126976606
UPPER = 3.3182142872462883

def _breast_cancer():
    sk_datasets = pytest.importorskip("sklearn.datasets")
    model_selection = pytest.importorskip("sklearn.model_selection")
    X, y = sk_datasets.load_breast_cancer(return_X_y=True)
    return model_selection.train_test_split(X, y, test_size=0.1, random_state=2)


def _pinned_bounds(tmp_path, extra):
    from sklearn.datasets import dump_svmlight_file
    X_train, X_test, y_train, y_test = _breast_cancer()
    train_data = lgb.Dataset(X_train, label=y_train)
    valid_data = train_data.create_valid(X_test, label=y_test)
    params = {"objective": "binary", "metric": "auc", "min_data": 10, "num_leaves": 15, "verbose": -1,
              "num_threads": 1, "max_bin": 255, "gpu_use_dp": True}
    params.update(extra)
    bst = lgb.Booster(params, train_data)
    bst.add_valid(valid_data, "valid_1")
    for _ in range(20):
        bst.update()
    assert bst.current_iteration() == 20
    assert bst.num_trees() == 20
    assert bst.num_model_per_iteration() == 1
    assert bst.lower_bound() == pytest.approx(LOWER, abs=1e-7)
    assert bst.upper_bound() == pytest.approx(UPPER, abs=1e-7)
    model = str(tmp_path / "model.txt")
    bst.save_model(model)
    pred_from_matr = bst.predict(X_test)
    fname = str(tmp_path / "test.svm")
    with open(fname, "wb") as f:
        dump_svmlight_file(X_test, y_test, f)
    np.testing.assert_allclose(pred_from_matr, bst.predict(fname))
    # the saved model predicts exactly the same
    bst2 = lgb.Booster(params, model_file=model)
    pred_from_model_file = bst2.predict(X_test)
    np.testing.assert_array_equal(pred_from_matr, pred_from_model_file)
    # prediction early stopping keeps the signs
    early = bst2.predict(X_test, pred_early_stop=True, pred_early_stop_freq=5, pred_early_stop_margin=1.5)
    np.testing.assert_array_equal(np.sign(pred_from_matr), np.sign(early))
    # the feature count is checked
    with pytest.raises(lgb.basic.LightGBMError, match="The number of features in data"):
        bst2.predict(X_test[:, 1:])


def test_pinned_bounds(tmp_path):
    _pinned_bounds(tmp_path, {})


@pytest.mark.gpu
def test_pinned_bounds_device(tmp_path, gpu_available):
    _pinned_bounds(tmp_path, {"device_type": "gpu"})


class _Example:
    """The reference's FileLoader: an example directory's train.conf as parameters."""

    def __init__(self, root, directory, prefix):
        self.directory = os.path.join(root, directory)
        self.prefix = prefix
        self.params = {"gpu_use_dp": True, "verbose": -1}
        with open(os.path.join(self.directory, "train.conf")) as f:
            for line in f:
                line = line.strip()
                if line and not line.startswith("#"):
                    key, value = [t.strip() for t in line.split("=")]
                    if "early_stopping" not in key:
                        self.params[key] = value if key != "num_trees" else int(value)
        # (file names in the config are relative to the example directory)
        for key in ("data", "valid_data", "output_model", "machine_list_file", "forcedsplits_filename",
                    "forcedbins_filename", "input_model", "output_result"):
            if key in self.params:
                self.params[key] = os.path.join(self.directory, self.params[key])
        self.params.pop("output_model", None)

    def path(self, suffix):
        return os.path.join(self.directory, self.prefix + suffix)

    def load_dataset(self, suffix, is_sparse=False):
        fn = self.path(suffix)
        if is_sparse:
            from sklearn.datasets import load_svmlight_file
            X, y = load_svmlight_file(fn, dtype=np.float64, zero_based=True)
            return X, y, fn
        mat = np.loadtxt(fn, dtype=np.float64)
        return mat[:, 1:], mat[:, 0], fn

    def load_field(self, suffix):
        return np.loadtxt(self.path(suffix))

    def train_predict_check(self, lgb_train, X_test, X_test_fn, sk_pred):
        params = dict(self.params)
        params["force_row_wise"] = True
        gbm = lgb.train(params, lgb_train)
        y_pred = gbm.predict(X_test)
        np.testing.assert_allclose(y_pred, gbm.predict(X_test_fn))
        np.testing.assert_allclose(y_pred, sk_pred)

    def file_load_check(self, lgb_train, name):
        lgb_train_f = lgb.Dataset(self.path(name), params=self.params).construct()
        for f in ("num_data", "num_feature", "get_label", "get_weight", "get_init_score", "get_group"):
            a = getattr(lgb_train, f)()
            b = getattr(lgb_train_f, f)()
            if a is None and b is None:
                continue
            if a is None:
                assert np.all(np.asarray(b) == 1), f
            elif isinstance(b, (list, np.ndarray)):
                np.testing.assert_allclose(a, b)
            else:
                assert a == b, f


def _sk_params(fd):
    return {k: v for k, v in fd.params.items() if k not in ("data", "valid_data", "task")}


def test_example_binary(example_data):
    fd = _Example(example_data, "binary_classification", "binary")
    X_train, y_train, _ = fd.load_dataset(".train")
    X_test, _, X_test_fn = fd.load_dataset(".test")
    weight_train = fd.load_field(".train.weight")
    lgb_train = lgb.Dataset(X_train, y_train, params=fd.params, weight=weight_train)
    gbm = lgb.LGBMClassifier(**_sk_params(fd))
    gbm.fit(X_train, y_train, sample_weight=weight_train)
    sk_pred = gbm.predict_proba(X_test)[:, 1]
    fd.train_predict_check(lgb_train, X_test, X_test_fn, sk_pred)
    fd.file_load_check(lgb_train, ".train")


def test_example_multiclass(example_data):
    fd = _Example(example_data, "multiclass_classification", "multiclass")
    X_train, y_train, _ = fd.load_dataset(".train")
    X_test, _, X_test_fn = fd.load_dataset(".test")
    lgb_train = lgb.Dataset(X_train, y_train)
    gbm = lgb.LGBMClassifier(**_sk_params(fd))
    gbm.fit(X_train, y_train)
    sk_pred = gbm.predict_proba(X_test)
    fd.train_predict_check(lgb_train, X_test, X_test_fn, sk_pred)
    fd.file_load_check(lgb_train, ".train")


def test_example_regression(example_data):
    fd = _Example(example_data, "regression", "regression")
    X_train, y_train, _ = fd.load_dataset(".train")
    X_test, _, X_test_fn = fd.load_dataset(".test")
    init_score_train = fd.load_field(".train.init")
    lgb_train = lgb.Dataset(X_train, y_train, init_score=init_score_train)
    gbm = lgb.LGBMRegressor(**_sk_params(fd))
    gbm.fit(X_train, y_train, init_score=init_score_train)
    sk_pred = gbm.predict(X_test)
    fd.train_predict_check(lgb_train, X_test, X_test_fn, sk_pred)
    fd.file_load_check(lgb_train, ".train")


@pytest.mark.parametrize("example", ["lambdarank", "xendcg"])
def test_example_ranking(example, example_data):
    fd = _Example(example_data, example, "rank")
    X_train, y_train, _ = fd.load_dataset(".train", is_sparse=True)
    X_test, _, X_test_fn = fd.load_dataset(".test", is_sparse=True)
    group_train = fd.load_field(".train.query")
    lgb_train = lgb.Dataset(X_train, y_train, group=group_train)
    params = _sk_params(fd)
    if example == "lambdarank":
        params["force_col_wise"] = True
    gbm = lgb.LGBMRanker(**params)
    gbm.fit(X_train, y_train, group=group_train)
    sk_pred = gbm.predict(X_test)
    fd.train_predict_check(lgb_train, X_test, X_test_fn, sk_pred)
    fd.file_load_check(lgb_train, ".train")


@pytest.mark.gpu
@pytest.mark.parametrize("example", ["binary", "regression"])
def test_example_device(example, gpu_available, example_data):
    """The same consistency checks with the device learner (wide histograms, as the reference's
    GPU runs of these examples)."""
    if example == "binary":
        fd = _Example(example_data, "binary_classification", "binary")
        side = {"weight": fd.load_field(".train.weight")}
        est = lgb.LGBMClassifier
    else:
        fd = _Example(example_data, "regression", "regression")
        side = {"init_score": fd.load_field(".train.init")}
        est = lgb.LGBMRegressor
    fd.params["device_type"] = "gpu"
    X_train, y_train, _ = fd.load_dataset(".train")
    X_test, _, X_test_fn = fd.load_dataset(".test")
    lgb_train = lgb.Dataset(X_train, y_train, params=fd.params, **side)
    gbm = est(**_sk_params(fd))
    fit_side = {"sample_weight": side["weight"]} if "weight" in side else side
    gbm.fit(X_train, y_train, **fit_side)
    sk_pred = gbm.predict_proba(X_test)[:, 1] if example == "binary" else gbm.predict(X_test)
    fd.train_predict_check(lgb_train, X_test, X_test_fn, sk_pred)
    fd.file_load_check(lgb_train, ".train")
