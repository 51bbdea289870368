"""The serial tail of a round -- each child's fold of its per-feature results (ChildBest,
src/device/round_find.hip) and the plan (src/device/round_plan.h) -- against one split per step.

The last split-scan workgroup of a child folds the child's per-feature records into its best
split; the winner's whole record travels with the fold (registers, then LDS) instead of being
loaded again, and the plan sizes the next round's row blocks beside composing its expansions.
Neither may change a tree: every case grows the same model text, byte for byte, with round
growth (LGBM_AMD_ROUND_K=8) and with one split per step (LGBM_AMD_ROUND_K=1).  The cases are the
ones in which a fold once published empty child bests: children that are not scanned
(min_data_in_leaf, max_depth), monotone constraints, lambda_l1, a categorical winner (its
category set is copied beside the record), exactly tied gains (a duplicated column: the smaller
real feature wins) and the device self check of every leaf's best split.  One case has more
features than a flat arrival counter takes (kRoundFlatMax = 128 split-scan workgroups per child),
so the two-level arrival runs.
"""
import functools
import json

import numpy as np
import pytest

import lightgbmv1_amd as lgb

pytestmark = pytest.mark.gpu

ROWS, FEATURES, TREES = 20000, 12, 4
FLAT_MAX = 128  # src/device/round_common.h kRoundFlatMax


@functools.lru_cache(maxsize=None)
def _data(features=FEATURES, tie=False):
    rng = np.random.RandomState(17)
    X = rng.randn(ROWS, features).astype(np.float32)
    X[:, 3] = np.abs(X[:, 3])
    X[rng.rand(ROWS) < 0.05, 5] = np.nan
    X[:, 6] = np.where(rng.rand(ROWS) < 0.6, 0.0, X[:, 6])
    X[:, 9] = rng.randint(0, 12, size=ROWS)  # (categorical in the case that names it)
    if tie:
        X[:, 11] = X[:, 0]  # the strongest column twice: every split on it ties with its copy
    logit = (X[:, 0] + 0.7 * X[:, 1] * X[:, 2] - 0.5 * X[:, 3] + 0.3 * np.nan_to_num(X[:, 5])
             + 0.6 * np.isin(X[:, 9], [1, 4, 7]))
    if features > FEATURES:
        logit = logit + 0.2 * X[:, FEATURES:].sum(1) / np.sqrt(features - FEATURES)
    y = (logit + 0.3 * rng.randn(ROWS) > 0).astype(np.float32)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _train(monkeypatch, k, X, y, params, keep=False):
    monkeypatch.setenv("LGBM_AMD_ROUND_K", str(k))
    p = {"objective": "binary", "verbose": -1, "device_type": "gpu", "seed": 11}
    p.update(params)
    cat = p.pop("_cat", None)
    ds = lgb.Dataset(X, y, params=p, categorical_feature=cat if cat is not None else "auto")
    return lgb.train(p, ds, TREES, keep_training_booster=keep)


CASES = {
    "plain": {},
    "min_data": {"min_data_in_leaf": 200},
    "monotone": {"monotone_constraints": [1, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 0], "monotone_constraints_method": "basic"},
    "lambda_l1": {"lambda_l1": 1.0},
    "categorical": {"_cat": [9]},
    "max_depth": {"max_depth": 4},
    "tied_gains": {},
    "self_check": {},
}


@pytest.mark.parametrize("max_bin", [63, 255])
@pytest.mark.parametrize("leaves", [31, 63])
@pytest.mark.parametrize("case", list(CASES))
def test_round_tail_equals_one_split_per_step(case, leaves, max_bin, monkeypatch, gpu_available):
    X, y = _data(tie=case == "tied_gains")
    params = dict(CASES[case], num_leaves=leaves, max_bin=max_bin)
    check = case == "self_check"
    if check:
        monkeypatch.setenv("LGBM_AMD_SPECULATE", "0")  # (the device must hold the last tree, not the next)
    base = _train(monkeypatch, 1, X, y, params).model_to_string()
    bst = _train(monkeypatch, 8, X, y, params, keep=check)
    spec = bst.model_to_string()
    assert spec.count("Tree=") == TREES
    if case == "tied_gains":
        # the tie is real: column 0 is split on and its copy, the larger real feature, never
        used = {int(f) for line in spec.splitlines() if line.startswith("split_feature=") for f in line[14:].split()}
        assert 0 in used and 11 not in used, sorted(used)
    assert base == spec
    if check:
        from lightgbmv1_amd import _native as nat
        res = json.loads(nat.read_string(lambda size, need, buf: nat.call(
            "LGBM_AMD_BoosterDeviceCheckSplits", bst.handle, size, need, buf), 1 << 16))
        assert res["device_mode"] and res["checked"] > 0
        assert res["mismatched"] == 0, res


def test_round_tail_two_level_arrival(monkeypatch, gpu_available):
    """More split-scan workgroups per child than one arrival counter takes: the sub-counters'
    last arriver folds the child."""
    X, y = _data(features=FLAT_MAX + 1)
    params = {"num_leaves": 31, "max_bin": 63}
    base = _train(monkeypatch, 1, X, y, params).model_to_string()
    spec = _train(monkeypatch, 8, X, y, params).model_to_string()
    assert base == spec
