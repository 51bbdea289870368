"""The per-leaf path tables behind device SHAP contributions (src/boosting/shap_paths.cpp),
without a GPU: their host evaluator (LGBM_AMD_BoosterPathTableContrib, the kernel's arithmetic in
the kernel's order) against the recursive host predictor, Booster.predict(pred_contrib=True), on
the models of tests/helpers/contrib_cases.py at that module's tolerance."""
import numpy as np
import pytest

import lightgbmv1_amd as lgb

from helpers import contrib_cases as cc


@pytest.mark.parametrize("name", cc.CASES)
def test_path_tables_match_the_recursive_predictor(name):
    c = cc.case(name)
    X = c.X[:600]
    want = c.booster.predict(X, pred_contrib=True, **c.window)
    raw = c.booster.predict(X, raw_score=True, **c.window)
    got = cc.path_table_contrib(c.booster, X, c.start, c.num)
    assert got.shape == (600, c.num_class * (c.num_features + 1))
    cc.check_contrib(got, want.reshape(got.shape), raw, c, name)


def test_cases_have_the_shapes_they_are_meant_to():
    def leaves(c):
        return [t["num_leaves"] for t in c.booster.dump_model()["tree_info"]]

    assert max(leaves(cc.case("repeat3"))) == 31 and cc.case("repeat3").num_features == 3
    assert set(leaves(cc.case("stumps"))) == {2}
    assert set(leaves(cc.case("single_leaf"))) == {1}
    assert cc.case("multiclass3").num_class == 3
    assert len(leaves(cc.case("window"))) == 20
    assert "cat_threshold=" in cc.case("categorical_zero_missing").booster.model_to_string()


def test_unused_features_get_exactly_zero():
    c = cc.case("stumps")
    got = cc.path_table_contrib(c.booster, c.X[:50])
    used = set(np.nonzero(c.booster.feature_importance())[0])
    for f in range(c.num_features):
        if f not in used:
            assert np.all(got[:, f] == 0.0)


def test_path_tables_report_a_wrong_column_count():
    c = cc.case("stumps")
    with pytest.raises(Exception):
        cc.path_table_contrib(c.booster, c.X[:10, :3])


@pytest.mark.parametrize("k", [119, 120])
def test_long_chain_paths(k):
    """one tree whose deepest path has k distinct features, on rows for which the host recursion is
    still accurate (its contributions sum to its raw score within the bound)"""
    bst = lgb.Booster(model_str=cc.chain_model_text(k))
    X = cc.chain_rows(k, n=200)
    c = cc.Case(bst, X)
    want = bst.predict(X, pred_contrib=True)
    raw = bst.predict(X, raw_score=True)
    assert np.max(np.abs(want.sum(axis=1) - raw)) <= (k + 1) * cc.tolerance(bst)
    cc.check_contrib(cc.path_table_contrib(bst, X), want, raw, c, "chain of %d" % k)
