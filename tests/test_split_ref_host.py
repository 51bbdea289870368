"""The host split finder (src/treelearner/split_finder.cpp, through the host learner) against the
rule of tests/helpers/split_ref.py, on the hand-built cases of tests/helpers/split_cases.py.  No GPU.

Per case: the binning produced the meta the case intends (LGBM_AMD_DatasetFeatureMeta); then the
tree that device_type=cpu grows must equal the rule's growth in split feature, threshold (the upper
bound of the rule's threshold bin), default direction, category set and counts; leaf values to 1e-12
and internal values to 1e-12 relative; gain to float32 rounding (both read from the tree in memory,
Booster.dump_model of the booster that trained).
"""
import pytest

import lightgbmv1_amd as lgb
from helpers import split_cases as C


@pytest.mark.parametrize("name", C.NAMES)
def test_host_finder_grows_the_rule_tree(name):
    case = C.BY_NAME[name]
    ds, params = C.dataset(case, device_type="cpu")
    meta = C.feature_meta(ds)
    C.assert_meta(case, meta)
    bst = lgb.train(params, ds, 1, keep_training_booster=True)
    C.check_booster(case, case.grow(), bst, meta)
