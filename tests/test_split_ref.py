"""The split rule of tests/helpers/split_ref.py against the reference itself, on the hand-built
cases of tests/helpers/split_cases.py.  No GPU, and no reference at hand: the trees the reference's
command line program grew on the cases are fixtures (tests/golden/split_cases/, one file per family,
written by oracle/record_split_cases.py where the oracle is built).

Per case the rule's best-first growth must find in the recorded tree: split feature, threshold bin
(the recorded threshold separates the values of the threshold bin and the next), default direction,
category set and counts, equal; leaf values to 1e-12 relative; gain and internal values to the width
the model text gives them (%g of the float32 gain, six digits).  The digest of the case's rows must be
the recorded one: the dataset builder is deterministic.
"""
import json
import os

import pytest

from helpers import split_cases as C
from helpers import split_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_cases")


@pytest.fixture(scope="module")
def recorded():
    out = {}
    for family in C.FAMILIES:
        with open(os.path.join(GOLDEN, family + ".json")) as f:
            out.update(json.load(f))
    return out


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(C.NAMES)


@pytest.mark.parametrize("name", C.NAMES)
def test_rule_grows_the_reference_tree(name, recorded):
    case = C.BY_NAME[name]
    assert recorded[name]["digest"] == case.digest(), "the case's rows are not the recorded ones"
    grown = case.grow()
    root = grown["scanned"][0]["split"]
    if case.winner == "none":
        assert root is None
    elif case.winner is not None:
        assert root is not None and root["inner"] == case.winner, root
    C.check_tree(case, grown, recorded[name]["tree"], 1e-12)


def _root_candidates(case, f=0):
    leaf = case.grow()["scanned"][0]
    st = leaf["state"]
    _, _, cands = R.find_feature(leaf["hists"][f], case.metas()[f], case.rule_params(), st["sum_g"], st["sum_h"],
                                 st["n"], st["cmin"], st["cmax"], st["output"], st["depth"])
    return [c for c in cands if c["passed"]]


def test_tie_cases_are_ties_in_the_rule():
    """bit-equal gains in Python floats, where the case table says so"""
    best = {}
    for name in ("tie_reverse", "tie_reverse_rebuilt", "tie_reverse_k2", "tie_forward", "tie_directions", "tie_directions_mid",
                 "tie_directions_nan"):
        cands = _root_candidates(C.BY_NAME[name])
        top = max(c["gain"] for c in cands)
        best[name] = [(c["threshold"], c["reverse"]) for c in cands if c["gain"] == top]
    assert best["tie_reverse"] == [(1, True), (0, True)]
    assert best["tie_reverse_rebuilt"] == [(1, True), (0, True)]
    assert best["tie_reverse_k2"] == [(128, True), (127, True)]
    assert best["tie_forward"] == [(1, False), (2, False)]
    assert best["tie_directions"] == [(1, True), (1, False)]
    assert best["tie_directions_mid"] == [(1, True), (0, False)]
    assert best["tie_directions_nan"] == [(0, True), (0, False)]
    # two features, two leaves
    case = C.BY_NAME["tie_features"]
    leaf = case.grow()["scanned"][0]
    st = leaf["state"]
    gains = [R.find_feature(leaf["hists"][f], case.metas()[f], case.rule_params(), st["sum_g"], st["sum_h"], st["n"])[0]
             ["gain"] for f in (0, 1)]
    assert gains[0] == gains[1] and leaf["split"]["inner"] == 0
    scanned = C.BY_NAME["tie_leaves"].grow()["scanned"]
    assert [s["leaf"] for s in scanned][:3] == [0, 0, 1]
    assert scanned[1]["split"]["gain"] == scanned[2]["split"]["gain"] == 2.0
    assert [nd["leaf"] for nd in C.BY_NAME["tie_leaves"].grow()["nodes"]] == [0, 0, 1]


def test_only_the_direction_cases_are_marked_as_ties():
    assert sorted(c.name for c in C.CASES if c.tie) == ["tie_directions", "tie_directions_mid", "tie_directions_nan"]


def test_limit_cases_sit_on_their_limits():
    """the candidate on the limit: accepted at min_data_in_leaf / min_sum_hessian_in_leaf, rejected at
    min_gain_to_split (gain > shift), and gone one step past"""
    def root(name):
        return C.BY_NAME[name].grow()["scanned"][0]["split"]
    assert root("min_data_on")["threshold"] == 0 and root("min_data_on")["left_count"] == 50
    assert root("min_data_past")["threshold"] == 1
    assert root("min_hessian_on")["threshold"] == 0 and root("min_hessian_on")["left_sum_hessian"] == 50.0
    assert root("min_hessian_past")["threshold"] == 1
    assert root("min_gain_on") is None
    assert root("min_gain_past")["threshold"] == 0 and 0 < root("min_gain_past")["gain"] < 1e-11
    assert root("count_half_up")["left_count"] == 3 and root("count_half_up")["right_count"] == 93
    assert root("count_half_up_blocked") is None


def test_filter_cases_tell_their_candidate_counts_apart():
    """the set the rule finds with 1, 2 and 3 candidates after the cat_smooth filter: category 0; the
    outlier only the descending direction reaches; a set of two"""
    def bins(name):
        return C.BY_NAME[name].grow()["scanned"][0]["split"]["cat_bins"]
    assert bins("cat_filter_1") == [1] and bins("cat_filter_2") == [2] and bins("cat_filter_3") == [2, 3]
    assert len(bins("cat_filter_many")) > 2
