"""The rule of one CSR row of the device binning (src/device/csr_bins.h), evaluated on the host
(LGBM_AMD_CsrToGroupBins) against the Dataset the host push builds from the same raw arrays
(LGBM_DatasetCreateFromCSR with LGBM_AMD_DEVICE_BINNING=0, read back with
LGBM_AMD_DatasetGetGroupBins): equal in every group without a categorical member.  The edge cases
of tests/helpers/csr_bin_cases.py -- an empty row, descending columns, a column stored twice,
two members of an EFB bundle in one row, columns past the end, stored 0.0 / 1e-36 / NaN under
every missing-value setting, values on bin bounds, the push-zeros column absent / present / at its
most frequent value, a bundle of 2-byte cells -- with float32 / float64 values and int32 / int64
indptr.  Needs no GPU.
"""
import numpy as np
import pytest

from helpers import csr_bin_cases as cb

SETTINGS = {
    "default": {},
    "no_missing": {"use_missing": False},
    "zero_as_missing": {"zero_as_missing": True},
    "no_bundle": {"enable_bundle": False},
    "categorical": {"categorical_feature": "9,14"},
    "max_bin_15": {"max_bin": 15, "min_data_in_bin": 3},
}


@pytest.fixture(scope="module")
def rows():
    clean = cb.base_rows()
    edge, at = cb.edge_rows(clean)
    return clean, edge, at


@pytest.fixture(autouse=True)
def _host_binning(monkeypatch):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")


def _compare(ds, arrays, host_only_expected):
    host, bounds = ds.group_bins()
    rule = ds.eval_group_bins(*arrays)
    assert rule.shape == host.shape and host.shape[1] >= 2
    host_only = [g for g in range(host.shape[1]) if (rule[:, g] == -1).all()]
    assert (len(host_only) > 0) == host_only_expected, host_only
    for g in range(host.shape[1]):
        if g in host_only:
            continue
        bad = np.flatnonzero(host[:, g] != rule[:, g])
        assert bad.size == 0, (g, bad[:8], host[bad[:8], g], rule[bad[:8], g])
        assert host[:, g].min() >= 0 and host[:, g].max() < bounds[g + 1] - bounds[g]
    return host, bounds, host_only


@pytest.mark.parametrize("ptype", [np.int32, np.int64], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("vtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_rule_matches_host_push_with_reference(rows, setting, vtype, ptype):
    """the edge rows binned with the mappers of a Dataset of the clean rows (reference=)"""
    clean, edge, at = rows
    params = dict(cb.PARAMS, **SETTINGS[setting])
    train = cb.NativeDataset(*cb.flatten(clean, vtype, ptype), cb.NCOL, params)
    arrays = cb.flatten(edge, vtype, ptype)
    valid = cb.NativeDataset(*arrays, cb.NCOL, params, reference=train)
    host, bounds, host_only = _compare(valid, arrays, setting == "categorical")
    _compare(train, train.arrays, setting == "categorical")
    if setting == "default":
        # the scenario is what the cases name: a bundle of 2-byte cells, and a group whose absent
        # rows hold a pushed zero bin while its most frequent value holds none
        widths = np.diff(bounds)
        assert widths.max() > 256 and host.shape[1] < cb.NCOL
        g = [g for g in range(host.shape[1]) if host[at["pz_absent"], g] != 0 and host[at["pz_most_frequent"], g] == 0
             and host[at["empty"], g] != 0]
        assert len(g) == 1
        assert host[at["pz_other"], g[0]] not in (0, host[at["pz_absent"], g[0]])
        assert host[at["pz_twice"], g[0]] == host[at["pz_other"], g[0]]
        assert host[at["pz_value_then_zero"], g[0]] == host[at["pz_absent"], g[0]]
        wide = int(np.argmax(widths))
        assert host[at["twice_second_mfb"], wide] != 0
        assert host[at["twice_second_wins"], wide] not in (0, host[at["twice_second_mfb"], wide])
        assert host[at["bundle_lower_last"], wide] != host[at["bundle_upper_last"], wide]
        assert host[at["bundle_second_mfb"], wide] == host[at["bundle_lower_last"], wide]


@pytest.mark.parametrize("ptype", [np.int32, np.int64], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("vtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("setting", ["default", "no_missing", "zero_as_missing"])
def test_rule_matches_host_push_without_reference(rows, setting, vtype, ptype):
    """the edge rows as the training matrix itself, declared with fewer columns than it stores:
    the column count grows while sampling, and the rule reads the dataset's num_total_features"""
    _, edge, _ = rows
    params = dict(cb.PARAMS, **SETTINGS[setting])
    arrays = cb.flatten(edge, vtype, ptype)
    ds = cb.NativeDataset(*arrays, 8, params)
    _compare(ds, arrays, False)


def test_null_buffers_return_the_group_count(rows):
    clean, _, _ = rows
    ds = cb.NativeDataset(*cb.flatten(clean), cb.NCOL, cb.PARAMS)
    assert ds.num_groups() >= 2  # (eval_group_bins asserts the count of the null-buffer call)
    ds.eval_group_bins(*cb.flatten(clean[:3]))


def test_launch_info_and_stats_need_no_gpu():
    import lightgbmv1_amd.ops as ops
    info = ops.csr_bin_launch_info()
    assert info["batch"] == 64 and info["tile_rows"] == 256 and info["rows_per_block"] >= 1
    assert info["max_push_zero_features"] >= 64
    dense, csr = cb.bin_stats()
    assert dense >= 0 and csr >= 0
