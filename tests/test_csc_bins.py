"""The rule of the device binning of a CSC matrix (src/device/csc_bins.h), evaluated on the host
(LGBM_AMD_CscToGroupBins) against the Dataset the host path builds from the same raw arrays
(LGBM_DatasetCreateFromCSC with LGBM_AMD_DEVICE_BINNING=0: the matrix transposed into rows, every
row pushed; read back with LGBM_AMD_DatasetGetGroupBins) and against the rule of one CSR row
(LGBM_AMD_CsrToGroupBins) on a stable NumPy transposition: equal in every group without a
categorical member.  The edge matrix of tests/helpers/csc_bin_cases.py -- an empty column, one of
one entry, cells stored twice, descending and shuffled columns, a push-zeros column, two members
of one bundle on the same rows, columns past the reference's, and (against the rule alone) row
indices outside the matrix and a pointer past the entries -- with float32 / float64 values and
int32 / int64 pointers.  And the column-wise bin sample (LGBM_AMD_CSC_COLUMN_SAMPLE=1) against the
row-wise one.  Needs no GPU.
"""
import numpy as np
import pytest

from helpers import csc_bin_cases as cc
from helpers import csr_bin_cases as cb

SETTINGS = {
    "default": {},
    "no_missing": {"use_missing": False},
    "zero_as_missing": {"zero_as_missing": True},
    "categorical": {"categorical_feature": "9,14"},
    "no_bundle": {"enable_bundle": False},
}
N = 3000


@pytest.fixture(scope="module")
def cols():
    clean = cc.columns_of(cb.base_rows(N))
    edge, at = cc.edge_columns(clean, N)
    return clean, edge, at


@pytest.fixture(autouse=True)
def _host_binning(monkeypatch):
    monkeypatch.setenv("LGBM_AMD_DEVICE_BINNING", "0")
    monkeypatch.delenv("LGBM_AMD_CSC_COLUMN_SAMPLE", raising=False)


def _compare(ds, arrays, host_only_expected):
    host, bounds = ds.group_bins()
    rule = ds.eval_group_bins(*arrays, N)
    assert rule.shape == host.shape and host.shape[1] >= 2
    host_only = [g for g in range(host.shape[1]) if (rule[:, g] == -1).all()]
    assert (len(host_only) > 0) == host_only_expected, host_only
    for g in range(host.shape[1]):
        if g in host_only:
            continue
        bad = np.flatnonzero(host[:, g] != rule[:, g])
        assert bad.size == 0, (g, bad[:8], host[bad[:8], g], rule[bad[:8], g])
        assert host[:, g].min() >= 0 and host[:, g].max() < bounds[g + 1] - bounds[g]
    return host, rule


@pytest.mark.parametrize("ptype", [np.int32, np.int64], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("vtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_rule_matches_host_path(cols, setting, vtype, ptype):
    clean, edge, at = cols
    params = dict(cc.PARAMS, **SETTINGS[setting])
    train = cc.NativeCscDataset(*cc.flatten(clean, vtype, ptype), N, params)
    _compare(train, train.arrays, setting == "categorical")
    arrays = cc.flatten(edge, vtype, ptype)
    valid = cc.NativeCscDataset(*arrays, N, params, reference=train)  # (wider than its reference)
    host, rule = _compare(valid, arrays, setting == "categorical")
    # ... the rule of one CSR row on the stable transposition
    assert np.array_equal(rule, train.eval_csr_group_bins(*cc.to_csr(*arrays, N)))
    # rows -1 and num_row are dropped: the matrix without those entries
    bad = cc.flatten(cc.with_bad_rows(edge, N), vtype, ptype)
    assert len(bad[2]) == len(arrays[2]) + 4
    assert np.array_equal(train.eval_group_bins(*bad, N), rule)
    # a pointer past the entries is clamped to them
    over = arrays[0].copy()
    over[-1] += 7
    assert np.array_equal(train.eval_group_bins(over, arrays[1], arrays[2], N), rule)
    cut = len(arrays[2]) - 40
    short = train.eval_group_bins(arrays[0], arrays[1][:cut], arrays[2][:cut], N, nelem=cut)
    clamped = np.minimum(arrays[0], cut).astype(ptype)
    assert np.array_equal(short, train.eval_group_bins(clamped, arrays[1][:cut], arrays[2][:cut], N))
    assert np.array_equal(short, train.eval_csr_group_bins(*cc.to_csr(arrays[0], arrays[1][:cut], arrays[2][:cut], N)))
    if setting != "default":
        return
    # ---- the scenario is what the cases name
    assert host.shape[1] < cc.NCOL  # (EFB bundled something)

    def alone(c):
        """the rule on the edge matrix with every other column emptied"""
        return train.eval_group_bins(*cc.flatten([col if k == c else [] for k, col in enumerate(edge)], vtype, ptype), N)

    def group_of(c, bins):
        rows = [r for r, v in edge[c] if 0 <= r < N]
        g = np.flatnonzero((bins[rows] != none[rows]).any(axis=0))  # (none: the pushed zeros alone)
        assert g.size == 1, (c, g)
        return int(g[0])

    none, low, high = alone(23), alone(cc.LOW), alone(cc.HIGH)
    g = group_of(cc.LOW, low)
    assert g == group_of(cc.HIGH, high)  # one bundle holds both columns
    both = [r for r in at["both"] if low[r, g] != 0 and high[r, g] != 0]
    assert len(both) >= 8 and all(rule[r, g] == high[r, g] != low[r, g] for r in both)  # the higher column wins
    # cells stored twice in column 4: off the most frequent bin wins, 0 and NaN (-> 0.0) write nothing
    four = alone(4)
    first = train.eval_group_bins(*cc.flatten([col[:-3] if k == 4 else [] for k, col in enumerate(edge)], vtype, ptype), N)
    r_other, r_zero, r_nan = at["twice_4"]
    assert four[r_other, g] not in (0, first[r_other, g])
    assert four[r_zero, g] == first[r_zero, g] != 0 and four[r_nan, g] == first[r_nan, g] != 0
    # the push-zeros column: absent rows hold the pushed zero bin, stored zeros the same bin, the most
    # frequent value nothing; a second entry at the most frequent value leaves the first
    eight = alone(8)
    g8 = [k for k in range(rule.shape[1]) if eight[at["pz_absent"][0], k] != 0]
    assert len(g8) == 1
    zero_bin = eight[at["pz_absent"][0], g8[0]]
    assert (eight[at["pz_absent"], g8[0]] == zero_bin).all() and (eight[at["pz_stored_zero"], g8[0]] == zero_bin).all()
    mfv = [r for r, v in edge[8][:-4] if v == 1.0 and r not in at["twice_8"]]
    assert len(mfv) > 1000 and (eight[mfv, g8[0]] == 0).all()
    r_other, r_mfb, r_zero, r_nan = at["twice_8"]
    assert eight[r_other, g8[0]] not in (0, zero_bin)
    before = dict(edge[8][:-4])
    if before[r_mfb] != 1.0:
        assert eight[r_mfb, g8[0]] not in (0, zero_bin)  # (the first write survives)
    assert eight[r_zero, g8[0]] == zero_bin
    # the empty column and the one-entry column
    assert (none[:, g8[0]] == zero_bin).all() and (np.delete(none, g8[0], axis=1) == 0).all()
    one = alone(22)
    assert (one[5] != 0).sum() >= 1 and (one[[r for r in range(N) if r != 5]][:, group_of(22, one)] == 0).all()


@pytest.mark.parametrize("sample_cnt", [500, 100000], ids=["sample_below_rows", "sample_above_rows"])
@pytest.mark.parametrize("which", ["sorted", "edge"])
def test_column_sample_builds_the_same_dataset(monkeypatch, tmp_path, cols, which, sample_cnt):
    """the bin sample taken column by column (what the device path uses) against the one taken
    from the transposed rows: the same binary file, over sorted columns and over the edge matrix's
    descending / shuffled columns and cells stored twice"""
    clean, edge, _ = cols
    arrays = cc.flatten(clean if which == "sorted" else edge[:cc.NCOL], np.float64, np.int32)
    params = dict(cc.PARAMS, bin_construct_sample_cnt=sample_cnt)
    files = []
    for knob in (None, "1"):
        if knob is not None:
            monkeypatch.setenv("LGBM_AMD_CSC_COLUMN_SAMPLE", knob)
        before = cc.csc_stats()
        ds = cc.NativeCscDataset(*arrays, N, params)
        after = cc.csc_stats()
        assert after[0] == before[0] and after[1] - before[1] == (0 if knob is None else 1)
        files.append(ds.save(tmp_path / ("s_%s.bin" % knob)))
    assert len(files[0]) > 100 and files[0] == files[1]


def test_null_buffers_launch_info_and_stats_need_no_gpu(cols):
    import lightgbmv1_amd.ops as ops
    clean, _, _ = cols
    ds = cc.NativeCscDataset(*cc.flatten(clean), N, cc.PARAMS)
    assert ds.num_groups() >= 2  # (eval_group_bins asserts the count of the null-buffer call)
    info = ops.csc_bin_launch_info()
    assert info["segment_entries"] >= info["batch"] == 64 and info["tile_rows"] == 256
    assert info["max_push_zero_features"] >= 64
    assert min(cc.csc_stats()) >= 0
