"""The HIP split scans (FindNumericalBlock / FindCategoricalBlock of src/device/split_scan.h, run by
k_find and by k_round_find with k_round_childbest) against the rule of tests/helpers/split_ref.py,
on the hand-built cases of tests/helpers/split_cases.py.

Every case runs one split per step (LGBM_AMD_ROUND_K=1: k_find) and in round growth (=8), the
stored-bins width cases with gpu_use_dp as well.  Per run:

* the binning produced the meta the case intends, growth stayed on the device, and the round counts
  are those of the mode;
* the device's gradients sit exactly on its fixed-point grid (from the scales of
  LGBM_AMD_BoosterDeviceGradients) and equal the case's, so every histogram sum is exact;
* every leaf's rows are the rule's, and its raw histogram slot the rule's stored histogram;
* for every scanned leaf, the device's best-split record (the records of
  LGBM_AMD_BoosterDeviceCheckSplits) against the rule run on the histogram this test builds: feature,
  threshold, direction, counts and category set equal, the leaf's range, parent output and depth the
  rule's, and |gain_device - gain_rule| <= 32 * 2^-52 * mag, mag = |left gain| + |right gain| +
  |gain shift|.  Every partial sum is exact; what differs is a handful of roundings a term (the
  kEpsilon additions, the divisions, a possibly fused multiply-add in the gain), so 32 ulp of mag is a
  bound derived from the arithmetic, not a measurement.  Sums are held to 32 ulp of the leaf's sum of
  hessians (of the |gradients| it adds up): only the 1e-15 terms and the rebuilt bin round;
* the library's own check has no mismatch, and direction_ties only where the case makes both
  directions bit-equal;
* the model's applied splits and leaf values equal the rule's, as on the host.
"""
import ctypes
import json

import numpy as np
import pytest

import lightgbmv1_amd as lgb
from helpers import split_cases as C
from lightgbmv1_amd import _native as nat

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
RUNS = [(c.name, k, False) for c in C.CASES for k in (1, 8)] + [(c.name, k, True) for c in C.CASES if c.wide
                                                                 for k in (1, 8)]
_GROWN = {}


def _grown(case):
    if case.name not in _GROWN:
        _GROWN[case.name] = case.grow()
    return _GROWN[case.name]


def _gradients(bst, n):
    g = np.zeros(n, dtype=np.float32)
    h = np.zeros(n, dtype=np.float32)
    scales = np.zeros(2, dtype=np.float64)
    nat.call("LGBM_AMD_BoosterDeviceGradients", bst.handle, g.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
             h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), scales.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return g.astype(np.float64), h.astype(np.float64), scales


def _leaf_state(bst, leaf):
    cnt = ctypes.c_int(0)
    hlen = ctypes.c_int64(0)
    nat.call("LGBM_AMD_BoosterDeviceLeafState", bst.handle, ctypes.c_int(leaf), None, ctypes.byref(cnt), None,
             None, ctypes.byref(hlen), None)
    rows = np.zeros(cnt.value, dtype=np.int32)
    hist = np.zeros(hlen.value, dtype=np.int64)
    valid = np.zeros(hlen.value // 2, dtype=np.int8)
    sums = np.zeros(3, dtype=np.float64)
    nat.call("LGBM_AMD_BoosterDeviceLeafState", bst.handle, ctypes.c_int(leaf),
             rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(cnt),
             hist.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), valid.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
             ctypes.byref(hlen), sums.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return rows, hist.reshape(-1, 2), valid.astype(bool), sums


def _check_splits(bst):
    text = nat.read_string(lambda size, need, buf: nat.call("LGBM_AMD_BoosterDeviceCheckSplits", bst.handle, size,
                                                            need, buf), 1 << 16)
    return json.loads(text)


def _inf(v, sign):
    return sign * np.inf if v is None else v


def _compare(case, r, s, st, where, label):
    """a device best-split record r against the rule's split s of the leaf state st"""
    if s is None:
        assert r["feature"] < 0, where + (r,)
        return
    assert r["feature"] == s["inner"], where + (r["feature"], s["inner"])
    assert bool(r["is_categorical"]) == (s["cat_bins"] is not None), where
    if s["cat_bins"] is None:
        assert r["threshold"] == s["threshold"], where + (r["threshold"], s["threshold"])
        assert bool(r["default_left"]) == bool(s["default_left"]), where + ("default_left",)
    else:
        assert r["cat_bins"] == s["cat_bins"], where + (r["cat_bins"], s["cat_bins"])
    assert (r["left_count"], r["right_count"]) == (s["left_count"], s["right_count"]), where
    gscale = 32 * ULP * sum(abs(x) for x in case.g[st["rows"]])
    hscale = 32 * ULP * st["sum_h"]
    for key, tol in (("left_sum_gradient", gscale), ("right_sum_gradient", gscale), ("left_sum_hessian", hscale),
                     ("right_sum_hessian", hscale)):
        assert abs(r[key] - s[key]) <= tol, where + (key, r[key], s[key])
    for key in ("left_output", "right_output"):
        assert abs(r[key] - s[key]) <= 1e-12 * abs(s[key]), where + (key, r[key], s[key])
    multiple = abs(r["gain"] - s["gain"]) / (ULP * s["mag"])
    print("split-ulp %s %s: %.3f ulp of mag" % (case.family, label, multiple))
    assert multiple <= 32, where + ("gain", r["gain"], s["gain"], s["mag"], multiple)


@pytest.mark.parametrize("name,k,dp", RUNS, ids=["%s-k%d%s" % (n, k, "-dp" if dp else "") for n, k, dp in RUNS])
def test_device_scan_equals_the_rule(name, k, dp, gpu_available, monkeypatch, tmp_path):
    case = C.BY_NAME[name]
    grown = _grown(case)
    monkeypatch.setenv("LGBM_AMD_SPECULATE", "0")   # the hooks read the last tree's device state
    monkeypatch.setenv("LGBM_AMD_FUSE_GRAD", "0")   # ... and its gradients
    monkeypatch.setenv("LGBM_AMD_ROUND_K", str(k))
    log = tmp_path / "iters.jsonl"
    monkeypatch.setenv("LGBM_AMD_ITER_LOG", str(log))
    ds, params = C.dataset(case, device_type="gpu", **({"gpu_use_dp": True} if dp else {}))
    meta = C.feature_meta(ds)
    C.assert_meta(case, meta)
    bst = lgb.train(params, ds, 1, keep_training_booster=True)
    monkeypatch.delenv("LGBM_AMD_ITER_LOG")

    # growth mode
    rows = [json.loads(line) for line in log.read_text().splitlines()] if log.exists() else []
    splits = len(grown["nodes"])
    if splits == 0:
        assert rows == [] or rows[0]["leaves"] == [1], rows  # (a tree without a split ends the training)
    else:
        assert len(rows) == 1 and all(rows[0]["device_resident"]), rows
        assert rows[0]["leaves"] == [splits + 1], (rows, splits)
        assert (rows[0]["rounds"][0] > 0) == (k > 1), rows

    # the gradients are the case's, exactly on the device's grid
    n = len(case.g)
    g, h, scales = _gradients(bst, n)
    assert np.array_equal(g, case.g) and np.array_equal(h, case.h)
    for v, s in ((g, scales[0]), (h, scales[1])):
        assert np.array_equal(v * s, np.rint(v * s)) and np.all(np.abs(v * s) < 2.0 ** 52), (name, s)

    # leaves: rows and raw histogram slots
    for leaf, st in enumerate(grown["leaves"]):
        lrows, hist, valid, sums = _leaf_state(bst, leaf)
        assert sorted(lrows.tolist()) == st["rows"], (name, "rows of leaf", leaf)
        assert int(sums[2]) == st["n"]
        for f, m in enumerate(meta):
            ft = case.metas()[f]
            want = C.R.stored_histogram(case.bins, f, case.g, case.h, st["rows"], ft)
            for t in range(m["hist_size"]):
                if valid[m["hist_offset"] + t] and t != ft["most_freq_bin"] - ft["offset"]:
                    got = hist[m["hist_offset"] + t]
                    assert got[0] == want[t][0] * scales[0] and got[1] == want[t][1] * scales[1], (name, leaf, f, t)

    # the library's own check
    rep = _check_splits(bst)
    assert rep["device_mode"] and rep["mismatched"] == 0 and rep["gain_mismatch"] == 0, json.dumps(rep)[:2000]
    if not case.tie:
        assert rep["direction_ties"] == 0, rep["direction_ties"]

    # every scanned leaf's record against the rule
    final = {}
    for entry in grown["scanned"]:
        if entry["state"] is grown["leaves"][entry["leaf"]]:
            final[entry["leaf"]] = entry
    records = {r["leaf"]: r for r in rep["records"]}
    assert sorted(records) == sorted(final), (name, sorted(records), sorted(final))
    for leaf, entry in final.items():
        r, st, s = records[leaf], entry["state"], entry["split"]
        where = (name, "leaf", leaf)
        assert r["num_data"] == st["n"] and r["depth"] == st["depth"], where
        assert abs(r["sum_g"] - st["sum_g"]) <= 32 * ULP * sum(abs(x) for x in case.g[st["rows"]]), where
        assert abs(r["sum_h"] - st["sum_h"]) <= 32 * ULP * st["sum_h"], where
        assert abs(r["parent_output"] - st["output"]) <= 1e-12 * abs(st["output"]), where + (r["parent_output"], st["output"])
        for got, want in ((_inf(r["cmin"], -1), st["cmin"]), (_inf(r["cmax"], 1), st["cmax"])):
            assert got == want or abs(got - want) <= 1e-12 * abs(want), where + ("range", got, want)
        _compare(case, r, s, st, where, "%s k%d%s leaf %d" % (name, k, "-dp" if dp else "", leaf))

    # every applied split's record (the winner of the scan of the leaf it split) against the rule
    assert len(rep["applied"]) == len(grown["nodes"])
    for i, (r, nd) in enumerate(zip(rep["applied"], grown["nodes"])):
        assert r["leaf"] == nd["leaf"], (name, "split", i, r["leaf"], nd["leaf"])
        _compare(case, r, nd["split"], nd["state"], (name, "split", i),
                 "%s k%d%s split %d" % (name, k, "-dp" if dp else "", i))

    # the model's applied splits and leaf values
    C.check_booster(case, grown, bst, meta)
