"""Hand-built histograms for the split scans, each expressed as a dataset.

Every case is an L2 regression with boost_from_average=false, one tree and learning_rate=1, so
g_i = -label_i * weight_i and h_i = weight_i: the reference's program, the host learner and the
device learner all see exactly the histogram the case designs.  Hessians come from {0.5, 1, 2}
and gradients are multiples of 2^-8 with |g| <= 8: label and product are exact in float32 and
every sum is exact in float64 and on the device's fixed-point grid.

A case is designed in bin space: a feature lists the raw value of each of its bins (every value
is its own bin: min_data_in_bin=1 and a max_bin that fits) and the meta the binning must produce;
the tests assert that meta (LGBM_AMD_DatasetFeatureMeta), so a case cannot degrade silently.
tests/helpers/split_ref.py is the rule the cases are judged by.
"""
import hashlib
import math

import numpy as np

from . import split_ref as R

NONE, ZERO, NAN = R.NONE, R.ZERO, R.NAN
NAN_VALUE = float("nan")


class Feat:
    """a feature in bin space: values[b] is the raw value of bin b (None: no row is designed there)"""

    def __init__(self, values, missing=NONE, default_bin=0, mfb=0, categorical=False, monotone=0, penalty=1.0):
        self.values = list(values)
        self.num_bin = len(self.values)
        self.missing, self.default_bin, self.mfb = missing, default_bin, mfb
        self.categorical, self.monotone, self.penalty = categorical, monotone, penalty

    def meta(self, real):
        return dict(num_bin=self.num_bin, missing_type=self.missing, default_bin=self.default_bin,
                    most_freq_bin=self.mfb, offset=1 if self.mfb == 0 else 0, categorical=self.categorical,
                    monotone=self.monotone, penalty=self.penalty, real=real)


class Case:
    def __init__(self, name, family, feats, bins, g, h, leaves=2, winner=0, tie=False, wide=False, **extra):
        self.name, self.family, self.feats = name, family, feats
        self.bins = np.asarray(bins, dtype=np.int32).reshape(len(g), len(feats))
        self.g = np.asarray(g, dtype=np.float64)
        self.h = np.asarray(h, dtype=np.float64)
        self.leaves = leaves
        self.winner = winner      # the inner feature of the root's split by design ("none": no split; None: unstated)
        self.tie = tie            # both scan directions are bit-equal by design (direction_ties tolerated)
        self.wide = wide          # a stored-bins width case: run with gpu_use_dp as well
        self.extra = extra        # training parameters beyond the common ones
        assert len(self.g) <= 8400 and len(self.g) == len(self.h)
        assert np.all(np.isin(self.h, (0.5, 1.0, 2.0)))
        assert np.all(self.g * 256 == np.rint(self.g * 256)) and np.all(np.abs(self.g) <= 8)
        for f, ft in enumerate(feats):
            assert self.bins[:, f].min() >= 0 and self.bins[:, f].max() < ft.num_bin
            cnt = np.bincount(self.bins[:, f], minlength=ft.num_bin)
            top = int(np.argmax(cnt))  # the binning's rule: the fullest bin if it holds 70 %, else the default bin
            assert ft.mfb == (top if top == ft.default_bin or cnt[top] >= 0.7 * len(self.g) else ft.default_bin), (name, f)
            assert all(ft.values[b] is not None for b in np.flatnonzero(cnt)), (name, f)

    # -- the dataset
    def X(self):
        X = np.zeros(self.bins.shape, dtype=np.float64)
        for f, ft in enumerate(self.feats):
            vals = np.array([NAN_VALUE if v is None else v for v in ft.values], dtype=np.float64)
            X[:, f] = vals[self.bins[:, f]]
        return X

    def label(self):
        y = -self.g / self.h
        assert np.all(y.astype(np.float32).astype(np.float64) == y)
        return y

    def weight(self):
        return self.h

    def categorical_features(self):
        return [f for f, ft in enumerate(self.feats) if ft.categorical]

    def train_params(self):
        p = {"objective": "regression", "boost_from_average": False, "learning_rate": 1.0, "num_leaves": self.leaves,
             "min_data_in_bin": 1, "min_data_in_leaf": 1, "min_sum_hessian_in_leaf": 1e-3, "feature_pre_filter": False,
             "enable_bundle": False, "max_bin_by_feature": [4 * ft.num_bin + 16 for ft in self.feats],
             "max_bin": max(4 * ft.num_bin + 16 for ft in self.feats), "verbose": -1, "num_threads": 1,
             "force_col_wise": True, "min_data_per_group": 1, "cat_smooth": 1.0, "cat_l2": 0.0,
             "max_cat_to_onehot": 4, "max_cat_threshold": 32}
        p.update(self.extra)
        if any(ft.monotone for ft in self.feats):
            p["monotone_constraints"] = [ft.monotone for ft in self.feats]
        if any(ft.penalty != 1.0 for ft in self.feats):
            p["feature_contri"] = [ft.penalty for ft in self.feats]
        return p

    # -- the rule's view
    def metas(self):
        return [ft.meta(f) for f, ft in enumerate(self.feats)]

    def rule_params(self):
        t = self.train_params()
        keys = ("lambda_l1", "lambda_l2", "max_delta_step", "path_smooth", "min_gain_to_split",
                "min_sum_hessian_in_leaf", "min_data_in_leaf", "cat_l2", "cat_smooth", "max_cat_threshold",
                "min_data_per_group", "max_cat_to_onehot", "monotone_penalty", "max_depth")
        kw = {k: t[k] for k in keys if k in t}
        return R.params(use_mc="monotone_constraints" in t, **kw)

    def grow(self):
        return R.grow(self.bins.tolist(), self.g.tolist(), self.h.tolist(), self.metas(), self.rule_params(),
                      self.leaves)

    def digest(self):
        m = hashlib.sha256()
        for a in (self.bins, self.g, self.h):
            m.update(np.ascontiguousarray(a).tobytes())
        m.update(repr([(ft.values, ft.missing, ft.default_bin, ft.mfb, ft.categorical) for ft in self.feats]).encode())
        m.update(repr(sorted(self.train_params().items())).encode())
        return m.hexdigest()[:24]


# ---------------------------------------------------------------------------------- builders

def rows_of(spec):
    """[(bin, g, h, count)] -> (bins, g, h) row arrays, in the order given"""
    b, g, h = [], [], []
    for bin_, gg, hh, cnt in spec:
        b += [bin_] * cnt
        g += [gg] * cnt
        h += [hh] * cnt
    return np.array(b), np.array(g, dtype=np.float64), np.array(h, dtype=np.float64)


def companion(n, k=3):
    """a narrow second feature that carries no signal to speak of: the row index modulo k (k >= 2
    bins, bin 0 the most frequent)"""
    c = np.arange(n) % k
    return c, Feat(list(range(k)))


def numeric(num_bin, zero_at=0, mfb=None, missing=NONE, nan=False, **kw):
    """a numerical feature of num_bin bins: consecutive integers with 0 in bin `zero_at` (the default
    bin), a NaN bin last if `nan`.  The most frequent bin is the default bin unless another holds 70 %
    of the rows (the binning's rule), which a case states with mfb"""
    values = list(range(-zero_at, num_bin - (1 if nan else 0) - zero_at)) + ([NAN_VALUE] if nan else [])
    return Feat(values, missing=missing, default_bin=zero_at, mfb=zero_at if mfb is None else mfb, **kw)


def step_rows(num_bin, split_after, seed, per_bin=3, skip=(), heavy=None, heavy_rows=0):
    """rows of one numerical feature over bins 0..num_bin-1: per_bin rows a bin (heavy_rows in the bin
    `heavy`), gradient +(1..1.25) up to bin `split_after` and -(1..1.25) above it, in steps of 2^-8,
    hessians cycling through {0.5, 1, 2}"""
    rng = np.random.RandomState(seed)
    spec = []
    hs = (0.5, 1.0, 2.0)
    for b in range(num_bin):
        if b in skip:
            continue
        for k in range(heavy_rows if b == heavy else per_bin):
            mag = 1.0 + rng.randint(0, 64) / 256.0
            spec.append((b, mag if b <= split_after else -mag, hs[(b + k) % 3], 1))
    return rows_of(spec)


def two_col(main_bins, comp):
    return np.stack([main_bins, comp], axis=1)


def cat3(*parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert c.name not in [x.name for x in CASES]
    CASES.append(c)
    return c


# ---- stored bins: one wave / 256 threads, K = 1 -> 2 -> 3, LDS-staged -> read from the slot
def _widths():
    for stored in (2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049):
        # odd widths store from bin 1 (the most frequent bin is 0), even ones rebuild a middle bin
        if stored % 2 == 1 or stored == 2:
            num_bin, zero_at = stored + 1, 0
        else:
            num_bin, zero_at = stored, stored // 2
        b, g, h = step_rows(num_bin, (num_bin * 5) // 8, seed=stored)
        comp, cf = companion(len(g))
        add("width_%d" % stored, "widths", [numeric(num_bin, zero_at), cf], two_col(b, comp), g, h, wide=True)


# ---- the most frequent bin at the places a thread's slice begins and ends
def _mfb():
    for name, num_bin, mfb in (("mfb_k2_first", 400, 200), ("mfb_k2_last", 400, 201), ("mfb_63", 100, 63),
                               ("mfb_64", 100, 64), ("mfb_last", 100, 99), ("mfb_zero", 40, 0),
                               ("mfb_first_stored", 40, 1)):
        b, g, h = step_rows(num_bin, num_bin // 2 + 3, seed=num_bin + mfb)
        comp, cf = companion(len(g))
        add(name, "mfb", [numeric(num_bin, mfb), cf], two_col(b, comp), g, h)
    # a dominant bin (80 % of the rows) that is not the default bin
    b, g, h = step_rows(10, 4, seed=70, heavy=6, heavy_rows=108)
    add("mfb_dominant", "mfb", [numeric(10, 0, mfb=6)], b, g, h)
    # ... and equal to the default bin under zero-as-missing: values -3..3, zero is bin 3
    b, g, h = step_rows(7, 4, seed=77)
    add("mfb_is_default", "mfb", [numeric(7, 3, missing=ZERO)], b, g, h, zero_as_missing=True)


# ---- missing types
def _missing():
    # zero as missing, the default bin first, in the middle and last, next to a dominant bin that is
    # rebuilt from the totals; the zero rows pull hard to one side
    for name, d, pull in (("zero_first", 0, -4.0), ("zero_middle", 5, 4.0), ("zero_last", 9, -4.0)):
        rows = cat3(step_rows(10, 4, seed=90 + d, skip=(d,), heavy=7, heavy_rows=96), rows_of([(d, pull, 1.0, 6)]))
        add(name, "missing", [numeric(10, d, mfb=7, missing=ZERO)], *rows, zero_as_missing=True)
    # NaN as missing: offset 0 and offset 1 (the forward scan starts from what is stored nowhere)
    for name, zero_at, pull in (("nan_offset0_right", 5, -4.0), ("nan_offset0_left", 5, 4.0),
                                ("nan_offset1_right", 0, -4.0), ("nan_offset1_left", 0, 4.0)):
        rows = cat3(step_rows(10, 4, seed=120 + zero_at), rows_of([(10, pull, 2.0, 5)]))
        add(name, "missing", [numeric(11, zero_at, missing=NAN, nan=True)], *rows)
    # an empty NaN bin: the first split (feature 1) takes every NaN row away, with rows of a middle bin
    # that no threshold of feature 0 puts with them; its left child scans feature 0 with nothing in the bin
    b, g, h = cat3(step_rows(10, 4, seed=131), rows_of([(10, -8.0, 2.0, 8), (5, -8.0, 2.0, 8)]))
    sep = np.concatenate([np.zeros(len(b) - 16, dtype=int), np.ones(16, dtype=int)])
    add("nan_empty_in_children", "missing", [numeric(11, 5, missing=NAN, nan=True), numeric(2)], two_col(b, sep), g, h,
        leaves=4, winner=1)
    # ... and the same where bin 0 is not stored: the forward scan's start from what is stored nowhere,
    # with an empty NaN bin
    add("nan_empty_in_children_offset1", "missing", [numeric(11, 0, missing=NAN, nan=True), numeric(2)],
        two_col(b, sep), g, h, leaves=4, winner=1)
    # features of two bins: the default_left rules (zero as missing leaves a feature of two bins
    # without a missing type: the binning's rule)
    b, g, h = rows_of([(0, 2.0, 1.0, 40), (1, -2.0, 1.0, 30)])
    add("two_bins_none", "missing", [numeric(2)], b, g, h)
    add("two_bins_zero", "missing", [numeric(2)], b, g, h, zero_as_missing=True)
    add("two_bins_nan", "missing", [numeric(2, missing=NAN, nan=True)], b, g, h)


# ---- limits: the best candidate exactly on the limit, and one row / one 0.5 of hessian past it
def _limits():
    # hessians of 1: counts are exact.  bins 0 | 1 | 2 hold 50 | 30 | 120 rows; the best split is 0 | 1 2
    b, g, h = rows_of([(0, 4.0, 1.0, 50), (1, -1.0, 1.0, 30), (2, -1.0, 1.0, 120)])
    f = [numeric(3)]
    add("min_data_on", "limits", f, b, g, h, min_data_in_leaf=50)
    add("min_data_past", "limits", f, b, g, h, min_data_in_leaf=51)
    # the left side's hessian is 50 to a threshold of 50, and of 50.5
    add("min_hessian_on", "limits", f, b, g, h, min_sum_hessian_in_leaf=50.0)
    add("min_hessian_past", "limits", f, b, g, h, min_sum_hessian_in_leaf=50.5)
    # gains that are exact: left (32, 64) -> 16, right (-16, 64) -> 4, the leaf (16, 128) -> 2.  With
    # min_gain_to_split = 18 the candidate's gain equals the shift: rejected (the rule is gain > shift)
    b, g, h = rows_of([(0, 0.5, 1.0, 64), (1, -0.25, 1.0, 32), (2, -0.25, 1.0, 32)])
    add("min_gain_on", "limits", f, b, g, h, min_gain_to_split=18.0, winner="none")
    add("min_gain_past", "limits", f, b, g, h, min_gain_to_split=18.0 - 2.0 ** -40)
    # the same candidate (feature 1 at the root, on the shift) decides whether the children scan the
    # feature at all: cells (f0, f1) of 32 rows hold (64 | 16) and (-32 | -32); feature 0 splits the root,
    # feature 1 could split the left child (a gain of 36 over the shift) but is not splittable at the root
    cells = [(0, 0, 2.0), (0, 1, 0.5), (1, 0, -1.0), (1, 1, -1.0)]
    b0 = np.concatenate([[c[0]] * 32 for c in cells])
    b1 = np.concatenate([[c[1]] * 32 for c in cells])
    g = np.concatenate([[c[2]] * 32 for c in cells])
    add("min_gain_on_flag", "limits", [numeric(2), numeric(2)], two_col(b0, b1), g, np.ones(128), leaves=4,
        min_gain_to_split=18.0)
    # the 1e-15 the forward scan starts the left hessian with: one row of 0.5 on the left passes a limit
    # of 0.5 + 5e-16 only with it (zero as missing, the zero rows pull right: the forward scan wins)
    b, g, h = rows_of([(1, 4.0, 0.5, 1), (2, -0.25, 1.0, 20), (0, -1.0, 1.0, 10)])
    add("min_hessian_epsilon", "limits", [numeric(3, missing=ZERO)], b, g, h, zero_as_missing=True,
        min_sum_hessian_in_leaf=0.5 + 5e-16)


# ---- exact ties: mirrored histograms, every side's hessian >= 32 (the 1e-15 terms round away)
def _ties():
    # reverse scan, thresholds 0 and 1: (16, 64) | (0, 64) | (-16, 64): the higher threshold is kept
    b, g, h = rows_of([(0, 0.25, 1.0, 64), (1, 0.0, 2.0, 32), (2, -0.125, 0.5, 128)])
    add("tie_reverse", "ties", [numeric(3)], b, g, h)
    add("tie_reverse_rebuilt", "ties", [numeric(3, 2)], b, g, h)  # (the last bin rebuilt from the totals)
    # the same tie inside one thread's slice of two bins (257 stored bins: bins 128 and 129 go to thread
    # 64): 128 bins of (0.125, 0.5) | (0, 64) | 128 bins of (-0.125, 0.5); thresholds 127 and 128
    spec = [(t, 0.125, 0.5, 1) for t in range(128)] + [(128, 0.0, 2.0, 32)] + [(t, -0.125, 0.5, 1) for t in range(129, 257)]
    b, g, h = rows_of(spec)
    add("tie_reverse_k2", "ties", [numeric(257, 200)], b, g, h)
    # forward scan (zero as missing, the zero rows (-8, 32) pull right): (16, 64) | (0, 64) | (-8, 32);
    # the lower threshold is kept
    b, g, h = rows_of([(0, -0.5, 2.0, 16), (1, 0.125, 0.5, 128), (2, 0.0, 2.0, 32), (3, -0.125, 0.5, 64)])
    add("tie_forward", "ties", [numeric(4, missing=ZERO)], b, g, h, zero_as_missing=True)
    # reverse against forward: the zero rows (0, 64) fit either side with the same gain: reverse stays
    b, g, h = rows_of([(0, 0.0, 2.0, 32), (1, 0.25, 1.0, 64), (2, -0.125, 0.5, 128)])
    add("tie_directions", "ties", [numeric(3, missing=ZERO)], b, g, h, zero_as_missing=True, tie=True)
    b, g, h = rows_of([(1, 0.0, 2.0, 32), (0, 0.25, 1.0, 64), (2, -0.125, 0.5, 128)])
    add("tie_directions_mid", "ties", [numeric(3, 1, missing=ZERO)], b, g, h, zero_as_missing=True, tie=True)
    # the same with NaN rows
    b, g, h = rows_of([(2, 0.0, 2.0, 32), (0, 0.25, 1.0, 64), (1, -0.125, 0.5, 128)])
    add("tie_directions_nan", "ties", [numeric(3, missing=NAN, nan=True)], b, g, h, tie=True)
    # two identical columns: the lower real index wins
    b, g, h = step_rows(12, 6, seed=5)
    add("tie_features", "ties", [numeric(12, 3), numeric(12, 3)], two_col(b, b), g, h)
    # two leaves with identical children: the halves of feature 0 mirror each other on feature 1 --
    # (24, 64) | (8, 64) against (-8, 64) | (-24, 64), a gain of 9 + 1 - 8 each; the lower leaf id is split
    # first.  (Feature 1 has a gain of 4 at the root, or its children would not scan it)
    spec = [(0, 0, 0.375, 1.0, 64), (0, 1, 0.125, 1.0, 64), (1, 0, -0.25, 2.0, 32), (1, 1, -0.1875, 0.5, 128)]
    b0 = np.concatenate([[s[0]] * s[4] for s in spec])
    b1 = np.concatenate([[s[1]] * s[4] for s in spec])
    g = np.concatenate([[s[2]] * s[4] for s in spec])
    h = np.concatenate([[s[3]] * s[4] for s in spec])
    add("tie_leaves", "ties", [numeric(2), numeric(2)], two_col(b0, b1), g, h, leaves=4)


# ---- count rounding: 96 rows of mean hessian 1; the right side's hessian of 92.5 is estimated as 93
# rows (half up; half to even would say 92), which leaves 3 for the left side
def _counts():
    spec = [(0, 4.0, 2.0, 1), (0, 2.0, 1.0, 1), (0, 1.0, 0.5, 1), (1, -0.25, 0.5, 61), (1, -0.25, 2.0, 30),
            (1, -0.25, 1.0, 2)]
    b, g, h = rows_of(spec)
    add("count_half_up", "counts", [numeric(2, 0, mfb=1)], b, g, h, min_data_in_leaf=3)
    add("count_half_up_blocked", "counts", [numeric(2, 0, mfb=1)], b, g, h, min_data_in_leaf=4, winner="none")


# ---- the math beyond the plain formulas
def _noisy(seed, monotone=0, penalty=1.0, flip=False):
    """two features of 12 and 9 bins, a few hundred rows, signal on both"""
    rng = np.random.RandomState(seed)
    n = 600
    b0 = rng.randint(0, 12, n)
    b1 = rng.randint(0, 9, n)
    sgn = -1.0 if flip else 1.0
    raw = sgn * (b0 - 5.5) * 0.4 + (b1 > 4) * 1.5 - (b1 == 2) * 1.0 + rng.randn(n) * 0.7
    g = np.clip(np.rint(raw * 256) / 256, -8, 8)
    h = np.array((0.5, 1.0, 2.0))[rng.randint(0, 3, n)]
    feats = [numeric(12, 4, monotone=monotone, penalty=penalty), numeric(9)]
    return feats, two_col(b0, b1), g, h


def _math():
    # L1: the right side's |sum_g| just below, at and just above lambda_l1 = 4 (left (8, 64))
    for name, last in (("l1_below", -15.0 / 256), ("l1_at", -16.0 / 256), ("l1_above", -17.0 / 256)):
        b, g, h = rows_of([(0, 0.0625, 0.5, 128), (1, -0.0625, 1.0, 63), (1, last, 1.0, 1)])
        add(name, "math", [numeric(2)], b, g, h, lambda_l1=4.0)
    # max_delta_step = 0.25: outputs of -0.5 | 0.125 (one side), -0.5 | 0.5 (both), -0.125 | 0.125 (neither)
    for name, gl, gr in (("mds_one", 32.0, -8.0), ("mds_both", 32.0, -32.0), ("mds_neither", 8.0, -8.0)):
        b, g, h = rows_of([(0, gl / 128, 0.5, 128), (1, gr / 64, 1.0, 64)])
        add(name, "math", [numeric(2)], b, g, h, max_delta_step=0.25)
    variants = {
        "l1": dict(lambda_l1=3.0), "l2": dict(lambda_l2=2.5), "mds": dict(max_delta_step=0.3),
        "smooth": dict(path_smooth=8.0, min_data_in_leaf=2), "min_gain": dict(min_gain_to_split=0.75),
        "all": dict(lambda_l1=1.5, lambda_l2=1.25, max_delta_step=0.4, path_smooth=6.0, min_gain_to_split=0.25,
                    min_data_in_leaf=2),  # (path smoothing asks for two rows a leaf)
    }
    for k, extra in variants.items():
        feats, bins, g, h = _noisy(21)
        add("stump_" + k, "math", feats, bins, g, h, winner=None, **extra)
        feats, bins, g, h = _noisy(21)
        add("tree_" + k, "math", feats, bins, g, h, leaves=4, winner=None, **extra)
    # monotone: the data fall along feature 0 (flip) and the constraint is +1, or rise under -1: the
    # unconstrained best split violates it
    for name, mono, flip in (("mono_plus_violated", 1, False), ("mono_minus_violated", -1, True),
                             ("mono_plus", 1, True), ("mono_minus", -1, False)):
        for leaves in (2, 4):
            feats, bins, g, h = _noisy(33, monotone=mono, flip=flip)
            add("%s_%d" % (name, leaves), "math", feats, bins, g, h, leaves=leaves, winner=None)
    for pen in (0.5, 2.0):
        feats, bins, g, h = _noisy(34, monotone=1, flip=True)
        add("mono_penalty_%g" % pen, "math", feats, bins, g, h, leaves=4, winner=None, monotone_penalty=pen)
    feats, bins, g, h = _noisy(35, monotone=-1)
    add("mono_all", "math", feats, bins, g, h, leaves=4, winner=None, lambda_l1=1.5, lambda_l2=1.25,
        max_delta_step=0.4, path_smooth=6.0, monotone_penalty=0.5, min_data_in_leaf=2)
    for pen in (0.25, 3.0):
        feats, bins, g, h = _noisy(36, penalty=pen)
        add("feature_contri_%g" % pen, "math", feats, bins, g, h, leaves=4, winner=None)


# ---- categorical.  Bin 0 is the bin of values that are no kept category; category bins follow by
# falling row count (ties by rising category).  Bin 0 is the default bin, and the most frequent
# one unless a category holds 70 % of the rows
def _cat_feat(ncat, counts, mfb=0, dropped=False):
    """categories 100, 101, ... given falling counts -> bins 1, 2, ...; bin 0 holds the rows of the
    rarest category when the binning drops it (`dropped`: it keeps at most as many bins as there
    are distinct values), else no row"""
    assert all(counts[i] >= counts[i + 1] for i in range(len(counts) - 1))
    return Feat([9000 if dropped else None] + [100 + i for i in range(ncat)], categorical=True, mfb=mfb,
                missing=NAN if dropped else NONE)


def _cat_rows(counts, gfun, seed):
    rng = np.random.RandomState(seed)
    spec = []
    hs = (0.5, 1.0, 2.0)
    for i, c in enumerate(counts):
        for k in range(c):
            spec.append((i + 1, gfun(i) + rng.randint(-8, 9) / 256.0, hs[(i + k) % 3], 1))
    return rows_of(spec)


def _categorical():
    def wave(i):
        return ((i * 7) % 11 - 5) * 0.25

    # one-hot at num_bin = max_cat_to_onehot (4: three categories + bin 0), sorted at one more
    for name, ncat in (("cat_onehot_at", 3), ("cat_sorted_at", 4)):
        counts = [40 - 3 * i for i in range(ncat)]
        b, g, h = _cat_rows(counts, wave, seed=ncat)
        add(name, "categorical", [_cat_feat(ncat, counts)], b, g, h)
    # candidates left by the cat_smooth filter: 0, 1, 2, 3, many (counts 30, 20, 12, 11, 10, 9, 8, 7).  With
    # one candidate the set is category 0; with two, one category is still all a set may hold, but the
    # descending direction offers category 1, the outlier; with three a set of two wins
    counts = [30, 20, 12, 11, 10, 9, 8, 7]
    b, g, h = _cat_rows(counts, lambda i: (0.5, -2.0, -1.5)[i] if i < 3 else wave(i), seed=8)
    ones = np.ones(len(g))  # (hessians of 1: the estimated counts are the counts)
    for name, smooth, win in (("cat_filter_0", 64.0, "none"), ("cat_filter_1", 25.0, 0), ("cat_filter_2", 15.0, 0),
                              ("cat_filter_3", 12.0, 0), ("cat_filter_many", 2.0, 0)):
        add(name, "categorical", [_cat_feat(8, counts)], b, g, ones, cat_smooth=smooth, winner=win)
    b, g, h = _cat_rows(counts, wave, seed=8)
    add("cat_l2", "categorical", [_cat_feat(8, counts)], b, g, h, cat_l2=10.0, cat_smooth=10.0)
    # equal ratios g / (h + cat_smooth): pairs of categories with the same rows; the order is stable
    cnts = [12, 12, 10, 10, 8, 8]
    b, g, h = rows_of([(i + 1, ((i // 2) - 1) * 0.5, 1.0, c) for i, c in enumerate(cnts)])
    add("cat_equal_ratios", "categorical", [_cat_feat(6, cnts)], b, g, h)
    b, g, h = rows_of([(i + 1, (1 - (i // 2)) * 0.5, 1.0, c) for i, c in enumerate(cnts)])
    add("cat_equal_ratios_falling", "categorical", [_cat_feat(6, cnts)], b, g, h)
    # max_cat_threshold binding (2) and not (32); min_data_per_group on the limit
    counts = [24 - i for i in range(12)]
    b, g, h = _cat_rows(counts, lambda i: (i - 5.5) * 0.25, seed=12)
    add("cat_max_threshold_binding", "categorical", [_cat_feat(12, counts)], b, g, h, max_cat_threshold=2)
    add("cat_max_threshold_free", "categorical", [_cat_feat(12, counts)], b, g, h, max_cat_threshold=32)
    # (hessians of 1; the lowest ratio is category 0 with 24 rows: a first group exactly on the limit)
    add("cat_group_on", "categorical", [_cat_feat(12, counts)], b, g, np.ones(len(g)), min_data_per_group=24)
    add("cat_group_past", "categorical", [_cat_feat(12, counts)], b, g, np.ones(len(g)), min_data_per_group=25)
    # the winning set found from the high end: one category far above the rest
    b, g, h = _cat_rows(counts, lambda i: 3.0 if i == 4 else (i % 3 - 1) * 0.0625, seed=13)
    add("cat_descending", "categorical", [_cat_feat(12, counts)], b, g, h)
    # widths: the narrow kernel's ranks (<= 1024 bins) against the wide kernel's bitonic order
    for num_bin in (1023, 1024, 1025, 4096):
        ncat = num_bin - 1
        per = 2 if num_bin == 4096 else 4
        counts = [per + 1] * 8 + [per] * (ncat - 8)
        rows = cat3(_cat_rows(counts, lambda i: ((i * 37) % 101 - 50) / 64.0, seed=num_bin), rows_of([(0, 0.5, 1.0, 1)]))
        add("cat_width_%d" % num_bin, "categorical", [_cat_feat(ncat, counts, dropped=True)], *rows, max_cat_threshold=64)
    # the most frequent bin: bin 0 holding most rows (a value that is no category: negative), and a
    # category with 75 % of the rows
    counts = [9, 8, 7, 6, 5]
    rows = cat3(_cat_rows(counts, wave, seed=15), rows_of([(0, 0.5, 1.0, 30)]))
    add("cat_mfb_zero_full", "categorical",
        [Feat([-7] + [100 + i for i in range(5)], categorical=True, mfb=0, missing=NAN)], *rows)
    counts = [120, 9, 8, 7, 6, 5, 5]
    b, g, h = _cat_rows(counts, wave, seed=16)
    add("cat_mfb_category", "categorical", [_cat_feat(7, counts, mfb=1)], b, g, h)


for _build in (_widths, _mfb, _missing, _limits, _ties, _counts, _math, _categorical):
    _build()

BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
FAMILIES = sorted({c.family for c in CASES})


# ---------------------------------------------------------------------------------- comparisons

def model_tree(text):
    """the first tree of a model text -> dict of lists (floats / ints by field)"""
    cur = None
    for line in text.splitlines():
        line = line.strip()
        if line.startswith("Tree=0"):
            cur = {}
            continue
        if cur is not None:
            if line.startswith("Tree=") or line == "end of trees":
                break
            if "=" in line:
                k, v = line.split("=", 1)
                cur[k] = v
    assert cur is not None, "no tree in the model text"
    ints = ("split_feature", "decision_type", "left_child", "right_child", "leaf_count", "internal_count",
            "cat_boundaries", "cat_threshold")
    floats = ("split_gain", "threshold", "leaf_value", "internal_value")
    tree = {"num_leaves": int(cur["num_leaves"])}
    for k in ints:
        tree[k] = [int(x) for x in cur.get(k, "").split()]
    for k in floats:
        tree[k] = [float(x) for x in cur.get(k, "").split()]
    return tree


def categories_of(tree, node):
    """the category values of a categorical node's left set"""
    k = int(tree["threshold"][node])
    words = tree["cat_threshold"][tree["cat_boundaries"][k]:tree["cat_boundaries"][k + 1]]
    return [32 * w + b for w, word in enumerate(words) for b in range(32) if (word >> b) & 1]


def check_tree(case, grown, tree, value_rtol, upper_bounds=None, in_memory=None):
    """a model's first tree (model_tree of its text) against the rule's growth of the case: structure,
    feature, threshold bin, default direction, category set and counts equal; leaf values to value_rtol.
    upper_bounds[f]: the bins' upper bounds where known (else the threshold must separate the values of
    the threshold bin and the next).  Gains and internal values: a model text prints them with %g, and
    a recorded reference tree has no more, so they are held to exactly that text; with in_memory =
    (gains, internal values) by node, read from the tree the booster holds, the gain must be the
    float32 of the rule's and the internal values agree to value_rtol"""
    nodes = grown["nodes"]
    assert tree["num_leaves"] == len(nodes) + 1, (case.name, tree["num_leaves"], len(nodes) + 1)
    # the model's node k is the k-th applied split; children: ~leaf for leaves, node index otherwise
    node_of_leaf = {}
    for k, nd in enumerate(nodes):
        s, ft = nd["split"], case.feats[nd["split"]["inner"]]
        where = (case.name, "node", k)
        assert tree["split_feature"][k] == s["real"], where + (tree["split_feature"][k], s["real"])
        dt = tree["decision_type"][k]
        assert (dt & 1) == (1 if ft.categorical else 0), where
        assert (dt >> 2) & 3 == ft.missing, where + ("missing type", dt)
        if ft.categorical:
            want = sorted(int(ft.values[b]) for b in s["cat_bins"])
            assert categories_of(tree, k) == want, where + (categories_of(tree, k), want)
        else:
            assert bool(dt & 2) == bool(s["default_left"]), where + ("default_left", dt, s["default_left"])
            thr, t = tree["threshold"][k], s["threshold"]
            if upper_bounds is not None:
                assert thr == upper_bounds[s["inner"]][t], where + (thr, t, upper_bounds[s["inner"]][t])
            else:
                lo = ft.values[t]
                hi = next((v for v in ft.values[t + 1:] if v is not None and not math.isnan(v)), math.inf)
                assert lo <= thr and (thr < hi or hi == math.inf), where + (thr, t, lo, hi)
        # the tree keeps float32(gain + min_gain_to_split)
        gain32 = float(np.float32(s["gain"] + case.train_params().get("min_gain_to_split", 0.0)))
        if in_memory is not None:
            assert in_memory[0][k] == gain32, where + ("gain", in_memory[0][k], gain32, s["gain"])
            _close(in_memory[1][k], nd["internal_value"], value_rtol, where + ("internal_value",))
        shown = float("%g" % np.float32(gain32))
        assert tree["split_gain"][k] == shown, where + ("gain", tree["split_gain"][k], shown, s["gain"])
        assert tree["internal_count"][k] == nd["internal_count"], where
        # (the text prints internal values with %g)
        shown = float("%g" % nd["internal_value"])
        assert tree["internal_value"][k] == shown, where + ("internal_value", tree["internal_value"][k], shown)
        # the parent's pointer to this node
        if nd["leaf"] in node_of_leaf:
            pk, side = node_of_leaf[nd["leaf"]]
            assert tree[side][pk] == k, where + ("parent link",)
        else:
            assert k == 0, where
        node_of_leaf[nd["left"]] = (k, "left_child")
        node_of_leaf[nd["right"]] = (k, "right_child")
    for leaf, (k, side) in node_of_leaf.items():
        assert tree[side][k] == ~leaf, (case.name, "leaf link", leaf, tree[side][k])
    for i, lf in enumerate(grown["leaves"]):
        assert tree["leaf_count"][i] == lf["n"] if nodes else True, (case.name, "leaf_count", i)
        _close(tree["leaf_value"][i], lf["value"], value_rtol, (case.name, "leaf_value", i))


def _close(got, want, rtol, where):
    assert abs(got - want) <= rtol * abs(want) + 1e-300, where + (got, want)


# ---------------------------------------------------------------------------------- the library's side

def dataset(case, device_type="cpu", **more):
    """(constructed Dataset, training parameters) of a case"""
    import lightgbmv1_amd as lgb
    params = dict(case.train_params(), device_type=device_type, **more)
    cat = case.categorical_features()
    ds = lgb.Dataset(case.X(), case.label(), weight=case.weight(), params=params,
                     categorical_feature=cat if cat else "auto", free_raw_data=False)
    ds.construct()
    return ds, params


def feature_meta(ds):
    """LGBM_AMD_DatasetFeatureMeta: what the binning made of every used feature"""
    import json

    from lightgbmv1_amd import _native as nat
    text = nat.read_string(lambda size, need, buf: nat.call("LGBM_AMD_DatasetFeatureMeta", ds.handle, size, need, buf),
                           1 << 16)
    return json.loads(text)


def assert_meta(case, meta):
    """the binning produced the meta the case intends, every value in the bin it is designed for"""
    assert [m["real"] for m in meta] == list(range(len(case.feats))), (case.name, "a feature was dropped")
    for f, (ft, m) in enumerate(zip(case.feats, meta)):
        want = ft.meta(f)
        got = {k: m[k] for k in ("num_bin", "missing_type", "default_bin", "most_freq_bin", "offset")}
        got["categorical"] = bool(m["categorical"])
        assert got == {k: want[k] for k in got}, (case.name, f, got, want)
        assert m["hist_size"] == ft.num_bin - want["offset"], (case.name, f, m["hist_size"])
        for b, v in enumerate(ft.values):
            if v is None:
                continue
            if ft.categorical:  # (bin 0 holds what is no kept category)
                assert m["categories"][b] == (v if b > 0 else -1), (case.name, f, b, m["categories"][b], v)
            elif math.isnan(v):
                assert b == ft.num_bin - 1 and ft.missing == NAN, (case.name, f, b)
            else:
                ub = m["upper_bounds"]
                assert (b == 0 or ub[b - 1] < v) and v <= ub[b], (case.name, f, b, v)


def upper_bounds(meta):
    return [m.get("upper_bounds") for m in meta]


def check_booster(case, grown, bst, meta):
    """a training booster's one tree against the rule's growth: check_tree with the thresholds held to
    the bins' upper bounds, leaf and internal values to 1e-12 and the gain to float32 rounding.  Gains
    and internal values come from dump_model, which writes the tree in memory in full; the booster must
    be the one that trained (keep_training_booster=True: otherwise train() hands back a booster read
    from its own text, six digits)"""
    gains, internals = {}, {}

    def walk(node):
        if "split_index" in node:
            gains[node["split_index"]] = node["split_gain"]
            internals[node["split_index"]] = node["internal_value"]
            walk(node["left_child"])
            walk(node["right_child"])
    walk(bst.dump_model()["tree_info"][0]["tree_structure"])
    check_tree(case, grown, model_tree(bst.model_to_string()), 1e-12, upper_bounds(meta), in_memory=(gains, internals))
