"""The rule by which a forest sends a row to a leaf, written down apart from the project's code,
and a walker of v3 model text that applies it: the reference of tests/test_forest_ref_host.py
(CPU: the host predictor and the host path-table evaluator) and of
tests/test_device_forest_decisions.py (GPU: the score, leaf and SHAP kernels).  Pure Python and
NumPy; nothing here imports the project.

The rule.  A node has a decision type dt, a threshold, a missing type m = (dt >> 2) & 3 (0 None,
1 Zero, 2 NaN) and a default-left bit dt & 2.  The input v is the matrix element as float64 (a
float32 converts exactly).

  0. |v| <= float32(1e-35) reads as 0, on every route: dense elements, stored CSR entries, absent
     CSR entries and absent columns.
  1. Categorical (dt & 1): NaN goes right whatever m; v <= -1 goes right; v >= 2**31 (+inf too)
     goes right; otherwise c = trunc(v), so that values in (-1, 0) are category 0, and the row goes
     left iff c < 32 * words and bit c of the node's bitset is set.
  2. Numerical: a NaN with m != 2 reads as 0; then (m == 1 and v == 0) or (m == 2 and v is NaN)
     goes to the default side; otherwise left iff v <= threshold, compared in float64.

The raw score of class k is the float64 sum, in model order, of the leaf values of the trees t
with t % trees_per_iteration == k inside the iteration window: the order of the host predictor and
of the device kernel, so the three are compared for equality.

Also here: model_text(), which writes a v3 model from literal node lists, the hand-written
forests (table, offsets, classes16, classes17) and the edge values their rows carry.
"""
import math

import numpy as np

ZERO = float(np.float32(1e-35))  # kZeroThreshold as the code has it: a float constant
CATEGORICAL, DEFAULT_LEFT = 1, 2
MISSING_NONE, MISSING_ZERO, MISSING_NAN = 0, 1, 2

_INT_KEYS = ("split_feature", "decision_type", "left_child", "right_child", "cat_boundaries", "cat_threshold")
_FLOAT_KEYS = ("threshold", "leaf_value")


def parse(model_text_):
    """(trees per iteration, number of features, [tree]): a tree is a dict of lists split_feature,
    threshold, decision_type, left_child, right_child, leaf_value, cat_boundaries, cat_threshold
    and the int num_leaves.  A one-leaf tree has empty node lists."""
    header, trees, cur = {}, [], None
    for line in model_text_.splitlines():
        line = line.strip()
        if line == "end of trees":
            break
        if line.startswith("Tree="):
            cur = {}
            trees.append(cur)
            continue
        if "=" not in line:
            continue
        key, value = line.split("=", 1)
        (header if cur is None else cur)[key] = value
    out = []
    for raw in trees:
        tree = {"num_leaves": int(raw["num_leaves"])}
        for key in _INT_KEYS:
            tree[key] = [int(x) for x in raw.get(key, "").split()]
        for key in _FLOAT_KEYS:
            tree[key] = [float(x) for x in raw.get(key, "").split()]
        assert len(tree["leaf_value"]) == tree["num_leaves"]
        assert len(tree["split_feature"]) == (tree["num_leaves"] - 1 if tree["num_leaves"] > 1 else 0)
        out.append(tree)
    per_iteration = int(header.get("num_tree_per_iteration", header.get("num_class", "1")))
    return per_iteration, int(header["max_feature_idx"]) + 1, out


def goes_left(v, threshold, dt, words=()):
    """the rule of the module docstring for one node; `words` is a categorical node's bitset"""
    v = float(v)
    if abs(v) <= ZERO:
        v = 0.0
    missing = (dt >> 2) & 3
    if dt & CATEGORICAL:
        if math.isnan(v) or v <= -1.0 or v >= 2.0 ** 31:
            return False
        c = math.trunc(v)
        return c < 32 * len(words) and ((words[c // 32] >> (c % 32)) & 1) == 1
    if math.isnan(v) and missing != MISSING_NAN:
        v = 0.0
    if (missing == MISSING_ZERO and v == 0.0) or (missing == MISSING_NAN and math.isnan(v)):
        return (dt & DEFAULT_LEFT) != 0
    return v <= threshold


def leaf_of(tree, row):
    """the leaf of one tree for one row (a sequence of floats; absent columns read 0)"""
    if tree["num_leaves"] <= 1:
        return 0
    node = 0
    while node >= 0:
        f = tree["split_feature"][node]
        v = row[f] if f < len(row) else 0.0
        dt = tree["decision_type"][node]
        theta = tree["threshold"][node]
        words = ()
        if dt & CATEGORICAL:
            ci = int(theta)
            words = tree["cat_threshold"][tree["cat_boundaries"][ci]:tree["cat_boundaries"][ci + 1]]
        node = tree["left_child"][node] if goes_left(v, theta, dt, words) else tree["right_child"][node]
    return ~node


def walk(model_text_, X, start=0, num=-1):
    """(raw [n, classes], leaf [n, trees of the window]) of the dense matrix X, whose elements are
    taken as they are (float32 or float64); columns the model has and X has not read 0, columns
    past the model's are ignored"""
    per_iteration, _, trees = parse(model_text_)
    iterations = len(trees) // per_iteration
    start = min(max(start, 0), iterations)
    stop = iterations if num is None or num <= 0 else min(iterations, start + num)
    window = trees[start * per_iteration:stop * per_iteration]
    X = np.asarray(X)
    raw = np.zeros((X.shape[0], per_iteration), dtype=np.float64)
    leaf = np.zeros((X.shape[0], len(window)), dtype=np.float64)
    for r in range(X.shape[0]):
        row = [float(x) for x in X[r]]
        for t, tree in enumerate(window):
            j = leaf_of(tree, row)
            leaf[r, t] = j
            raw[r, t % per_iteration] += tree["leaf_value"][j]
    return raw, leaf


def csr_meaning(indptr, indices, data, num_features):
    """the dense matrix [n, num_features] that CSR arrays mean to a predictor: absent entries 0, of
    several stored entries on one column of a row the last one, other columns ignored"""
    data = np.asarray(data)
    out = np.zeros((len(indptr) - 1, num_features), dtype=data.dtype)
    for r in range(len(indptr) - 1):
        for i in range(int(indptr[r]), int(indptr[r + 1])):
            if 0 <= indices[i] < num_features:
                out[r, indices[i]] = data[i]
    return out


# ---- model text from literal node lists ----

def num(feature, threshold, missing, default_left, left, right):
    """a numerical node; children: a node index, or ~leaf"""
    return {"feature": feature, "threshold": float(threshold), "left": left, "right": right,
            "dt": (missing << 2) | (DEFAULT_LEFT if default_left else 0)}


def cat(feature, categories, missing, left, right, words=None):
    """a categorical node that sends `categories` left; its bitset has `words` 32-bit words (by
    default as many as the largest category needs)"""
    n = max(categories) // 32 + 1 if words is None else words
    bits = [0] * n
    for c in categories:
        bits[c // 32] |= 1 << (c % 32)
    return {"feature": feature, "bits": bits, "left": left, "right": right, "dt": (missing << 2) | CATEGORICAL}


def tree(nodes, leaf_values, leaf_counts=None):
    return {"nodes": nodes, "leaf_values": [float(v) for v in leaf_values],
            "leaf_counts": list(leaf_counts) if leaf_counts is not None else [8] * len(leaf_values)}


def _join(values):
    return " ".join(repr(v) if isinstance(v, float) else str(v) for v in values)


def model_text(trees, num_features, num_class=1):
    """v3 model text of literal trees (tree(): nodes from num() / cat(), leaf values and counts):
    leaf and internal counts are written, which contributions need"""
    lines = ["tree", "version=v3", "num_class=%d" % num_class, "num_tree_per_iteration=%d" % num_class,
             "label_index=0", "max_feature_idx=%d" % (num_features - 1)]
    if num_class == 1:
        lines.append("objective=regression")
    lines += ["feature_names=" + " ".join("Column_%d" % i for i in range(num_features)),
              "feature_infos=" + " ".join(["[-5:5]"] * num_features), ""]
    for t, tr in enumerate(trees):
        nodes, values, counts = tr["nodes"], tr["leaf_values"], tr["leaf_counts"]
        lines.append("Tree=%d" % t)
        lines.append("num_leaves=%d" % len(values))
        if not nodes:
            assert len(values) == 1
            lines += ["num_cat=0", "leaf_value=" + _join(values), "shrinkage=1", "", ""]
            continue
        assert len(values) == len(nodes) + 1

        def count(child):
            return counts[~child] if child < 0 else count(nodes[child]["left"]) + count(nodes[child]["right"])

        internal = [count(i) for i in range(len(nodes))]
        thresholds, boundaries, bits = [], [0], []
        for n in nodes:
            if n["dt"] & CATEGORICAL:
                thresholds.append(len(boundaries) - 1)
                bits += n["bits"]
                boundaries.append(len(bits))
            else:
                thresholds.append(n["threshold"])
        lines += ["num_cat=%d" % (len(boundaries) - 1),
                  "split_feature=" + _join(n["feature"] for n in nodes),
                  "split_gain=" + _join([1] * len(nodes)),
                  "threshold=" + _join(thresholds),
                  "decision_type=" + _join(n["dt"] for n in nodes),
                  "left_child=" + _join(n["left"] for n in nodes),
                  "right_child=" + _join(n["right"] for n in nodes),
                  "leaf_value=" + _join(values),
                  "leaf_weight=" + _join(counts),
                  "leaf_count=" + _join(counts),
                  "internal_value=" + _join([0] * len(nodes)),
                  "internal_weight=" + _join(internal),
                  "internal_count=" + _join(internal)]
        if len(boundaries) > 1:
            lines += ["cat_boundaries=" + _join(boundaries), "cat_threshold=" + _join(bits)]
        lines += ["shrinkage=1", "", ""]
    lines += ["end of trees", ""]
    return "\n".join(lines)


# ---- edge values ----

_F32_ZERO = np.float32(1e-35)
_F32_TENTH = np.float32(0.1)

NUMERICAL_EDGES = [
    float("nan"), 0.0, -0.0,
    ZERO, -ZERO, float(np.nextafter(ZERO, 1.0)), float(np.nextafter(-ZERO, -1.0)), 1e-40, 5e-324,
    0.1, float(np.nextafter(0.1, 0.0)), float(np.nextafter(0.1, 1.0)),
    float(_F32_TENTH),                                # above the double 0.1: goes right
    float(np.nextafter(_F32_TENTH, np.float32(0))),   # the float32 below it: goes left
    float("inf"), float("-inf"), 1e300, -1e300,
]

CATEGORICAL_EDGES = [
    float("nan"), 0.0, -0.0, -0.5, -0.999, -1.0, -1.5,
    0.999, 1.0, 4.999, 5.0, 5.5, 31.0, 31.9, 32.0, 33.0, 63.0, 63.99, 64.0, 65.0,
    1e9, 2147483647.0, 2147483648.0, 4294967296.0, 4294967301.0, 1e300,
    float("inf"), float("-inf"), -2147483649.0, ZERO, 1e-40,
]

OFFSETS_CATEGORIES = [0.0, 31.0, 32.0, 63.0, 64.0, 95.0, 96.0, 97.0]


class Forest:
    """a hand-written forest: its model text, the rows that probe it (float64; the tests cast them)
    and the iteration window it is predicted with"""

    def __init__(self, name, trees, num_features, rows, num_class=1, start=0, num=-1):
        self.name, self.trees, self.num_features, self.num_class = name, trees, num_features, num_class
        self.text = model_text(trees, num_features, num_class)
        self.rows = np.ascontiguousarray(rows, dtype=np.float64)
        self.start, self.num = start, num

    def tiled(self, n):
        """n rows: the probing rows over and over"""
        return self.rows[np.arange(n) % len(self.rows)]


# table: one stump per (kind, missing type, default side), each on its own feature, with leaf
# values that are distinct powers of two: a raw score names the side every stump took
TABLE_THETA = 0.1
TABLE_SET = [0, 5, 31, 32, 63]  # two words


def _table():
    trees = []
    for missing in (MISSING_NONE, MISSING_ZERO, MISSING_NAN):
        for default_left in (False, True):
            t = len(trees)
            trees.append(tree([num(t, TABLE_THETA, missing, default_left, ~0, ~1)],
                              [2.0 ** (2 * t - 8), 2.0 ** (2 * t - 7)], [8, 24]))
    for missing in (MISSING_NONE, MISSING_ZERO, MISSING_NAN):
        t = len(trees)
        trees.append(tree([cat(t, TABLE_SET, missing, ~0, ~1)], [2.0 ** (2 * t - 8), 2.0 ** (2 * t - 7)], [24, 8]))
    n = max(len(NUMERICAL_EDGES), len(CATEGORICAL_EDGES))
    rows = np.empty((n, 9))
    for r in range(n):  # one edge value in every column of its kind
        rows[r, :6] = NUMERICAL_EDGES[r % len(NUMERICAL_EDGES)]
        rows[r, 6:] = CATEGORICAL_EDGES[r % len(CATEGORICAL_EDGES)]
    return Forest("table", trees, 9, rows)


# offsets: three trees of numerical (features 0, 1) and categorical (features 2, 3) nodes whose
# bitsets are 1, 3 and 2 words long, in a different order in every tree: a tree's offset into the
# forest's boundaries and bitset words, and a node's own boundary, are non-zero somewhere
def _offsets():
    a = tree([num(0, 0.5, MISSING_NAN, True, 1, 2),
              cat(2, [0, 31], MISSING_NONE, ~0, 3),
              cat(3, [32, 64, 95], MISSING_NAN, ~1, ~2),
              cat(2, [5, 63], MISSING_ZERO, ~3, ~4)],
             [2.0 ** -7, 2.0 ** -6, 2.0 ** -5, 2.0 ** -4, 2.0 ** -3], [8, 8, 16, 24, 8])
    b = tree([cat(2, [31, 63, 64, 95], MISSING_ZERO, 1, 2),
              num(1, -0.25, MISSING_ZERO, False, ~0, ~1),
              cat(3, [0, 31], MISSING_NONE, ~2, 3),
              num(0, 1.5, MISSING_NONE, False, ~3, ~4)],
             [2.0 ** -2, 2.0 ** -1, 1.0, 2.0, 4.0], [8, 16, 8, 8, 24])
    c = tree([num(1, 0.0, MISSING_NAN, False, 1, 2),
              cat(3, [32, 63], MISSING_NAN, ~0, 3),
              cat(2, [0], MISSING_NONE, ~1, ~2),
              cat(3, [0, 64, 95], MISSING_ZERO, ~3, ~4)],
             [8.0, 16.0, 32.0, 64.0, 128.0], [16, 8, 8, 8, 8])
    f0 = [0.0, 1.0, 2.0, float("nan")]
    f1 = [-1.0, 0.0, 0.5, float("nan")]
    cats = OFFSETS_CATEGORIES + CATEGORICAL_EDGES
    rng = np.random.RandomState(17)
    rows = []
    for x2 in OFFSETS_CATEGORIES:  # every pair of the probed categories, the numerical values mixed
        for x3 in OFFSETS_CATEGORIES:
            rows.append([f0[rng.randint(4)], f1[rng.randint(4)], x2, x3])
    for _ in range(192):
        rows.append([f0[rng.randint(4)], f1[rng.randint(4)], cats[rng.randint(len(cats))], cats[rng.randint(len(cats))]])
    return Forest("offsets", [a, b, c], 4, rows)


# classes16 / classes17: two iterations of 16 (dev::kMaxPredClasses) and of 17 stumps
def _classes(k, **window):
    trees = []
    for t in range(2 * k):
        trees.append(tree([num(t % 4, (t % 9 - 4) * 0.125, t % 3, t % 2 == 1, ~0, ~1)],
                          [float(t + 1), -(t + 1) / 4.0], [8, 24]))
    rng = np.random.RandomState(k)
    rows = np.concatenate([np.repeat(np.array(NUMERICAL_EDGES)[:, None], 4, axis=1),
                           np.round(rng.randn(46, 4) * 4) / 8])
    rows[rng.rand(*rows.shape) < 0.1] = 0.0
    name = "classes%d" % k + ("_window" if window else "")
    return Forest(name, trees, 4, rows, num_class=k, **window)


FORESTS = {f.name: f for f in (_table(), _offsets(), _classes(16), _classes(16, start=1, num=1), _classes(17))}
DEVICE_FORESTS = ["table", "offsets", "classes16", "classes16_window"]
