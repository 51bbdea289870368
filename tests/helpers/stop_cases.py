"""Forests, rows and the reference of the early-stopped prediction of GPU tensors
(tests/test_tensor_predict_stop_host.py without a GPU, tests/test_device_tensor_predict_stop.py on one).

12 iterations of stumps: iteration i splits feature i % 9 at 0 into -1.0 and +1.0 for class 0; with
K > 1 classes, class 1 takes -0.5 and +0.5 on feature (i + 1) % 9 and the other classes one-leaf
trees of 0.  The rows are all 512 sign patterns of the 9 features and a row of zeros: two tiles of
256 rows and one of one row.  Every sum is a multiple of 0.5, exact in any order.

The rule (src/device/tensor_predict.h): a counter starts at the window's first iteration; after
every freq-th iteration a row whose margin -- 2 |score| for one class, the largest class sum minus
the second largest otherwise -- is above the threshold, strictly, keeps its sums as they are.

CASES lists (objective line, K, freq, margin, start_iteration, the iterations of the window after
which rows stop).  The last is asserted on the reference alone before the code under test runs, with
"some row never stops": it is every check of the window before its end, except the checks at which no
row of these stumps can stop.  Those are, for freq 1, the checks before a margin can be reached at
all and, for one class, the checks whose parity the sum's does not match (after n stumps the sum is
n mod 2); and check 3 of margin 6.0 with freq 3, where the largest margin 2 * 3 is not above 6.0 --
the case of the strict comparison.  By exhaustion the rows include some whose margin is above the
threshold between two checks and below it again at the check.
"""
import functools
import itertools

import numpy as np

from helpers import forest_ref as fr

ITERATIONS = 12
ROWS = np.vstack([np.array(list(itertools.product([-1.0, 1.0], repeat=9))), np.zeros((1, 9))])
BINARY, SOFT3, SOFT16 = "objective=binary sigmoid:1", "objective=multiclass num_class:3", "objective=multiclass num_class:16"

CASES = [
    (BINARY, 1, 1, 5.0, 0, {3, 5, 7, 9, 11}), (BINARY, 1, 1, 6.0, 0, {4, 6, 8, 10}),
    (BINARY, 1, 3, 5.0, 0, {3, 6, 9}), (BINARY, 1, 3, 6.0, 0, {6, 9}),
    (BINARY, 1, 5, 5.0, 0, {5, 10}), (BINARY, 1, 5, 6.0, 0, {5, 10}),
    (BINARY, 1, 3, 5.0, 2, {3, 6, 9}), (BINARY, 1, 1, 6.0, 2, {4, 6, 8}),
    (SOFT3, 3, 1, 2.0, 0, set(range(3, 12))), (SOFT3, 3, 3, 1.0, 0, {3, 6, 9}), (SOFT3, 3, 5, 2.0, 2, {5}),
    (SOFT16, 16, 3, 1.0, 0, {3, 6, 9}), (SOFT16, 16, 5, 1.5, 0, {5, 10}),
]


@functools.lru_cache(maxsize=None)
def model(line, K):
    """the model text of K trees per iteration under the objective `line`"""
    trees = []
    for i in range(ITERATIONS):
        trees.append(fr.tree([fr.num(i % 9, 0.0, 0, False, ~0, ~1)], [-1.0, 1.0]))
        if K > 1:
            trees.append(fr.tree([fr.num((i + 1) % 9, 0.0, 0, False, ~0, ~1)], [-0.5, 0.5]))
            trees += [fr.tree([], [0.0])] * (K - 2)
    text = fr.model_text(trees, 9, K)
    if K == 1:
        return text.replace("objective=regression", line)
    return text.replace("label_index=0", "label_index=0\n" + line)


@functools.lru_cache(maxsize=None)
def _leaves(K, start):
    return fr.walk(model("objective=regression", K), ROWS, start, -1)[1].astype(int)


def reference(K, freq, margin, start):
    """(raw scores [513, K] of the rule, the iteration of the window after which each row stopped
    or 0) for the window from `start` to the last iteration"""
    leaves = _leaves(K, start)
    values = [t["leaf_value"] for t in fr.parse(model("objective=regression", K))[2]][start * K:]
    raw, stopped = np.zeros((len(ROWS), K)), np.zeros(len(ROWS), dtype=int)
    for r in range(len(ROWS)):
        for i in range(ITERATIONS - start):
            for k in range(K):
                raw[r, k] += values[i * K + k][leaves[r, i * K + k]]
            top = np.sort(raw[r])
            if (i + 1) % freq == 0 and (2 * abs(raw[r, 0]) if K == 1 else top[-1] - top[-2]) > margin:
                stopped[r] = i + 1
                break
    stopped[stopped == ITERATIONS - start] = 0  # (after the last iteration nothing is left to skip)
    return raw, stopped


def checked_reference(K, freq, margin, start, stops):
    raw, stopped = reference(K, freq, margin, start)
    assert set(stopped.tolist()) == stops | {0}, sorted(set(stopped.tolist()))
    return raw
