"""The rule that picks the contribution kernel (src/device/shap_plan.h) through LGBM_AMD_ShapPlan,
against a literal table: no GPU.  The byte counts are worked out by hand from the layout of a
leaves-on-lanes workgroup, 8 * (W * (64 * path + elems) + [F + 1]) + 4 * W * mask words (an even
count), against the 65,536 bytes a workgroup may take."""
import ctypes

import pytest

from lightgbmv1_amd import _native as nat

ROWS, LEAVES = 0, 1  # the kernels; -1: none
AUTO, FORCE_ROWS, FORCE_LEAVES = 0, 1, 2


def _info():
    out = (ctypes.c_int64 * 8)()
    nat.call("LGBM_AMD_ShapLaunchInfo", out)
    return list(out)


def _plan(rows, num_class, max_leaves, max_tree_elems, max_path_len, num_features, choice):
    out = (ctypes.c_int64 * 4)()
    nat.call("LGBM_AMD_ShapPlan", ctypes.c_int64(rows), ctypes.c_int32(num_class), ctypes.c_int32(max_leaves),
             ctypes.c_int32(max_tree_elems), ctypes.c_int32(max_path_len), ctypes.c_int32(num_features),
             ctypes.c_int(choice), out)
    return tuple(out)


def test_launch_info():
    assert _info()[:6] == [64, 3, 4, 2, 1, 65536] and 1 < _info()[6]


# 63 leaves (2 mask words), paths of 15 elements, 28 features; (rows, elems of the largest tree, choice)
@pytest.mark.parametrize("rows, elems, choice, want", [
    (-1, 500, AUTO, (LEAVES, 4, 1, 46984)),          # one row below the threshold
    (0, 500, AUTO, (ROWS, 1, 1, 23272)),             # at it: 8 * (15 * 64 + 29 * 65) + 2 * 64 * 4
    (0, 500, FORCE_LEAVES, (LEAVES, 4, 1, 46984)),
    (1, 500, FORCE_ROWS, (ROWS, 1, 1, 23272)),
    (64, 1079, AUTO, (LEAVES, 4, 1, 65512)),         # the last size at which W = 4 holds phi in LDS
    (64, 1080, AUTO, (LEAVES, 4, 0, 65312)),         # ... then phi moves to a global tile
    (64, 1087, AUTO, (LEAVES, 4, 0, 65536)),         # exactly the budget
    (64, 1088, AUTO, (LEAVES, 2, 1, 33016)),         # W = 4 -> 2
    (64, 3120, AUTO, (LEAVES, 2, 1, 65528)),
    (64, 3135, AUTO, (LEAVES, 2, 0, 65536)),
    (64, 3136, AUTO, (LEAVES, 1, 1, 33008)),         # W = 2 -> 1
    (64, 7231, AUTO, (LEAVES, 1, 0, 65536)),
    (64, 7232, AUTO, (ROWS, 1, 1, 23272)),           # W = 1 does not fit: rows-on-lanes
    (64, 7232, FORCE_LEAVES, (-1, 0, 0, 0)),
])
def test_threshold_and_wave_ladder(rows, elems, choice, want):
    threshold = _info()[6]
    rows = threshold + rows if rows <= 0 else rows
    assert _plan(rows, 1, 63, elems, 15, 28, choice) == want


@pytest.mark.parametrize("num_class, max_path_len", [
    (1, 121),   # a path of 120 distinct features
    (1, 0),     # a node of data_count 0: no tables
    (17, 15),   # more than 16 trees per iteration
])
@pytest.mark.parametrize("choice", [AUTO, FORCE_ROWS, FORCE_LEAVES])
def test_models_no_kernel_serves(num_class, max_path_len, choice):
    assert _plan(64, num_class, 63, 500, max_path_len, 28, choice) == (-1, 0, 0, 0)
    assert _plan(100000, num_class, 63, 500, max_path_len, 28, choice) == (-1, 0, 0, 0)
