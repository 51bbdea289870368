"""The rule that sizes the chunks of rows of a device prediction (src/boosting/predict_chunks.h),
evaluated on the host by LGBM_AMD_PredictChunkPlan with the tile of 64 rows: the automatic size on
both sides of "one tile fits", the halving of a CSR chunk until its stored entries fit (uniform
rows, a row count that is no tile multiple, rows whose entries sit in the first tile) and the
forced size of LGBM_AMD_PREDICT_CHUNK_ROWS.  The expected values are what the three drivers of
dense, CSR and CSC inputs computed, each with its own copy of the arithmetic, before they became
one; tests/native/predict_chunks_driver.cpp walks the same table under the sanitizers."""
import ctypes

import numpy as np
import pytest

from lightgbmv1_amd import _native as nat

PER_ROW = 100
PER_ENTRY = 12  # where a pointer is given, else 0


def uniform(nrow, k=10):
    return np.arange(nrow + 1, dtype=np.int64) * k


def skewed(nrow=4096):
    """rows 0-63 hold 1000 entries each, the rest none"""
    return np.minimum(np.arange(nrow + 1, dtype=np.int64), 64) * 1000


def fullest(ptr, rows):
    starts = np.arange(0, len(ptr) - 1, rows)
    return int((ptr[np.minimum(starts + rows, len(ptr) - 1)] - ptr[starts]).max())


RAGGED = np.concatenate([[0], np.cumsum((np.arange(1000) * 7919) % 23)]).astype(np.int64)

# (id, nrow, budget, fixed, forced, ptr, expected (chunk, entries) or None for "does not fit")
TABLE = [
    ("whole_budget", 100000, 1000000, 0, 0, None, (9984, 0)),
    ("capped_by_rows", 5000, 1000000, 0, 0, None, (5000, 0)),
    ("one_tile_exactly", 5000, 6400, 0, 0, None, (64, 0)),
    ("one_byte_short", 5000, 6399, 0, 0, None, None),
    ("fixed_over_budget", 5000, 1000, 2000, 0, None, None),
    ("uniform_entries_halve_once", 4096, 500000, 8, 0, uniform(4096), (2048, 20480)),
    ("rows_not_a_tile_multiple", 3000, 400000, 0, 0, uniform(3000), (1472, 14720)),
    ("skewed", 4096, 800000, 0, 0, skewed(), (256, 64000)),
    ("skewed_never_fits", 4096, 760000, 0, 0, skewed(), None),
    ("forced_tiny_budget", 1000, 1, 0, 192, uniform(1000), (192, 1920)),
    ("forced_tiny_budget_ragged", 1000, 1, 0, 192, RAGGED, (192, fullest(RAGGED, 192))),
    ("forced_over_rows", 3000, 1000000, 0, 5000, None, (3000, 0)),
    ("forced_over_rows_entries", 3000, 1, 0, 5000, uniform(3000), (3000, 30000)),
]


def plan(nrow, budget, fixed, forced, ptr):
    out = (ctypes.c_int64 * 3)()
    p = None if ptr is None else ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nat.call("LGBM_AMD_PredictChunkPlan", ctypes.c_int64(nrow), ctypes.c_int64(budget), ctypes.c_int64(fixed),
             ctypes.c_int64(PER_ROW), ctypes.c_int64(0 if ptr is None else PER_ENTRY), ctypes.c_int64(forced), p, out)
    return out[0], out[1], bool(out[2])


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_chunk_plan(case):
    _, nrow, budget, fixed, forced, ptr, want = case
    assert ptr is None or (len(ptr) == nrow + 1 and ptr.dtype == np.int64)
    chunk, entries, fits = plan(nrow, budget, fixed, forced, ptr)
    if want is None:
        assert not fits
        return
    assert fits and (chunk, entries) == want
    if forced <= 0:  # what the plan promises: a tile multiple (or every row) that fits with its fullest chunk
        assert chunk == nrow or chunk % 64 == 0
        assert fixed + chunk * PER_ROW + entries * (0 if ptr is None else PER_ENTRY) <= budget
    if ptr is not None:
        assert entries == fullest(ptr, chunk)
