"""Raw CSC inputs for the tests of the CSC binning rule (src/device/csc_bins.h): the seeded base
matrix of tests/helpers/csr_bin_cases.py as columns of (row, value) pairs in stored order, the edge
cases placed on top of it, and the C API calls that construct a Dataset from CSC arrays and read
group bins back.

The edge matrix (edge_columns; to be binned with the mappers of a Dataset of the clean columns):
  column 23     empty
  column 22     one entry
  column 9      stored in descending row order
  column 10     stored in shuffled row order
  column 4      (a bundle member, most frequent bin: the zero bin) cells stored twice, the second
                value off the most frequent bin / 0 / NaN
  column 8      (zeros pushed, most frequent value 1.0) cells stored twice, the second value off the
                most frequent bin / at it / 0 / NaN; rows without an entry; rows with a stored 0
  column 1      (NaN bin) a cell stored twice, the second NaN
  columns 3, 6  both stored off their most frequent bins on BOTH_ROWS rows (one EFB bundle)
  columns NCOL, NCOL + 1   not below the reference's num_total_features
"""
import ctypes

import numpy as np

from lightgbmv1_amd import _native as nat
from helpers import csr_bin_cases as cb

NCOL = cb.NCOL
PARAMS = cb.PARAMS
BOTH_ROWS = 12
LOW, HIGH = 3, 6  # the two bundle members stored together


def columns_of(rows, ncol=NCOL):
    """the rows of csr_bin_cases as columns of (row, value), rows ascending"""
    cols = [[] for _ in range(ncol)]
    for r, row in enumerate(rows):
        for c, v in row:
            cols[c].append((r, v))
    return cols


def flatten(cols, vtype=np.float64, ptype=np.int32):
    col_ptr = np.zeros(len(cols) + 1, dtype=ptype)
    col_ptr[1:] = np.cumsum([len(c) for c in cols])
    indices = np.array([r for c in cols for r, _ in c], dtype=np.int32)
    data = np.array([v for c in cols for _, v in c], dtype=vtype)
    return col_ptr, indices, data


def edge_columns(cols, num_row, seed=21):
    """A copy of `cols` with the edge cases; returns (cols, {name: rows})."""
    rng = np.random.RandomState(seed)
    cols = [list(c) for c in cols] + [[(3, 2.0), (7, 1.0)], [(0, 5.0)]]  # (two columns past the reference)
    at = {}
    cols[23] = []
    cols[22] = [(5, 2.5)]
    cols[9] = cols[9][::-1]
    cols[10] = [cols[10][i] for i in rng.permutation(len(cols[10]))]

    def twice(c, seconds, name):
        stored = [r for r, _ in cols[c]]
        picks = [stored[i] for i in rng.choice(len(stored), size=len(seconds), replace=False)]
        cols[c] += list(zip(picks, seconds))
        at[name] = picks

    twice(4, [4.5, 0.0, float("nan")], "twice_4")
    twice(8, [3.0, 1.0, 0.0, float("nan")], "twice_8")
    twice(1, [float("nan")], "twice_1")
    # rows of the push-zeros column without an entry get a stored 0 (a few of them)
    have = set(r for r, _ in cols[8])
    absent = [r for r in range(num_row) if r not in have]
    at["pz_stored_zero"] = absent[:5]
    at["pz_absent"] = absent[5:]
    assert len(absent) > 20
    cols[8] = sorted(cols[8][:-4] + [(r, 0.0) for r in absent[:5]]) + cols[8][-4:]
    # both bundle members off their most frequent bins on the same rows
    rows_low = [r for r, _ in cols[LOW]][:BOTH_ROWS]
    at["both"] = rows_low
    cols[HIGH] = sorted(cols[HIGH] + [(r, 4.2 + 0.01 * k) for k, r in enumerate(rows_low)])
    return cols, at


def with_bad_rows(cols, num_row):
    """... with a row index of -1 and one of num_row (dropped by the rule)"""
    cols = [list(c) for c in cols]
    cols[0] = [(-1, 1.0)] + cols[0] + [(num_row, 1.0)]
    cols[8] = cols[8] + [(num_row, 3.0), (-1, 0.0)]
    return cols


def to_csr(col_ptr, indices, data, num_row):
    """the stable transposition: each row's entries in ascending stored index (pointers clamped
    to the entries, entries on rows outside the matrix dropped)"""
    nelem = len(data)
    ptr = np.clip(np.asarray(col_ptr, dtype=np.int64), 0, nelem)
    col_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    idx = np.asarray(indices[ptr[0]:ptr[-1]], dtype=np.int64)
    val = data[ptr[0]:ptr[-1]]
    keep = (idx >= 0) & (idx < num_row)
    idx, val, col_of = idx[keep], val[keep], col_of[keep]
    order = np.argsort(idx, kind="stable")
    indptr = np.zeros(num_row + 1, dtype=np.asarray(col_ptr).dtype)
    indptr[1:] = np.cumsum(np.bincount(idx, minlength=num_row))
    return indptr, col_of[order].astype(np.int32), val[order]


class NativeCscDataset(cb.NativeDataset):
    """A Dataset handle constructed from raw CSC arrays through LGBM_DatasetCreateFromCSC"""

    def __init__(self, col_ptr, indices, data, num_row, params, reference=None):
        self.arrays = (col_ptr, np.ascontiguousarray(indices, dtype=np.int32), data)
        self.num_row = num_row
        self.handle = ctypes.c_void_p()
        p_ptr, p_code = nat.pointer(col_ptr)
        v_ptr, v_code = nat.pointer(data)
        nat.call("LGBM_DatasetCreateFromCSC", p_ptr, nat.c_int(p_code),
                 self.arrays[1].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v_ptr, nat.c_int(v_code),
                 ctypes.c_int64(len(col_ptr)), ctypes.c_int64(len(data)), ctypes.c_int64(num_row),
                 nat.cstr(nat.params_str(params)), reference.handle if reference is not None else None,
                 ctypes.byref(self.handle))

    def group_bins(self):
        ng = self.num_groups()
        bins = np.full((self.num_row, ng), -7, dtype=np.int32)
        bounds = np.zeros(ng + 1, dtype=np.int64)
        nat.call("LGBM_AMD_DatasetGetGroupBins", self.handle, bins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                 bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(ctypes.c_int(ng)))
        return bins, bounds

    def eval_csr_group_bins(self, indptr, indices, data):
        return cb.NativeDataset.eval_group_bins(self, indptr, indices, data)

    def eval_group_bins(self, col_ptr, indices, data, num_row, nelem=None):
        """LGBM_AMD_CscToGroupBins: the shared rule on the host with this Dataset's mappers"""
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        p_ptr, p_code = nat.pointer(col_ptr)
        v_ptr, v_code = nat.pointer(data)
        ng = ctypes.c_int(-1)
        nat.call("LGBM_AMD_CscToGroupBins", self.handle, None, nat.c_int(p_code), None, None, nat.c_int(v_code),
                 ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), None, ctypes.byref(ng))
        assert ng.value == self.num_groups()
        bins = np.full((num_row, ng.value), -7, dtype=np.int32)
        nat.call("LGBM_AMD_CscToGroupBins", self.handle, p_ptr, nat.c_int(p_code),
                 indices.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v_ptr, nat.c_int(v_code),
                 ctypes.c_int64(len(col_ptr)), ctypes.c_int64(len(data) if nelem is None else nelem),
                 ctypes.c_int64(num_row), bins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ng))
        return bins

    def save(self, path):
        nat.call("LGBM_DatasetSaveBinary", self.handle, nat.cstr(str(path)))
        with open(str(path), "rb") as f:
            return f.read()


def csc_stats():
    """(device CSC constructions, column-wise bin samples) so far in this process"""
    d, c = ctypes.c_int64(-1), ctypes.c_int64(-1)
    nat.call("LGBM_AMD_DeviceBinCscStats", ctypes.byref(d), ctypes.byref(c))
    return d.value, c.value
