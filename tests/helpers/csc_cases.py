"""CSC arrays for the tests of device CSC prediction (tests/test_csc_slots.py without a GPU,
tests/test_device_csc_predict.py with one) and what they mean.

csc_meaning() is the dense matrix that CSC arrays mean to a predictor (the host's CSCToRows
followed by Predictor::Fill): absent entries 0, stored zeros and NaN kept, columns past the model's
ignored, an entry whose row is outside the matrix dropped, and of several stored entries on one
cell the last stored one.  scipy's toarray() *sums* repeated cells, so the expected values of a
matrix with repeats come from here.
"""
import numpy as np

WIDE_ROWS, WIDE_COLS = 1100, 2000
WIDE_INFORMATIVE = list(range(7, WIDE_COLS, 200))  # 10 columns
WIDE_COUNTS = [0, 1, 63, 64, 65, 257]              # stored entries of the first columns
WIDE_INFORMATIVE_COUNTS = [640, 641, 662, 639, 705, 736, 767, 769, 832, 257]


def csc_meaning(col_ptr, indices, data, num_row, num_features):
    """the dense matrix [num_row, num_features] of the arrays, built in stored order"""
    data = np.asarray(data)
    out = np.zeros((num_row, num_features), dtype=data.dtype)
    for c in range(min(len(col_ptr) - 1, num_features)):
        lo, hi = (min(max(int(p), 0), len(data)) for p in (col_ptr[c], col_ptr[c + 1]))
        for i in range(lo, hi):
            if 0 <= indices[i] < num_row:
                out[indices[i], c] = data[i]
    return out


def from_columns(columns, dtype=np.float64, ptr_dtype=np.int32):
    """(col_ptr, indices, data) of a list of columns, each a (rows, values) pair in stored order"""
    col_ptr = np.cumsum([0] + [len(r) for r, _ in columns]).astype(ptr_dtype)
    indices = np.array([i for r, _ in columns for i in r], dtype=np.int32)
    data = np.array([x for _, v in columns for x in v], dtype=dtype)
    return col_ptr, indices, data


def shuffled_within_columns(rng, col_ptr, indices, data, columns=None):
    """the same entries in another stored order within each column (all columns, or `columns`)"""
    indices, data = indices.copy(), data.copy()
    for c in (range(len(col_ptr) - 1) if columns is None else columns):
        lo, hi = int(col_ptr[c]), int(col_ptr[c + 1])
        perm = rng.permutation(hi - lo) + lo
        indices[lo:hi], data[lo:hi] = indices[perm], data[perm]
    return indices, data


def hostile(used, unused, num_col, num_row):
    """(columns for from_columns, the dense matrix they mean) of a hand-written matrix of num_col
    + 2 columns: cells stored twice and three times (a stored zero last), empty columns, columns
    past the model's num_col, and row indices -1, num_row and 2**31 - 1, which are dropped"""
    u0, u1, u2 = used[0], used[1], used[-1]
    columns = [([], []) for _ in range(num_col + 2)]
    columns[u0] = ([5, 2, 5, 9], [1.0, 2.0, 3.0, 0.0])                    # row 5 twice: 3.0; a stored zero
    columns[u1] = ([4, 4, 0, 4, 7, 7], [4.0, 5.0, 6.0, 0.0, 7.0, 0.0])    # row 4 three times, row 7 twice: zeros last
    columns[u2] = ([-1, 3, num_row, 1, 2 ** 31 - 1, num_row - 1], [9.0, 8.0, 9.0, np.nan, 9.0, -2.5])
    columns[unused] = ([0, 1, 2], [1.5, 2.5, 3.5])                        # (no tree splits on it)
    columns[num_col] = ([0, 3], [9.0, 9.0])                               # columns the model does not have
    columns[num_col + 1] = ([num_row - 1], [9.0])
    want = np.zeros((num_row, num_col))
    want[[5, 2], u0] = 3.0, 2.0
    want[0, u1] = 6.0
    want[[3, 1, num_row - 1], u2] = 8.0, np.nan, -2.5
    want[[0, 1, 2], unused] = 1.5, 2.5, 3.5
    return columns, want


def wide_matrix():
    """(CSC arrays, the dense matrix they mean) of WIDE_ROWS x WIDE_COLS at ~1% density: the first
    columns hold WIDE_COUNTS stored entries, every third informative column is shuffled, one
    informative column stores a cell three times more than 64 entries apart and another repeats
    cells inside one batch of 64, and explicit zeros are stored"""
    rng = np.random.RandomState(8)
    columns = []
    for c in range(WIDE_COLS):
        if c < len(WIDE_COUNTS):
            n = WIDE_COUNTS[c]
        elif c in WIDE_INFORMATIVE:  # (the shuffled ones end on, before and after a batch of 64)
            n = WIDE_INFORMATIVE_COUNTS[WIDE_INFORMATIVE.index(c)]
        else:
            n = rng.randint(0, 12)
        rows = np.sort(rng.choice(WIDE_ROWS, size=n, replace=False))
        vals = rng.randn(n)
        vals[rng.rand(n) < 0.1] = 0.0  # explicit zeros
        if c in WIDE_INFORMATIVE and WIDE_INFORMATIVE.index(c) % 3 == 0:
            rows = rng.permutation(rows)
        if c == WIDE_INFORMATIVE[1]:   # one cell three times, 64-entry batches apart (ascending otherwise)
            rows[[3, 200, 500]] = rows[3]
        if c == WIDE_INFORMATIVE[2]:   # repeats inside one batch of 64: entries 64 .. 127
            rows[[70, 75, 90]] = rows[66]
            rows[100] = rows[99]
        columns.append((rows.tolist(), vals.tolist()))
    col_ptr, indices, data = from_columns(columns)
    return (col_ptr, indices, data), csc_meaning(col_ptr, indices, data, WIDE_ROWS, WIDE_COLS)


def mixed_csc(X, ptr_dtype=np.int32):
    """(col_ptr, indices, data, columns) of the rows of X with, by turns, the zeros absent or
    stored, a stored NaN, one cell stored twice (a decoy first: the last stored entry is the
    value) and a column past X's; and the dense matrix that this means.  Elements with 0 < |v| <=
    1e-35 become 0 first: host and device read such a stored value differently (README, Open
    issues)"""
    X = X.copy()
    n, f = X.shape
    X[1::7, 0] = np.nan
    columns = []
    for c in range(f):
        rows, vals = [], []
        for r in range(n):
            v = X[r, c]
            if 0 < abs(v) <= 1e-35:
                X[r, c] = 0.0
                v = X[r, c]
            if r % 3 == 0 and r % f == c:
                rows.append(r)
                vals.append(5.0)  # (the decoy; where the cell holds an absent zero, its only entry)
            if v != 0 or r % 2 == 1:  # (NaN != 0: stored)
                rows.append(r)
                vals.append(v)
        columns.append((rows, vals))
    columns.append((list(range(0, n, 4)), [3.0] * len(range(0, n, 4))))
    col_ptr, indices, data = from_columns(columns, X.dtype, ptr_dtype)
    assert np.isnan(data).any() and (data == 0).any() and any(len(set(r)) < len(r) for r, _ in columns)
    return (col_ptr, indices, data, f + 1), csc_meaning(col_ptr, indices, data, n, f)
