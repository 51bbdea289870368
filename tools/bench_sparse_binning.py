"""Construction time of a Dataset from a scipy CSR matrix, in seconds, with the stored entries
binned on the host (LGBM_AMD_DEVICE_BINNING=0: Dataset::PushSparseRow per row, the only path
before the device CSR binning) and on the device (=1: src/device/csr_bin_kernels.hip):

  train   lgb.Dataset(X).construct(): the row sample and the bin mappers (host on both paths),
          then the binning of every stored entry
  valid   lgb.Dataset(X, reference=train).construct(): the binning alone

for seeded float32 matrices of --shapes rows x cols x entries-per-row (default: 1M x 2000 at 2 %
and 10M x 40 at 10 %), and for the first rows of the first shape at every --sweep row count (the
break-even of the gate).  Every construction ends in a blocking device-to-host copy on the device
path, so the host clock around it covers the device work.  Host and device alternate inside one
run after a warm-up of each; the median of --repeats is reported.  "equal" tells whether both
paths saved the same binary file (checked on the smallest sweep entry).  Prints one JSON line.

--layout csc times LGBM_DatasetCreateFromCSC on the same matrices converted to CSC, on three paths:
  host     LGBM_AMD_DEVICE_BINNING=0: the matrix transposed into rows, every row pushed
  tocsr    X.tocsr() inside the timed region, then the device CSR path
  device   the device CSC path (src/device/csc_bin_kernels.hip)
--equal-full compares the binary files of all paths at every full shape as well; --shuffle-column
times the device CSC path again with the entries of one column in shuffled order (that column is
walked by a single wave).

  python tools/bench_sparse_binning.py
  python tools/bench_sparse_binning.py --shapes 200000x2000x40 --sweep
  rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_binning.py --shapes 1000000x2000x40 \\
      --sweep --modes 1 --repeats 1       # (the kernels of the device path alone)
  python tools/bench_sparse_binning.py --layout csc --equal-full --shuffle-column
  rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_binning.py --layout csc --sweep \
      --paths device --repeats 1
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_csr(rows, cols, per_row, seed):
    """per_row stored entries in every row, one in each of per_row equal strata of the columns:
    sorted, no duplicates, density per_row / cols"""
    rng = np.random.RandomState(seed)
    width = cols // per_row
    indices = (rng.randint(0, width, size=(rows, per_row), dtype=np.int32) +
               (np.arange(per_row, dtype=np.int32) * width)[None, :]).reshape(-1)
    data = rng.standard_normal(rows * per_row).astype(np.float32)
    indptr = np.arange(rows + 1, dtype=np.int64) * per_row
    return sp.csr_matrix((data, indices, indptr.astype(np.int32 if indptr[-1] < 2 ** 31 else np.int64)),
                         shape=(rows, cols))


def csr_calls():
    from lightgbmv1_amd import _native as nat
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DeviceBinStats", None, ctypes.byref(out))
    return out.value


def csc_calls():
    from lightgbmv1_amd import _native as nat
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DeviceBinCscStats", ctypes.byref(out), None)
    return out.value


def shuffled_column(X):
    """a copy of the CSC matrix X with the entries of its longest column in shuffled order"""
    c = int(np.argmax(np.diff(X.indptr)))
    s, e = X.indptr[c], X.indptr[c + 1]
    order = np.random.RandomState(3).permutation(e - s)
    indices, data = X.indices.copy(), X.data.copy()
    indices[s:e], data[s:e] = indices[s:e][order], data[s:e][order]
    return sp.csc_matrix((data, indices, X.indptr), shape=X.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["1000000x2000x40", "10000000x40x4"])
    ap.add_argument("--sweep", nargs="*", type=int, default=[400_000, 100_000, 25_000, 6_000],
                    help="row counts of the first shape timed as well")
    ap.add_argument("--modes", nargs="*", default=["0", "1"], choices=["0", "1"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--layout", default="csr", choices=["csr", "csc"])
    ap.add_argument("--paths", nargs="*", default=None, help="only these paths (host, tocsr, device)")
    ap.add_argument("--equal-full", action="store_true", help="compare the files at the full shapes too")
    ap.add_argument("--shuffle-column", action="store_true", help="csc: one column unsorted, device path")
    args = ap.parse_args()

    import lightgbmv1_amd as lgb

    if lgb.device_count() < 1:
        raise SystemExit("bench_sparse_binning.py needs a HIP device")
    params = {"objective": "regression", "device_type": "gpu", "max_bin": 255, "verbose": -1,
              "num_threads": args.host_threads}

    csc = args.layout == "csc"
    # the paths timed: (name, LGBM_AMD_DEVICE_BINNING, convert to CSR inside the timed region)
    if csc:
        paths = [("host", "0", False), ("tocsr", "1", True), ("device", "1", False)]
    else:
        paths = [("host", "0", False), ("device", "1", False)]
    paths = [p for p in paths if p[1] in args.modes and (args.paths is None or p[0] in args.paths)]

    def build(X, path, reference=None):
        name, mode, convert = path
        os.environ["LGBM_AMD_DEVICE_BINNING"] = mode
        before = csr_calls(), csc_calls()
        t = time.perf_counter()
        ds = lgb.Dataset(X.tocsr() if convert else X, params=params if reference is None else None,
                         reference=reference).construct()
        dt = time.perf_counter() - t
        took = csr_calls() != before[0], csc_calls() != before[1]
        if took != (mode == "1" and (convert or not csc), mode == "1" and csc and not convert):
            raise SystemExit("path %s did not run as asked" % name)
        return dt, ds

    def measure(X, paths=paths, note=None):
        out = {"rows": X.shape[0], "cols": X.shape[1], "entries": int(X.nnz)}
        if note:
            out["note"] = note
        times = {(p[0], k): [] for p in paths for k in ("train", "valid")}
        for rep in range(args.repeats + 1):  # (the first round warms every path up)
            for path in paths:
                dt, train = build(X, path)
                dv, valid = build(X, path, reference=train)
                if rep > 0:
                    times[(path[0], "train")].append(dt)
                    times[(path[0], "valid")].append(dv)
                del train, valid
        for (name, kind), v in times.items():
            out["%s_%s_s" % (name, kind)] = round(statistics.median(v), 4)
            out["%s_%s_all" % (name, kind)] = [round(x, 4) for x in v]
        print(json.dumps(out), file=sys.stderr, flush=True)  # (progress; the result line goes to stdout)
        return out

    def files_equal(X):
        """whether every path saves the same training set and the same reference= set of its first third"""
        files = []
        with tempfile.TemporaryDirectory() as d:
            for path in paths:
                _, train = build(X, path)
                _, valid = build(X[:max(1, X.shape[0] // 3)], path, reference=train)
                mine = []
                for k, ds in enumerate((train, valid)):
                    f = os.path.join(d, "%s_%d.bin" % (path[0], k))
                    ds.save_binary(f)
                    with open(f, "rb") as fh:
                        mine.append(fh.read())
                    os.remove(f)
                files.append(mine)
                del train, valid
        return all(f == files[0] for f in files[1:])

    result = {"tool": "bench_sparse_binning", "layout": args.layout, "host_threads": args.host_threads,
              "repeats": args.repeats, "shapes": [], "sweep": []}
    first = None
    for k, shape in enumerate(args.shapes):
        rows, cols, per_row = (int(v) for v in shape.split("x"))
        X = make_csr(rows, cols, per_row, 1 + k)
        if first is None:
            first = X  # (CSR: the sweep slices rows)
        if csc:
            X = X.tocsc()
        result["shapes"].append(measure(X))
        if args.equal_full and len(paths) > 1:
            result["shapes"][-1]["equal"] = files_equal(X)
        if csc and args.shuffle_column:
            device = [p for p in paths if p[0] == "device"]
            result["shapes"].append(measure(shuffled_column(X), device, "one column shuffled"))
        del X
    for rows in args.sweep:
        if first is not None and rows < first.shape[0]:
            result["sweep"].append(measure(first[:rows].tocsc() if csc else first[:rows]))
    if first is not None and len(paths) > 1:
        small = first[:min([first.shape[0]] + [r for r in args.sweep if r < first.shape[0]])]
        result["equal"] = files_equal(small.tocsc() if csc else small)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
