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

  python tools/bench_sparse_binning.py
  python tools/bench_sparse_binning.py --shapes 200000x2000x40 --sweep
  rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_binning.py --shapes 1000000x2000x40 \\
      --sweep --modes 1 --repeats 1       # (the kernels of the device path alone)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["1000000x2000x40", "10000000x40x4"])
    ap.add_argument("--sweep", nargs="*", type=int, default=[400_000, 100_000, 25_000, 6_000],
                    help="row counts of the first shape timed as well")
    ap.add_argument("--modes", nargs="*", default=["0", "1"], choices=["0", "1"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    args = ap.parse_args()

    import lightgbmv1_amd as lgb

    if lgb.device_count() < 1:
        raise SystemExit("bench_sparse_binning.py needs a HIP device")
    params = {"objective": "regression", "device_type": "gpu", "max_bin": 255, "verbose": -1,
              "num_threads": args.host_threads}

    def build(X, mode, reference=None):
        os.environ["LGBM_AMD_DEVICE_BINNING"] = mode
        before = csr_calls()
        t = time.perf_counter()
        ds = lgb.Dataset(X, params=params if reference is None else None, reference=reference).construct()
        dt = time.perf_counter() - t
        if (csr_calls() != before) != (mode == "1"):
            raise SystemExit("LGBM_AMD_DEVICE_BINNING=%s did not choose the path" % mode)
        return dt, ds

    def measure(X):
        out = {"rows": X.shape[0], "cols": X.shape[1], "entries": int(X.nnz)}
        times = {(m, k): [] for m in args.modes for k in ("train", "valid")}
        for rep in range(args.repeats + 1):  # (the first round warms both paths up)
            for mode in args.modes:
                dt, train = build(X, mode)
                dv, valid = build(X, mode, reference=train)
                if rep > 0:
                    times[(mode, "train")].append(dt)
                    times[(mode, "valid")].append(dv)
                del train, valid
        for (mode, kind), v in times.items():
            out["%s_%s_s" % ("host" if mode == "0" else "device", kind)] = round(statistics.median(v), 4)
        print(json.dumps(out), file=sys.stderr, flush=True)  # (progress; the result line goes to stdout)
        return out

    result = {"tool": "bench_sparse_binning", "host_threads": args.host_threads, "repeats": args.repeats,
              "shapes": [], "sweep": []}
    first = None
    for k, shape in enumerate(args.shapes):
        rows, cols, per_row = (int(v) for v in shape.split("x"))
        X = make_csr(rows, cols, per_row, 1 + k)
        if first is None:
            first = X
        result["shapes"].append(measure(X))
        del X
    for rows in args.sweep:
        if first is not None and rows < first.shape[0]:
            result["sweep"].append(measure(first[:rows]))
    if first is not None and len(args.modes) == 2:
        small = first[:min([first.shape[0]] + [r for r in args.sweep if r < first.shape[0]])]
        files = []
        with tempfile.TemporaryDirectory() as d:
            for mode in ("0", "1"):
                _, ds = build(small, mode)
                ds.save_binary(os.path.join(d, mode + ".bin"))
                with open(os.path.join(d, mode + ".bin"), "rb") as f:
                    files.append(f.read())
        result["equal"] = files[0] == files[1]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
