"""Prediction time of a wide sparse matrix (1M rows x 2000 columns at 2% density by default,
float32; 100 trees x 63 leaves trained on the device on a sample of it) for raw scores, leaf
indices and SHAP contributions, through Booster.predict, in seconds:

  host    the host predictor on the CSR matrix (LGBM_AMD_HOST_PREDICT=1): what a CSR input cost
          before device CSR prediction
  dense   X.toarray() (timed, its own figure) and the dense device path on the result
  csr     the device path on the CSR matrix (src/device/csr_kernels.hip and the forest kernels)
  csc_host   the host predictor on the same matrix as CSC (converted once, outside the timed
          region): the transposition into rows, then the host predictor -- what a CSC input cost
          before device CSC prediction
  tocsr_csr  m.tocsr() inside the timed region, then the device CSR path: what a Python caller
          could do instead
  csc     the device path on the CSC matrix (src/device/csc_kernels.hip and the forest kernels);
          --shuffle-column stores one used column of it in shuffled order (the single-wave path)

  python tools/bench_sparse_predict.py
  python tools/bench_sparse_predict.py --rows 100000 --kinds raw --paths csr
  python tools/bench_sparse_predict.py --rows 50000 --kinds --save-model m.txt   # train only, then
  rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_predict.py --model m.txt --paths csr
                                                   # (a trace of the prediction kernels alone)

Contributions are rows x (columns + 1) doubles (16 GB at the default shape) on every path, so
they are measured on --contrib-rows rows.  Every path is warmed up once, then timed --repeats
times (median); a run slower than --slow-s is not repeated.  Prints one JSON line; "equal"
tells whether the csr path's raw scores and leaf indices equalled the host's and the dense path's,
and the csc path's those of every other path measured; "copied_bytes" is what the csr and csc
device paths copy to the device per call.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRED = {"raw": {"raw_score": True}, "leaf": {"pred_leaf": True}, "contrib": {"pred_contrib": True}}


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


def timed(fn, repeats, slow_s):
    t = time.perf_counter()
    out = fn()  # warm-up
    first = time.perf_counter() - t
    if first > slow_s:
        return first, 1, out
    times = []
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return statistics.median(times), len(times), out


def device_predictions():
    from lightgbmv1_amd import _native as nat
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DevicePredictCount", ctypes.byref(out))
    return out.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--contrib-rows", type=int, default=100_000)
    ap.add_argument("--cols", type=int, default=2000)
    ap.add_argument("--per-row", type=int, default=40)
    ap.add_argument("--train-rows", type=int, default=50_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--leaves", type=int, default=63)
    ap.add_argument("--kinds", nargs="*", default=["raw", "leaf", "contrib"], choices=list(PRED))
    ap.add_argument("--paths", nargs="*", default=["host", "dense", "csr"],
                    choices=["host", "dense", "csr", "csc_host", "tocsr_csr", "csc"])
    ap.add_argument("--shuffle-column", action="store_true",
                    help="store the longest used column of the CSC matrix in shuffled order")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slow-s", type=float, default=20.0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--save-model", help="write the trained model here")
    ap.add_argument("--model", help="predict with this model file instead of training one")
    args = ap.parse_args()

    import lightgbmv1_amd as lgb

    if lgb.device_count() < 1:
        raise SystemExit("bench_sparse_predict.py needs a HIP device")
    X = make_csr(args.rows, args.cols, args.per_row, 1)
    if args.model:
        bst = lgb.Booster(model_file=args.model)
    else:
        sample = X[:args.train_rows].toarray()
        w = np.random.RandomState(2).standard_normal(args.cols) * (np.random.RandomState(3).rand(args.cols) < 0.25)
        y = sample @ w + np.sin(3 * sample[:, : args.cols // args.per_row].sum(axis=1))
        params = {"objective": "regression", "device_type": "gpu", "num_leaves": args.leaves, "max_bin": 63,
                  "min_data_in_leaf": 20, "verbose": -1, "num_threads": args.host_threads}
        bst = lgb.train(params, lgb.Dataset(sample, y, params=params), num_boost_round=args.trees)
        del sample
        if args.save_model:
            bst.save_model(args.save_model)
    used = int(np.count_nonzero(bst.feature_importance()))
    result = {"tool": "bench_sparse_predict", "rows": args.rows, "contrib_rows": args.contrib_rows, "cols": args.cols,
              "density": args.per_row / args.cols, "trees": bst.num_trees(), "leaves": args.leaves,
              "used_features": used, "host_threads": args.host_threads, "kinds": {}, "equal": True}
    gpu = {"device_type": "gpu", "num_threads": args.host_threads}

    def on_device(fn):
        before = device_predictions()
        r = timed(fn, args.repeats, args.slow_s)
        if device_predictions() == before:
            raise SystemExit("the prediction did not run on the device")
        return r

    want_csc = any(p in args.paths for p in ("csc_host", "tocsr_csr", "csc"))
    csc_of = {}

    def as_csc(M):
        """M as CSC, converted once per matrix outside every timed region"""
        if id(M) not in csc_of:
            C = M.tocsc()
            if args.shuffle_column:
                cols = np.nonzero(bst.feature_importance())[0]
                c = cols[np.argmax(np.diff(C.indptr)[cols])]
                lo, hi = C.indptr[c], C.indptr[c + 1]
                perm = np.random.RandomState(4).permutation(hi - lo) + lo
                C.indices[lo:hi], C.data[lo:hi] = C.indices[perm], C.data[perm]
                C.has_sorted_indices = False
                result["shuffled_column_entries"] = int(hi - lo)
            csc_of[id(M)] = C
        return csc_of[id(M)]

    def copied_bytes(M, C):
        """bytes the device paths copy to the device per call: every stored entry and the row
        pointer (csr), the stored entries of the used columns and their pointer (csc)"""
        cols = np.nonzero(bst.feature_importance())[0]
        per = 4 + M.data.dtype.itemsize
        return {"csr": int(M.nnz * per + M.indptr.nbytes),
                "csc": int(np.diff(C.indptr)[cols].sum() * per + 8 * (len(cols) + 1) + 4 * len(cols))}

    for kind in args.kinds:
        M = X if kind != "contrib" else X[:args.contrib_rows]
        row = {"rows": M.shape[0]}
        outs = {}
        if want_csc:
            C = as_csc(M)
            row["copied_bytes"] = copied_bytes(M, C)
        if "csc" in args.paths:
            t, k, outs["csc"] = on_device(lambda: bst.predict(C, **PRED[kind], **gpu))
            row["csc"] = {"seconds": t, "runs": k}
        if "tocsr_csr" in args.paths:
            t, k, outs["tocsr_csr"] = on_device(lambda: bst.predict(C.tocsr(), **PRED[kind], **gpu))
            row["tocsr_csr"] = {"seconds": t, "runs": k}
            t, k, _ = timed(C.tocsr, args.repeats, args.slow_s)
            row["tocsr"] = {"seconds": t, "runs": k}
        if "csc_host" in args.paths:
            os.environ["LGBM_AMD_HOST_PREDICT"] = "1"
            try:
                t, k, outs["csc_host"] = timed(lambda: bst.predict(C, **PRED[kind], **gpu), args.repeats, args.slow_s)
            finally:
                del os.environ["LGBM_AMD_HOST_PREDICT"]
            row["csc_host"] = {"seconds": t, "runs": k}
        if "csr" in args.paths:
            t, k, outs["csr"] = on_device(lambda: bst.predict(M, **PRED[kind], **gpu))
            row["csr"] = {"seconds": t, "runs": k}
        if "dense" in args.paths:
            t, k, D = timed(M.toarray, 1, 0.0)
            row["toarray"] = {"seconds": t, "runs": k}
            t, k, outs["dense"] = on_device(lambda: bst.predict(D, **PRED[kind], **gpu))
            row["dense"] = {"seconds": t, "runs": k}
            del D
        if "host" in args.paths:
            os.environ["LGBM_AMD_HOST_PREDICT"] = "1"
            try:
                t, k, outs["host"] = timed(lambda: bst.predict(M, **PRED[kind], **gpu), args.repeats, args.slow_s)
            finally:
                del os.environ["LGBM_AMD_HOST_PREDICT"]
            row["host"] = {"seconds": t, "runs": k}
        if kind != "contrib" and "csr" in outs:
            for other in ("host", "dense"):
                if other in outs and not np.array_equal(outs["csr"], outs[other]):
                    result["equal"] = False
        if kind != "contrib" and "csc" in outs:
            for other in ("csc_host", "tocsr_csr", "csr", "host", "dense"):
                if other in outs and not np.array_equal(outs["csc"], outs[other]):
                    result["equal"] = False
        result["kinds"][kind] = row
        print("# %s: %s" % (kind, json.dumps(row)), file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
