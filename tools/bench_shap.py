"""SHAP contribution throughput (pred_contrib) of the three prediction paths on a Higgs-shaped
model (28 features, 100 trees x 63 leaves by default), in rows per second:

  host    the host predictor (LGBM_AMD_HOST_PREDICT=1), one OpenMP thread per row
  capi    the device path of Booster.predict / LGBM_BoosterPredictForMat on a numpy matrix,
          host-to-device and device-to-host transfers included
  ops     lightgbmv1_amd.ops.forest_predict on a GPU tensor, result left on the GPU

  python tools/bench_shap.py                       # 10K, 100K and 1M rows
  python tools/bench_shap.py --rows 10000 --trees 20

Every path is warmed up once per row count, then timed --repeats times (median); a path whose
first timed run takes longer than --slow-s is timed once (its warm-up alone if that took four
times as long), and the host is not run above
--host-max-rows (it takes minutes per million rows).  Prints one JSON line; "ratio_eps_S" is
the largest |device - host| / (2**-52 * S) over the rows both computed (S: the sum over trees of
the largest |leaf value|, the tolerance scale of tests/helpers/contrib_cases.py).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats, slow_s):
    t = time.perf_counter()
    out = fn()  # warm-up
    times = []
    if time.perf_counter() - t > 4 * slow_s:  # (too slow to repeat: the warm-up is the measurement)
        times.append(time.perf_counter() - t)
    for _ in range(0 if times else repeats):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
        if times[-1] > slow_s:
            break
    return statistics.median(times), len(times), out


def device_predictions():
    import ctypes

    from lightgbmv1_amd import _native as nat
    out = ctypes.c_int64(0)
    nat.call("LGBM_AMD_DevicePredictCount", ctypes.byref(out))
    return out.value


def max_abs_leaf(node):
    if "leaf_value" in node:
        return abs(node["leaf_value"])
    return max(max_abs_leaf(node["left_child"]), max_abs_leaf(node["right_child"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--train-rows", type=int, default=500_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--leaves", type=int, default=63)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow-s", type=float, default=8.0)
    ap.add_argument("--host-max-rows", type=int, default=100_000)
    ap.add_argument("--host-threads", type=int, default=16)
    args = ap.parse_args()

    import torch

    import lightgbmv1_amd as lgb
    from lightgbmv1_amd import ops
    from lightgbmv1_amd.models.workloads import make_higgs

    if lgb.device_count() < 1:
        raise SystemExit("bench_shap.py needs a HIP device")
    Xt, yt, _ = make_higgs(args.train_rows)
    params = {"objective": "binary", "device_type": "gpu", "num_leaves": args.leaves, "max_bin": 63,
              "min_data_in_leaf": 20, "verbose": -1, "num_threads": args.host_threads}
    bst = lgb.train(params, lgb.Dataset(Xt, yt, params=params), num_boost_round=args.trees)
    scale = 2.0 ** -52 * sum(max_abs_leaf(t["tree_structure"]) for t in bst.dump_model()["tree_info"])
    result = {"tool": "bench_shap", "features": int(Xt.shape[1]), "trees": bst.num_trees(), "leaves": args.leaves,
              "host_threads": args.host_threads, "rows": {}}
    worst = 0.0
    for n in args.rows:
        X = make_higgs(n, start=args.train_rows)[0]
        Xd = torch.tensor(X, device="cuda")
        row = {}

        def run_ops():
            out = ops.forest_predict(bst, Xd, kind="contrib")
            torch.cuda.synchronize()
            return out

        # (train() hands back a booster reloaded from its model text, whose configuration is the
        # default: device_type=gpu in the predict parameters selects the device path)
        before = device_predictions()
        t, k, _ = timed(lambda: bst.predict(X, pred_contrib=True, device_type="gpu"), args.repeats, args.slow_s)
        if device_predictions() != before:
            row["capi"] = {"rows_per_s": n / t, "seconds": t, "runs": k}
        elif n < 1024:
            row["capi"] = "host (below the row gate of 1024)"
        else:
            raise SystemExit("the C API prediction did not run on the device")
        t, k, dev = timed(run_ops, args.repeats, args.slow_s)
        row["ops"] = {"rows_per_s": n / t, "seconds": t, "runs": k}
        if n <= args.host_max_rows:
            os.environ["LGBM_AMD_HOST_PREDICT"] = "1"
            try:
                t, k, host = timed(lambda: bst.predict(X, pred_contrib=True), args.repeats, args.slow_s)
            finally:
                del os.environ["LGBM_AMD_HOST_PREDICT"]
            row["host"] = {"rows_per_s": n / t, "seconds": t, "runs": k}
            row["ratio_eps_S"] = float(np.max(np.abs(dev.cpu().numpy() - host)) / scale)
            worst = max(worst, row["ratio_eps_S"])
        else:
            row["host"] = "not measured"
        result["rows"][str(n)] = row
        print("# %d rows: %s" % (n, json.dumps(row)), file=sys.stderr, flush=True)
    result["ratio_eps_S"] = worst
    print(json.dumps(result))


if __name__ == "__main__":
    main()
