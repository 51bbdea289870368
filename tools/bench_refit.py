"""Refit time of a device booster (device_type=gpu), host branch against device path, on the same
model and data: by default a binary model of 100 trees x 63 leaves refitted on 1M rows x 28
columns (float32).

  host    LGBM_AMD_HOST_REFIT=1: gradients downloaded every iteration, a CPU learner created per
          tree, a counting sort of the rows by leaf, and a tree walk for the score update
  device  per-leaf sums and the score update on the device over the staged leaf matrix
          (src/device/refit_kernels.hip)

  python tools/bench_refit.py
  python tools/bench_refit.py --rows 100000 --trees 20 --paths device

Every step that uses the GPU is a child process of its own under a time limit (--step-timeout):
training the model, then one child per path.  A child times, in seconds: the leaf matrix
(Booster.predict(pred_leaf=True)), the new booster over the refit data (binning and upload), and
the LGBM_BoosterRefit call itself -- the part the two paths differ in -- over --repeats fresh
boosters (median).  Prints one JSON line; "leaf_value_diff" is the largest difference of the two
paths' leaf values relative to the largest |leaf value| (the host branch's scores are wrong from
the second iteration on for a model merged from text: docs/ENVIRONMENT.md, LGBM_AMD_HOST_REFIT).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_data(rows, cols, seed):
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((rows, cols)).astype(np.float32)
    z = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + np.sin(2 * X[:, 3]) + 0.3 * rng.standard_normal(rows)
    return X, (z > 0).astype(np.float32)


def leaf_values(text):
    return np.concatenate([np.array(ln.split("=")[1].split(), dtype=np.float64)
                           for ln in text.split("\n") if ln.startswith("leaf_value=")])


def step_train(args):
    import lightgbmv1_amd as lgb
    X, y = make_data(args.rows, args.cols, 1)
    params = {"objective": "binary", "device_type": "gpu", "num_leaves": args.leaves, "max_bin": 63, "verbose": -1,
              "num_threads": args.host_threads}
    t = time.perf_counter()
    bst = lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=args.trees)
    bst.save_model(args.model)
    return {"train_seconds": time.perf_counter() - t, "trees": bst.num_trees()}


def step_refit(args):
    import lightgbmv1_amd as lgb
    from lightgbmv1_amd import _native as nat
    if args.path == "host":
        os.environ["LGBM_AMD_HOST_REFIT"] = "1"
    params = {"objective": "binary", "device_type": "gpu", "num_leaves": args.leaves, "max_bin": 63, "verbose": -1,
              "num_threads": args.host_threads, "refit_decay_rate": 0.9}
    base = lgb.Booster(model_file=args.model, params=params)
    X, y = make_data(args.rows, args.cols, 2)
    t = time.perf_counter()
    leaves = base.predict(X, pred_leaf=True, device_type="gpu").reshape(args.rows, -1)
    leaves = np.ascontiguousarray(leaves, dtype=np.int32)
    t_leaves = time.perf_counter() - t
    t = time.perf_counter()
    data = lgb.Dataset(X, y, params=params).construct()
    t_data = time.perf_counter() - t
    pred = base._to_predictor()
    times, t_booster, text = [], [], None
    for _ in range(args.repeats + 1):  # (the first one warms up)
        t = time.perf_counter()
        bst = lgb.Booster(params, data)
        nat.call("LGBM_BoosterMerge", bst.handle, pred.handle)
        t_booster.append(time.perf_counter() - t)
        t = time.perf_counter()
        nat.call("LGBM_BoosterRefit", bst.handle, leaves.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                 ctypes.c_int32(leaves.shape[0]), ctypes.c_int32(leaves.shape[1]))
        times.append(time.perf_counter() - t)
        text = bst.model_to_string()
        del bst
    with open(args.out_model, "w") as f:
        f.write(text)
    return {"leaf_matrix_seconds": t_leaves, "dataset_seconds": t_data, "booster_seconds": statistics.median(t_booster[1:]),
            "first_refit_seconds": times[0], "refit_seconds": statistics.median(times[1:]), "runs": len(times) - 1}


def child(args, step, timeout, **extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rows", str(args.rows), "--cols", str(args.cols),
           "--trees", str(args.trees), "--leaves", str(args.leaves), "--repeats", str(args.repeats),
           "--host-threads", str(args.host_threads), "--model", args.model]
    for k, v in extra.items():
        cmd += ["--" + k.replace("_", "-"), v]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("bench_refit.py: step %s ended with status %d" % (step, r.returncode))
    return json.loads(r.stdout.decode().strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=28)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--leaves", type=int, default=63)
    ap.add_argument("--paths", nargs="*", default=["host", "device"], choices=["host", "device"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--step-timeout", type=float, default=420.0, help="seconds a GPU step may take")
    ap.add_argument("--step", choices=["train", "refit"], help=argparse.SUPPRESS)
    ap.add_argument("--path", help=argparse.SUPPRESS)
    ap.add_argument("--model", help=argparse.SUPPRESS)
    ap.add_argument("--out-model", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        print(json.dumps(step_train(args) if args.step == "train" else step_refit(args)))
        return
    with tempfile.TemporaryDirectory(prefix="bench_refit_") as tmp:
        args.model = os.path.join(tmp, "model.txt")
        result = {"tool": "bench_refit", "rows": args.rows, "cols": args.cols, "leaves": args.leaves,
                  "host_threads": args.host_threads}
        result.update(child(args, "train", args.step_timeout))
        for path in args.paths:
            result[path] = child(args, "refit", args.step_timeout, path=path, out_model=os.path.join(tmp, path + ".txt"))
            print("# %s: %s" % (path, json.dumps(result[path])), file=sys.stderr, flush=True)
        if len(args.paths) == 2:
            a, b = (leaf_values(open(os.path.join(tmp, p + ".txt")).read()) for p in args.paths)
            result["leaf_value_diff"] = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
            result["speedup"] = result["host"]["refit_seconds"] / result["device"]["refit_seconds"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
