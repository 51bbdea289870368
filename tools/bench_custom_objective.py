"""Milliseconds per boosting iteration of an objective written in torch, three ways, on a booster
trained with device_type=gpu (by default 1M and 10M rows x 28 columns, 63 leaves, 255 bins):

  builtin   the built-in objective (regression / binary): nothing leaves the GPU
  unmarked  fobj without the mark: the scores are downloaded to NumPy, the callable moves them to
            the GPU, computes there and brings float32 gradients back to NumPy, which are uploaded
  marked    the same arithmetic under lightgbmv1_amd.on_device: the scores arrive as a GPU tensor,
            the gradients are returned as GPU tensors (src/device/custom_kernels.hip)

  python tools/bench_custom_objective.py
  python tools/bench_custom_objective.py --rows 1000000 --objectives l2 --modes builtin marked

Every shape runs in a child process of its own under a time limit (--step-timeout).  A child
bins the matrix once and trains one booster per (objective, mode): --warmup iterations, then
--repeats windows of --steps iterations, each between a synchronise of torch and of the learner's
device; the figure is the median window over its steps.  Prints one JSON line per shape and one
with everything.  --trace-iterations N instead trains N marked iterations and nothing else (for a
kernel trace of that path).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_data(rows, cols, seed):
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((rows, cols)).astype(np.float32)
    z = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + np.sin(2 * X[:, 3]) + 0.3 * rng.standard_normal(rows)
    return X, z.astype(np.float32)


def objectives(torch, lgb, label):
    """name -> (built-in objective, torch gradients of (scores, label))"""
    def l2(p, y):
        return p - y, torch.ones_like(p)

    def logloss(p, y):
        q = torch.sigmoid(p)
        return q - y, q * (1.0 - q)

    return {"l2": ("regression", l2, label), "logloss": ("binary", logloss, (label > 0).to(label.dtype))}


def run_mode(lgb, torch, data, params, mode, grads, y, args):
    def unmarked(preds, ds):
        g, h = grads(torch.from_numpy(preds).cuda(), y)
        return g.float().cpu().numpy(), h.float().cpu().numpy()

    @lgb.on_device
    def marked(preds, ds):
        g, h = grads(preds, y)
        return g.float(), h.float()

    fobj = {"builtin": None, "unmarked": unmarked, "marked": marked}[mode]
    booster = lgb.Booster(params=params, train_set=data)

    def sync():
        torch.cuda.synchronize()
        lgb.device_synchronize()

    for _ in range(args.warmup):
        booster.update(fobj=fobj)
    windows = []
    for _ in range(args.repeats):
        sync()
        t = time.perf_counter()
        for _ in range(args.steps):
            booster.update(fobj=fobj)
        sync()
        windows.append((time.perf_counter() - t) * 1e3 / args.steps)
    return {"ms_per_iteration": statistics.median(windows), "min": min(windows), "max": max(windows),
            "iterations": booster.current_iteration()}


def step_shape(args):
    import torch

    import lightgbmv1_amd as lgb
    X, z = make_data(args.rows, args.cols, 1)
    label = torch.from_numpy(z.astype(np.float64)).cuda()
    objs = objectives(torch, lgb, label)
    out = {"rows": args.rows, "cols": args.cols}
    for name in args.objectives:
        builtin, grads, y = objs[name]
        params = {"objective": builtin, "device_type": "gpu", "num_leaves": args.leaves, "max_bin": args.max_bin,
                  "verbose": -1, "num_threads": args.host_threads, "boost_from_average": False}
        t = time.perf_counter()
        data = lgb.Dataset(X, y.cpu().numpy().astype(np.float32), params=params).construct()
        out.setdefault("dataset_seconds", {})[name] = time.perf_counter() - t
        if args.trace_iterations > 0:
            args.warmup, args.repeats, args.steps = 0, 1, args.trace_iterations
            out[name] = {"marked": run_mode(lgb, torch, data, params, "marked", grads, y, args)}
            continue
        res = {}
        for mode in args.modes:
            res[mode] = run_mode(lgb, torch, data, params, mode, grads, y, args)
            print("# %d rows %s %s: %s" % (args.rows, name, mode, json.dumps(res[mode])), file=sys.stderr, flush=True)
        if "unmarked" in res and "marked" in res:
            res["unmarked_over_marked"] = res["unmarked"]["ms_per_iteration"] / res["marked"]["ms_per_iteration"]
        if "builtin" in res and "marked" in res:
            res["marked_over_builtin"] = res["marked"]["ms_per_iteration"] / res["builtin"]["ms_per_iteration"]
        out[name] = res
        del data
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 10_000_000])
    ap.add_argument("--cols", type=int, default=28)
    ap.add_argument("--leaves", type=int, default=63)
    ap.add_argument("--max-bin", type=int, default=255)
    ap.add_argument("--objectives", nargs="*", default=["l2", "logloss"], choices=["l2", "logloss"])
    ap.add_argument("--modes", nargs="*", default=["builtin", "unmarked", "marked"],
                    choices=["builtin", "unmarked", "marked"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--trace-iterations", type=int, default=0)
    ap.add_argument("--step-timeout", type=float, default=400.0, help="seconds one shape may take")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        args.rows = args.rows[0]
        print(json.dumps(step_shape(args)))
        return
    result = {"tool": "bench_custom_objective", "leaves": args.leaves, "max_bin": args.max_bin, "warmup": args.warmup,
              "steps": args.steps, "repeats": args.repeats, "shapes": []}
    for rows in args.rows:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "--rows", str(rows), "--cols", str(args.cols),
               "--leaves", str(args.leaves), "--max-bin", str(args.max_bin), "--warmup", str(args.warmup),
               "--steps", str(args.steps), "--repeats", str(args.repeats), "--host-threads", str(args.host_threads),
               "--trace-iterations", str(args.trace_iterations), "--objectives"] + args.objectives + ["--modes"] + args.modes
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.step_timeout)
        if r.returncode != 0:
            raise SystemExit("bench_custom_objective.py: %d rows ended with status %d" % (rows, r.returncode))
        shape = json.loads(r.stdout.decode().strip().split("\n")[-1])
        print(json.dumps(shape), flush=True)
        result["shapes"].append(shape)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
