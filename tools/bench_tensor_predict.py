"""Prediction time of a GPU tensor, in seconds, by every route the package has for it:

  host_round_trip  Booster.predict(X): the tensor copied to the host, predicted there or uploaded
                   again (device_type=gpu), NumPy back
  forest_predict   ops.forest_predict(X.float().contiguous()), the conversion included (for a
                   contiguous float32 tensor it is free): k_predict_forest, one thread per row
  predict_device   Booster.predict_device(X) for float32, float64, float16 and bfloat16 tensors, each
                   row-major and column-major (src/device/tensor_predict_kernels.hip), raw scores, and
                   once through the objective's output transform
  slots            the same call with LGBM_AMD_TENSOR_PREDICT_SLOTS=1: the compact slot matrix and
                   k_predict_forest, float32 in both layouts

for seeded tensors of --shapes rows x cols (default 10M x 28 and 1M x 2000) and a booster of --trees
trees of --leaves leaves trained on the first --train-rows rows.  Every route ends in a device
synchronise or a copy to the host before it returns, so the host clock around a call covers the
device work.  The routes alternate inside one run after a warm-up of each; the median, the spread
(max - min) and every time of --repeats are reported.  "equal" tells whether predict_device and
the slots route gave the bits of forest_predict on the float32 tensor.  Prints one JSON line.

  python tools/bench_tensor_predict.py
  python tools/bench_tensor_predict.py --shapes 2000000x200 --repeats 5
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["10000000x28", "1000000x2000"])
    ap.add_argument("--trees", type=int, default=500)
    ap.add_argument("--leaves", type=int, default=63)
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    args = ap.parse_args()

    import torch

    import lightgbmv1_amd as lgb
    from lightgbmv1_amd import ops

    if lgb.device_count() < 1:
        raise SystemExit("bench_tensor_predict.py needs a HIP device")

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def measure(rows, cols, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        X = torch.randn(rows, cols, generator=g, device="cuda", dtype=torch.float32)
        w = torch.randn(cols, generator=g, device="cuda") / cols ** 0.5
        n = min(rows, args.train_rows)
        y = (X[:n] @ w + 0.3 * torch.sin(3 * X[:n, 0]) * X[:n, cols - 1]).cpu().numpy()
        params = {"objective": "regression", "device_type": "gpu", "num_leaves": args.leaves, "max_bin": 63,
                  "min_data_in_leaf": 5, "verbose": -1}
        bst = lgb.train(params, lgb.Dataset(X[:n].contiguous(), label=y, params=params), num_boost_round=args.trees)
        used = sum(1 for v in bst.feature_importance() if v > 0)
        plan = ops.tensor_predict_launch_info()
        out = {"rows": rows, "cols": cols, "trees": bst.num_trees(), "slots": used, "launch_info": plan}

        def slots(T):
            os.environ["LGBM_AMD_TENSOR_PREDICT_SLOTS"] = "1"
            try:
                return bst.predict_device(T, raw_score=True)
            finally:
                del os.environ["LGBM_AMD_TENSOR_PREDICT_SLOTS"]

        routes = {"host_round_trip": lambda: bst.predict(X, raw_score=True),
                  "forest_predict": lambda: ops.forest_predict(bst, X.float().contiguous())}
        tensors = {}
        for name, dtype in (("float32", torch.float32), ("float64", torch.float64), ("float16", torch.float16),
                            ("bfloat16", torch.bfloat16)):
            tensors[name] = X.to(dtype)
            tensors[name + "_colmajor"] = tensors[name].t().contiguous().t()
        for name, T in tensors.items():
            routes["predict_device_" + name] = lambda T=T: bst.predict_device(T, raw_score=True)
        routes["predict_device_float32_transformed"] = lambda: bst.predict_device(X)
        routes["slots_float32"] = lambda: slots(tensors["float32"])
        routes["slots_float32_colmajor"] = lambda: slots(tensors["float32_colmajor"])
        routes["forest_predict_float16_converted"] = lambda: ops.forest_predict(bst, tensors["float16"].float().contiguous())

        times = {k: [] for k in routes}
        for rep in range(args.repeats + 1):  # (the first round warms every route up)
            for k, f in routes.items():
                if k == "host_round_trip" and rep > args.host_repeats:
                    continue
                dt, _ = timed(f)
                if rep > 0:
                    times[k].append(dt)
        for k, v in times.items():
            out[k] = {"median_s": round(statistics.median(v), 5), "spread_s": round(max(v) - min(v), 5),
                      "all": [round(x, 5) for x in v]}
        ref = ops.forest_predict(bst, X)
        out["equal"] = all(bool(torch.equal(f(), ref)) for f in (
            routes["predict_device_float32"], routes["predict_device_float32_colmajor"], routes["slots_float32"]))
        print(json.dumps(out), file=sys.stderr, flush=True)  # (progress; the result line goes to stdout)
        return out

    result = {"tool": "bench_tensor_predict", "repeats": args.repeats, "shapes": []}
    for k, shape in enumerate(args.shapes):
        rows, cols = (int(v) for v in shape.split("x"))
        result["shapes"].append(measure(rows, cols, 1 + k))
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
