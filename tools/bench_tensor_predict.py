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

With --early-stop FREQ,MARGIN the booster has a binary objective and the routes are instead, on the
float32 tensor, raw scores: plain predict_device; predict_device(pred_early_stop=True) with FREQ and
MARGIN, with a margin that stops no row (the cost of the periods alone), with margin 0 (every row
stops at the first check), and with MARGIN and LGBM_AMD_TENSOR_STOP_COMPACT=0 (survivors left on
their lanes); and the host predictor with the same option on the tensor's host copy.  "stopped"
gives the share of rows that stop at each check, "equal" whether the device's early-stopped scores
are the host predictor's bits.

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
    ap.add_argument("--early-stop", default=None, metavar="FREQ,MARGIN")
    args = ap.parse_args()
    stop = None
    if args.early_stop:
        freq, margin = args.early_stop.split(",")
        stop = (int(freq), float(margin))

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

    def finish(out, routes, equal):
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
        out["equal"] = equal()
        print(json.dumps(out), file=sys.stderr, flush=True)  # (progress; the result line goes to stdout)
        return out

    def measure(rows, cols, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        X = torch.randn(rows, cols, generator=g, device="cuda", dtype=torch.float32)
        w = torch.randn(cols, generator=g, device="cuda") / cols ** 0.5
        n = min(rows, args.train_rows)
        y = (X[:n] @ w + 0.3 * torch.sin(3 * X[:n, 0]) * X[:n, cols - 1]).cpu().numpy()
        if stop:
            y = (y > 0).astype("float32")
        params = {"objective": "binary" if stop else "regression", "device_type": "gpu", "num_leaves": args.leaves, "max_bin": 63,
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

        def stopped(margin, compact=True, T=X):
            if not compact:
                os.environ["LGBM_AMD_TENSOR_STOP_COMPACT"] = "0"
            try:
                return bst.predict_device(T, raw_score=True, pred_early_stop=True, pred_early_stop_freq=stop[0],
                                          pred_early_stop_margin=margin)
            finally:
                os.environ.pop("LGBM_AMD_TENSOR_STOP_COMPACT", None)

        if stop:
            host = X.cpu().numpy()
            routes = {"host_round_trip": lambda: bst.predict(host, raw_score=True, pred_early_stop=True,
                                                             pred_early_stop_freq=stop[0], pred_early_stop_margin=stop[1]),
                      "predict_device": lambda: bst.predict_device(X, raw_score=True),
                      "stop": lambda: stopped(stop[1]), "stop_none": lambda: stopped(1e300),
                      "stop_all_at_first": lambda: stopped(0.0), "stop_no_compaction": lambda: stopped(stop[1], False)}
            iterations, alive, shares = bst.num_trees(), torch.ones(rows, dtype=torch.bool, device="cuda"), []
            for check in range(stop[0], iterations, stop[0]):
                over = 2 * bst.predict_device(X, raw_score=True, num_iteration=check)[:, 0].abs() > stop[1]
                shares.append(round(float((alive & over).sum()) / rows, 4))
                alive &= ~over
            out.update(early_stop={"freq": stop[0], "margin": stop[1]}, stopped=shares, never=round(float(alive.sum()) / rows, 4))
            return finish(out, routes, lambda: bool(torch.equal(routes["stop"]().cpu()[:, 0], torch.from_numpy(routes["host_round_trip"]()))))

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

        ref = ops.forest_predict(bst, X)
        return finish(out, routes, lambda: all(bool(torch.equal(f(), ref)) for f in (
            routes["predict_device_float32"], routes["predict_device_float32_colmajor"], routes["slots_float32"])))

    result = {"tool": "bench_tensor_predict", "repeats": args.repeats, "shapes": []}
    for k, shape in enumerate(args.shapes):
        rows, cols = (int(v) for v in shape.split("x"))
        result["shapes"].append(measure(rows, cols, 1 + k))
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
