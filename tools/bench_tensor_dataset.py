"""Construction time of a Dataset from a GPU tensor, in seconds, two ways:

  host     lgb.Dataset(X.cpu().numpy()): the tensor copied to the host and built as a host matrix
           (LGBM_AMD_DEVICE_BINNING unset: DeviceBinDenseMatrix uploads it again from 4M values on) --
           what a GPU tensor went through before it was read in place
  device   lgb.Dataset(X) with LGBM_AMD_DEVICE_BINNING=1 (the path at every size):
           LGBM_AMD_DatasetCreateFromDeviceMat (src/device/tensor_bin_kernels.hip)

each as the training set (the row sample and the bin mappers, then the binning) and as a
reference= set (the binning alone), for seeded float32 tensors of --shapes rows x cols (default
10M x 28 and 1M x 2000) and for --sweep row counts at 28 columns, with and without two
categorical columns.  Both ways end in blocking device-to-host copies, so the host clock around a
construction covers the device work.  The two alternate inside one run after a warm-up of each;
the median and every time of --repeats are reported.  "equal" tells whether both ways saved the
same binary file (checked on the smallest sweep entry).  Prints one JSON line.

With --bin-find the tool measures the training set of the device way alone, with the first step of
the bin finder (the sort of each column's sample and its distinct values) on the host
(LGBM_AMD_DEVICE_BIN_FIND=0: the path before src/device/bin_find_kernels.hip) and on the device (=1),
alternating, for --shapes and for --gate entries (rows x cols with rows below
bin_construct_sample_cnt, so that rows is the sample size).  Host timers (LGBM_AMD_TIMETAG=1,
lgb.get_timers) split each construction into: sample (gather, copy and zero filter; with =1 also the
wait for the device sort and the copy of the runs), sort and search (the wall time of the bin-finder
loop, divided by the thread time its two halves took; with =1 the loop is the search alone), bundle
(feature bundling and the dataset's layout) and bin (the binning of the whole tensor).

  python tools/bench_tensor_dataset.py
  python tools/bench_tensor_dataset.py --shapes --sweep 1000 10000 100000
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["10000000x28", "1000000x2000"])
    ap.add_argument("--sweep", nargs="*", type=int, default=[1_000, 10_000, 100_000, 1_000_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--bin-find", action="store_true")
    ap.add_argument("--gate", nargs="*", default=[])
    args = ap.parse_args()
    if args.bin_find:
        os.environ["LGBM_AMD_TIMETAG"] = "1"  # (read when the library first looks at its timers)

    import torch

    import lightgbmv1_amd as lgb
    from lightgbmv1_amd import ops

    if lgb.device_count() < 1:
        raise SystemExit("bench_tensor_dataset.py needs a HIP device")
    params = {"objective": "regression", "device_type": "gpu", "max_bin": 255, "verbose": -1,
              "num_threads": args.host_threads}

    def make(rows, cols, categorical, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        X = torch.randn(rows, cols, generator=g, device="cuda", dtype=torch.float32)
        if categorical:
            X[:, :2] = torch.randint(0, 50, (rows, 2), generator=g, device="cuda").float()
        return X

    def build(X, way, cat, reference=None):
        os.environ.pop("LGBM_AMD_DEVICE_BINNING", None)
        if way == "device":
            os.environ["LGBM_AMD_DEVICE_BINNING"] = "1"
        before = ops.tensor_bin_stats()
        torch.cuda.synchronize()
        t = time.perf_counter()
        data = X.cpu().numpy() if way == "host" else X
        ds = lgb.Dataset(data, params=params if reference is None else None, reference=reference,
                         categorical_feature=[0, 1] if cat else "auto").construct()
        dt = time.perf_counter() - t
        if (ops.tensor_bin_stats() != before) != (way == "device"):
            raise SystemExit("way %s did not run as asked" % way)
        return dt, ds

    def measure(X, cat):
        out = {"rows": X.shape[0], "cols": X.shape[1], "categorical": cat}
        times = {(w, k): [] for w in ("host", "device") for k in ("train", "valid")}
        for rep in range(args.repeats + 1):  # (the first round warms both ways up)
            for way in ("host", "device"):
                dt, train = build(X, way, cat)
                dv, valid = build(X, way, cat, reference=train)
                if rep > 0:
                    times[(way, "train")].append(dt)
                    times[(way, "valid")].append(dv)
                del train, valid
        for (way, kind), v in times.items():
            out["%s_%s_s" % (way, kind)] = round(statistics.median(v), 5)
            out["%s_%s_all" % (way, kind)] = [round(x, 5) for x in v]
        print(json.dumps(out), file=sys.stderr, flush=True)  # (progress; the result line goes to stdout)
        return out

    def files_equal(X, cat):
        files = []
        with tempfile.TemporaryDirectory() as d:
            for way in ("host", "device"):
                _, train = build(X, way, cat)
                f = os.path.join(d, way + ".bin")
                train.save_binary(f)
                with open(f, "rb") as fh:
                    files.append(fh.read())
        return files[0] == files[1]

    def phases(before, after):
        d = {k: after.get(k, 0.0) - before.get(k, 0.0) for k in after}
        loop, sort, search = (d.get("Dataset::find_bins" + k, 0.0) for k in ("", "/sort_thread_time", "/search_thread_time"))
        share = sort / (sort + search) if sort + search > 0 else 0.0
        return {"sample": d.get("DeviceMat::sample", 0.0), "sort": loop * share, "search": loop * (1 - share),
                "bundle": d.get("Dataset::bundle_and_layout", 0.0), "bin": d.get("DeviceMat::bin", 0.0)}

    def measure_bin_find(X):
        out = {"rows": X.shape[0], "cols": X.shape[1]}
        runs = {"0": [], "1": []}
        for rep in range(args.repeats + 1):
            for knob in ("0", "1"):
                os.environ["LGBM_AMD_DEVICE_BIN_FIND"] = knob
                calls, timers = ops.tensor_bin_stats(bin_find=True), lgb.get_timers()
                dt, train = build(X, "device", False)
                if (ops.tensor_bin_stats(bin_find=True) != calls) != (knob == "1"):
                    raise SystemExit("LGBM_AMD_DEVICE_BIN_FIND=%s did not run as asked" % knob)
                if rep > 0:
                    runs[knob].append(dict(phases(timers, lgb.get_timers()), total=dt))
                del train
        os.environ.pop("LGBM_AMD_DEVICE_BIN_FIND", None)
        for knob, name in (("0", "host_sort"), ("1", "device_sort")):
            out[name + "_s"] = {k: round(statistics.median(r[k] for r in runs[knob]), 5) for k in runs[knob][0]}
            out[name + "_all"] = [round(r["total"], 5) for r in runs[knob]]
        print(json.dumps(out), file=sys.stderr, flush=True)
        return out

    if args.bin_find:
        result = {"tool": "bench_tensor_dataset --bin-find", "host_threads": args.host_threads,
                  "repeats": args.repeats, "shapes": [], "gate": []}
        for k, shape in enumerate(args.shapes + args.gate):
            rows, cols = (int(v) for v in shape.split("x"))
            result["shapes" if k < len(args.shapes) else "gate"].append(measure_bin_find(make(rows, cols, False, 1 + k)))
            torch.cuda.empty_cache()
        print(json.dumps(result))
        return

    result = {"tool": "bench_tensor_dataset", "host_threads": args.host_threads, "repeats": args.repeats,
              "shapes": [], "sweep": []}
    for k, shape in enumerate(args.shapes):
        rows, cols = (int(v) for v in shape.split("x"))
        X = make(rows, cols, False, 1 + k)
        result["shapes"].append(measure(X, False))
        del X
        torch.cuda.empty_cache()
    for rows in args.sweep:
        for cat in (False, True):
            result["sweep"].append(measure(make(rows, 28, cat, 7), cat))
    if args.sweep:
        result["equal"] = files_equal(make(min(args.sweep), 28, True, 7), True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
