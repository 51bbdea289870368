"""Times the set-up of a device learner on an already constructed Dataset: the wall time of
``lgb.Booster(params, train_set)``, the storage-build phase of the LGBM_AMD_TIMETAG timers inside
it, the host memory it adds at its peak and the first tree.  The binned rows are built on the host
(LGBM_AMD_DEVICE_STORAGE=0), on the GPU (=1) or by the default rule (unset); the branches alternate
inside one process, after a warm-up of each, and every figure is the median of --repeats runs with
its min and max.  On a commit without the knob only the `unset` branch means anything.

    python tools/bench_learner_setup.py --shapes dense28,nibble28 --rows 10000000
    python tools/bench_learner_setup.py --shapes sweep28

Prints one JSON line per shape and branch and, at the end, a markdown table."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

os.environ.setdefault("LGBM_AMD_TIMETAG", "1")  # (read when the library loads)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import lightgbmv1_amd as lgb  # noqa: E402
from lightgbmv1_amd._native import call, read_string  # noqa: E402

KNOB = "LGBM_AMD_DEVICE_STORAGE"


def rss_bytes():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


class PeakRss:
    """The most resident memory above the level at entry, sampled every 5 ms."""

    def __enter__(self):
        self.base, self.peak, self.stop = rss_bytes(), 0, False
        self.thread = threading.Thread(target=self._run)
        self.thread.start()
        return self

    def _run(self):
        while not self.stop:
            self.peak = max(self.peak, rss_bytes() - self.base)
            time.sleep(0.005)

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()


def storage_phase_s():
    text = read_string(lambda size, need, buf: call("LGBM_AMD_GetTimers", size, need, buf), 1 << 14)
    total = 0.0
    for item in text.split(";"):
        if item.startswith("GPUTreeLearner::storage_build"):
            total += float(item.split("=")[1])
    return total


def make_shape(name, rows, rng):
    """(X, params, environment) of a shape; X may be a scipy CSR matrix."""
    params = {"objective": "binary", "device_type": "gpu", "verbose": -1, "num_leaves": 63, "min_data_in_leaf": 20}
    env = {}
    if name in ("dense28", "nibble28", "sweep28"):
        X = rng.standard_normal((rows, 28), dtype=np.float32)
        params["max_bin"] = 15 if name == "nibble28" else 63
        if name == "nibble28":
            env["LGBM_AMD_NIBBLE_BINS"] = "1"
    elif name == "dense2000":
        X = rng.integers(0, 64, (rows, 2000), dtype=np.uint8).astype(np.float32)
        params.update(max_bin=63, enable_bundle=False)
    elif name == "sparse":  # Criteo-shaped: 13 dense counts and 26 one-hot categoricals hashed to 2000 columns each
        import scipy.sparse as sp
        dense = sp.csr_matrix(rng.poisson(2.0, (rows, 13)).astype(np.float32))
        cols = rng.integers(0, 2000, (rows, 26)) + 2000 * np.arange(26)
        onehot = sp.csr_matrix((np.ones(rows * 26, np.float32), cols.reshape(-1), 26 * np.arange(rows + 1)),
                               shape=(rows, 52000))
        X = sp.hstack([dense, onehot], format="csr")
        params.update(max_bin=63)
        env["LGBM_AMD_SPARSE_ROWS"] = "1"
    else:
        raise SystemExit("unknown shape " + name)
    return X, params, env


def one_setup(params, train, branch):
    if branch == "unset":
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = branch
    phase0 = storage_phase_s()
    with PeakRss() as rss:
        t0 = time.perf_counter()
        booster = lgb.Booster(params=params, train_set=train)
        setup = time.perf_counter() - t0
    phase = storage_phase_s() - phase0
    t0 = time.perf_counter()
    booster.update()
    first_tree = time.perf_counter() - t0
    del booster
    return {"setup_s": setup, "storage_s": phase, "first_tree_s": first_tree, "peak_rss_gb": rss.peak / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dense28")
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--branches", default="0,1,unset")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if lgb.device_count() < 1:
        raise SystemExit("bench_learner_setup needs a GPU")
    branches = args.branches.split(",")
    table = []
    for name in args.shapes.split(","):
        sizes = [args.rows] if name != "sweep28" else [10000, 30000, 100000, 300000, 1000000, 3000000]
        for rows in sizes:
            rng = np.random.default_rng(7)
            X, params, env = make_shape(name, rows, rng)
            os.environ.update(env)
            y = (rng.random(rows) < 0.5).astype(np.float32)
            t0 = time.perf_counter()
            train = lgb.Dataset(X, y, params=params).construct()
            construct_s = time.perf_counter() - t0
            del X
            for b in branches:  # warm-up: code objects, allocator, page cache of the columns
                one_setup(params, train, b)
            runs = {b: [] for b in branches}
            for _ in range(args.repeats):
                for b in branches:
                    runs[b].append(one_setup(params, train, b))
            for b in branches:
                rec = {"shape": name, "rows": rows, "branch": b, "construct_s": round(construct_s, 2)}
                for key in ("setup_s", "storage_s", "first_tree_s", "peak_rss_gb"):
                    vals = [r[key] for r in runs[b]]
                    rec[key] = [round(statistics.median(vals), 4), round(min(vals), 4), round(max(vals), 4)]
                print(json.dumps(rec), flush=True)
                table.append(rec)
            for k in env:
                os.environ.pop(k)
            del train
    dev, host = ctypes.c_int64(0), ctypes.c_int64(0)
    if hasattr(lgb.basic._load_lib(), "LGBM_AMD_DeviceStorageStats"):
        call("LGBM_AMD_DeviceStorageStats", ctypes.byref(dev), ctypes.byref(host))
    print("builds: %d on the device, %d on the host" % (dev.value, host.value))
    print("| shape | rows | branch | Booster() s: median (min-max) | storage build s | first tree s | host peak GB |")
    print("|---|---|---|---|---|---|---|")
    for r in table:
        cell = lambda v: "%.3f (%.3f-%.3f)" % tuple(v)  # noqa: E731
        print("| %s | %d | %s | %s | %s | %s | %.2f |" % (r["shape"], r["rows"], r["branch"], cell(r["setup_s"]),
                                                         cell(r["storage_s"]), cell(r["first_tree_s"]), r["peak_rss_gb"][0]))


if __name__ == "__main__":
    main()
