"""bench.py's command line on the CPU learner at a small size: a plain run times exactly --steps
steps and reports ms_per_step without the held-out AUC, --dump-outputs writes the last step's
outputs as float32/float64 .npy files, and --full adds the AUC fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--device", "cpu", "--rows", "20000", "--test-rows", "2000", "--params", '{"num_threads": 2}']


def _bench(tmp_path, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(args), cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_outputs(tmp_path):
    dump = tmp_path / "dump"
    rec = _bench(tmp_path, "--steps", "3", "--warmup", "2", "--dump-outputs", str(dump))
    assert rec["steps"] == 3 and rec["warmup"] == 2 and rec["trees"] == 5
    assert rec["unit"] == "s/iter" and rec["higher_is_better"] is False
    assert rec["ms_per_step"] > 0
    assert abs(rec["ms_per_step"] - 1000.0 * rec["value"]) <= 1e-3
    assert not any(k.startswith("auc") for k in rec), sorted(rec)
    arrays = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    pred, rows = arrays["train_pred"], arrays["train_pred_rows"]
    assert pred.shape == rows.shape == (20000,)
    assert np.array_equal(rows, np.arange(20000)) and np.all((pred > 0) & (pred < 1))
    leaves = arrays["last_tree_leaf_value"]
    assert 2 <= len(leaves) <= 63 and np.all(np.isfinite(leaves))
    assert arrays["last_tree_leaf_count"].sum() == 20000
    for k in ("split_feature", "threshold", "left_child", "right_child"):
        assert arrays["last_tree_" + k].shape == (len(leaves) - 1,), k
    assert arrays["last_tree_split_feature"].max() < 28


def test_full_run_adds_heldout_auc(tmp_path):
    rec = _bench(tmp_path, "--steps", "3", "--warmup", "2", "--full")
    assert rec["ms_per_step"] > 0 and rec["trees"] == 5
    assert rec["auc_heldout"] > 0.7
    assert "auc_ref" in rec and "auc_delta" in rec
    assert not os.listdir(tmp_path)


@pytest.mark.gpu
def test_device_dumps_repeat_run_to_run(tmp_path, gpu_available):
    """Two device runs with the same arguments train on the same rows and leave the same outputs,
    so that two builds can be compared file by file."""
    args = ["--gpus", "1", "--rows", "100000", "--steps", "3", "--warmup", "1"]
    # (the two runs go side by side: most of a run this small is start-up)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / d)],
                              cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for d in ("a", "b")]
    recs = []
    for p in procs:
        stdout, stderr = p.communicate(timeout=300)
        assert p.returncode == 0, stdout[-2000:] + stderr[-3000:]
        recs.append(json.loads([l for l in stdout.splitlines() if l.startswith("{")][-1]))
    assert all(r["steps"] == 3 and r["trees"] == 4 and r["ms_per_step"] > 0 for r in recs)
    assert not any(k.startswith("auc") for k in recs[0])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "train_pred.npy" in names and "last_tree_leaf_value.npy" in names
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f
    assert np.load(tmp_path / "a" / "train_pred.npy").shape == (100000,)
