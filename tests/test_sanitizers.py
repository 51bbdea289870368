"""Host-code sanitizer run: the CLI built with AddressSanitizer +
UndefinedBehaviorSanitizer (`make sanitize`, built by the first test that needs it, ~1 min on
8 cores) trains the reference's example configs (conftest.py's ``example_data``) on the CPU
learner; any ASan / UBSan report fails the test.  The instrumented programs are host-code checks
for machines without a GPU: where a HIP device is visible the tests skip before building anything
(device code is never instrumented, and the sanitizer runtimes are kept away from the GPU driver
stack)."""
import fcntl
import os
import shutil
import subprocess

import pytest

import lightgbmv1_amd as lgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_CLI = os.path.join(ROOT, "build_asan", "lightgbm")


def _build(target, path):
    # (make is incremental: an up-to-date build returns at once, a stale one is rebuilt).  Under
    # pytest-xdist several workers get here at once: an exclusive lock makes one build while the
    # others wait, so none runs a binary another is still linking
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".sanitize.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            subprocess.run(["make", "-j" + str(min(8, os.cpu_count() or 4)), target], cwd=ROOT, check=True,
                           capture_output=True, timeout=1500)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    assert os.path.isfile(path), target


@pytest.fixture(scope="module")
def host_only():
    n = lgb.device_count()
    if n > 0:
        pytest.skip("host-code sanitizer programs run on machines without a GPU, found %d HIP device(s)" % n)


@pytest.fixture(scope="module")
def asan_cli(host_only):
    _build("sanitize", ASAN_CLI)
    return ASAN_CLI


@pytest.mark.parametrize("example,extra", [("binary_classification", ["num_trees=10"]),
                                           ("regression", ["num_trees=10"]),
                                           ("lambdarank", ["num_trees=5"])])
def test_examples_clean_under_asan_ubsan(tmp_path, asan_cli, example_data, example, extra):
    work = tmp_path / example
    shutil.copytree(os.path.join(example_data, example), work)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([asan_cli, "config=train.conf", "output_model=" + str(tmp_path / "m.txt")] + extra,
                         cwd=work, env=env, capture_output=True, text=True, timeout=600)
    log = out.stdout + out.stderr
    assert out.returncode == 0, log[-4000:]
    assert "AddressSanitizer" not in log and "runtime error" not in log, log[-4000:]
    assert (tmp_path / "m.txt").exists()


GROWTH_DRIVER = os.path.join(ROOT, "build_asan", "growth_plan_driver")


def test_growth_plan_clean_under_asan_ubsan(host_only):
    """The device learner's growth rules and the JSON glue of LGBM_AMD_GrowthPlan
    (src/treelearner/growth_plan.cpp, plain C++) with a few rows of tests/test_growth_plan.py's
    table (tests/native/growth_plan_driver.cpp), as a stand-alone instrumented program."""
    _build("build_asan/growth_plan_driver", GROWTH_DRIVER)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([GROWTH_DRIVER], env=env, capture_output=True, text=True, timeout=60)
    log = out.stdout + out.stderr
    assert out.returncode == 0 and "growth plan driver ok" in log, log[-4000:]
    assert "AddressSanitizer" not in log and "runtime error" not in log, log[-4000:]


TSAN_DRIVER = os.path.join(ROOT, "build_tsan", "tsan_driver")


def test_threads_clean_under_tsan(tmp_path, host_only, example_data):
    """ThreadSanitizer (`make tsan`): two_round loading's reader thread, and training under the
    booster's exclusive lock while three threads predict and one reads evaluations through the
    C API (tests/native/tsan_driver.cpp).  Found and fixed with it: the log level written by
    every C API call, and booster getters reading the model without the lock."""
    _build("tsan", TSAN_DRIVER)
    env = dict(os.environ, OMP_NUM_THREADS="1", TSAN_OPTIONS="exitcode=66 halt_on_error=0")
    out = subprocess.run([TSAN_DRIVER, os.path.join(example_data, "binary_classification", "binary.train"), "28"],
                         cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    log = out.stdout + out.stderr
    assert "ThreadSanitizer" not in log, log[-6000:]
    assert out.returncode == 0 and "tsan driver ok: 15 iterations, row-wise boosters 5 / 5" in log, log[-3000:]
