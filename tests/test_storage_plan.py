"""The rule that plans the device build of the learner's binned rows (src/device/storage_plan.h)
through LGBM_AMD_StoragePlan, against a table worked out by hand; no GPU.  The same table runs
under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program of the header alone
(tests/native/storage_plan_driver.cpp), as tests/test_predict_chunks_sanitized.py does for its rule."""
import ctypes
import os
import shutil
import subprocess

import pytest

import lightgbmv1_amd as lgb
from lightgbmv1_amd._native import call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
GiB, MiB = 1 << 30, 1 << 20

# (rows, column bytes per row, row bytes, free bytes, keep) ->
# (kept, window rows, window stride, window bytes, staging bytes, windows).  A quarter of what is
# free beside the resident images is the share; the staging is a quarter of it within [4 KiB, 64 MiB]
CASES = {
    "kept at 8 GiB": ((GiB, 8, 8, 48 * GiB, -1), (1, GiB, GiB, 0, 64 * MiB, 1)),
    "one row past 8 GiB": ((GiB + 1, 8, 8, 48 * GiB, -1), (0, GiB + 1, GiB + 4, 8 * GiB + 32, 64 * MiB, 1)),
    # share 14096 - staging 4096 = 10000 bytes: 1000 rows of 10 bytes; one byte of share less: 2 x 500
    "window fits exactly": ((1000, 10, 0, 56384, 0), (0, 1000, 1000, 10000, 4096, 1)),
    "window halved": ((1000, 10, 0, 56000, 0), (0, 500, 500, 5000, 4096, 2)),
    "one row, kept": ((1, 40, 64, 0, -1), (1, 1, 4, 0, 4096, 1)),
    "one row, no memory": ((1, 40, 64, 0, 0), (0, 1, 4, 160, 4096, 1)),
    "stride product past 2^31": ((10**9, 40, 40, 256 * GiB, -1), (0, 10**9, 10**9, 4 * 10**10, 64 * MiB, 1)),
    "six windows of a billion rows": ((10**9, 40, 40, 64 * GiB, -1), (0, 166666667, 166666668, 6666666720, 64 * MiB, 6)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_storage_plan_table(name):
    (rows, col, row, free, keep), want = CASES[name]
    out = (ctypes.c_int64 * 6)()
    call("LGBM_AMD_StoragePlan", ctypes.c_int64(rows), ctypes.c_int64(col), ctypes.c_int64(row), ctypes.c_int64(free),
         ctypes.c_int(keep), out)
    assert tuple(out) == want


def test_storage_plan_clean_under_asan_ubsan(tmp_path):
    n = lgb.device_count()
    if n > 0:
        pytest.skip("host-code sanitizer programs run on machines without a GPU, found %d HIP device(s)" % n)
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no AddressSanitizer / UndefinedBehaviorSanitizer runtimes")
    driver = tmp_path / "storage_plan_driver"
    build = subprocess.run([cxx] + FLAGS + [os.path.join(ROOT, "tests", "native", "storage_plan_driver.cpp"), "-o", str(driver)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(driver)], env=env, capture_output=True, text=True, timeout=60)
    log = out.stdout + out.stderr
    assert out.returncode == 0 and "storage plan driver ok" in log, log[-4000:]
    assert "AddressSanitizer" not in log and "runtime error" not in log, log[-4000:]
