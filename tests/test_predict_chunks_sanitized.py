"""The chunk-size rule of device prediction (src/boosting/predict_chunks.h) under AddressSanitizer
+ UndefinedBehaviorSanitizer: tests/native/predict_chunks_driver.cpp, a stand-alone program of the
header alone (no device code, no HIP runtime), walks the table of tests/test_predict_chunks.py
with pointers that end at their last entry; any report fails.  As in
tests/test_score_convert_sanitized.py the program is a host-code check for machines without a GPU.
Skips where the compiler has no sanitizer runtimes."""
import os
import shutil
import subprocess

import pytest

import lightgbmv1_amd as lgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def test_predict_chunk_rule_clean_under_asan_ubsan(tmp_path):
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
    driver = tmp_path / "predict_chunks_driver"
    build = subprocess.run([cxx] + FLAGS + [os.path.join(ROOT, "tests", "native", "predict_chunks_driver.cpp"), "-o", str(driver)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(driver)], env=env, capture_output=True, text=True, timeout=60)
    log = out.stdout + out.stderr
    assert out.returncode == 0 and "predict chunks driver ok" in log, log[-4000:]
    assert "AddressSanitizer" not in log and "runtime error" not in log, log[-4000:]
