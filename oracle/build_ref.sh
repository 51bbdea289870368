#!/bin/bash
# Golden oracle: the reference's CPU command line program built from
# its sources in a scratch copy (USE_GPU=OFF), for tests/test_golden.py.  Nothing prebuilt from
# the reference is used.  The copy and the build tree are made under oracle/_ref/, which is
# kept out of git, and removed when the script ends, whether the build succeeded or not: only
# the program and the two logs stay.
# usage: oracle/build_ref.sh REFERENCE_CHECKOUT [OUT_DIR=oracle/_ref]
set -e
REF=${1:?usage: oracle/build_ref.sh REFERENCE_CHECKOUT [OUT_DIR]}
OUT=${2:-$(dirname "$0")/_ref}
if [ -x "$OUT/lightgbm" ]; then echo "$OUT/lightgbm"; exit 0; fi
rm -rf "$OUT" && mkdir -p "$OUT"
trap 'rm -rf "$OUT/build" "$OUT/src" "$OUT/include" "$OUT/CMakeLists.txt"' EXIT
cp -r "$REF/CMakeLists.txt" "$REF/src" "$REF/include" "$OUT/"
chmod -R u+w "$OUT"
cmake -S "$OUT" -B "$OUT/build" -DUSE_GPU=OFF -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=Release > "$OUT/cmake.log" 2>&1
make -C "$OUT/build" -j"${JOBS:-6}" lightgbm > "$OUT/make.log" 2>&1
# the program runs: without arguments it reads its (empty) parameters and asks for data
if ! "$OUT/lightgbm" 2>&1 | grep -q "No training/prediction data"; then
  echo "oracle/build_ref.sh: $OUT/lightgbm was built but does not run" >&2
  rm -f "$OUT/lightgbm"
  exit 1
fi
echo "$OUT/lightgbm"
