#!/usr/bin/env python3
"""Record what the reference's command line program grows on the hand-built split cases
(tests/helpers/split_cases.py), for tests/test_split_ref.py.

Every case's rows go to a text file (label first, weights beside it), the oracle program that
oracle/build_ref.sh builds trains one tree on it (num_threads=1), and the tree section of its model
text is kept as JSON: one file per family under tests/golden/split_cases/, with the digest of the
case's rows.  The output is deterministic: a second run writes the same bytes.

usage: python oracle/record_split_cases.py [ORACLE_PROGRAM=oracle/_ref/lightgbm] [CASE_PREFIX ...]
"""
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import split_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "split_cases")
KEPT = ("num_leaves", "split_feature", "split_gain", "threshold", "decision_type", "left_child", "right_child",
        "leaf_value", "leaf_count", "internal_value", "internal_count", "cat_boundaries", "cat_threshold")


def _value(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (list, tuple)):
        return ",".join(_value(x) for x in v)
    return repr(v) if isinstance(v, float) else str(v)


def record(case, program, tmp):
    data = os.path.join(tmp, case.name + ".tsv")
    X, y = case.X(), case.label()
    with open(data, "w") as f:
        for i in range(len(y)):
            f.write("\t".join([repr(float(y[i]))] + ["nan" if math.isnan(v) else repr(float(v)) for v in X[i]]) + "\n")
    with open(data + ".weight", "w") as f:
        f.write("\n".join(repr(float(w)) for w in case.weight()) + "\n")
    params = dict(case.train_params(), task="train", data=data, output_model=data + ".model", num_iterations=1,
                  label_column=0, header=False, device_type="cpu", deterministic=True)
    cat = case.categorical_features()
    if cat:
        params["categorical_feature"] = cat
    conf = data + ".conf"
    with open(conf, "w") as f:
        f.write("".join("%s = %s\n" % (k, _value(v)) for k, v in sorted(params.items())))
    run = subprocess.run([program, "config=" + conf], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if run.returncode != 0:
        raise RuntimeError("%s: the oracle failed\n%s" % (case.name, run.stdout[-2000:]))
    with open(data + ".model") as f:
        tree = C.model_tree(f.read())
    return {"digest": case.digest(), "tree": {k: tree[k] for k in KEPT}}


def main(argv):
    program = os.path.join(ROOT, "oracle", "_ref", "lightgbm")
    if argv and os.path.isfile(argv[0]):
        program, argv = argv[0], argv[1:]
    if not os.access(program, os.X_OK):
        sys.exit("no oracle program at %s: build it with oracle/build_ref.sh" % program)
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for family in C.FAMILIES:
            cases = [c for c in C.CASES if c.family == family and (not argv or any(c.name.startswith(a) for a in argv))]
            if not cases:
                continue
            path = os.path.join(OUT, family + ".json")
            done = {}
            if argv and os.path.isfile(path):
                with open(path) as f:
                    done = json.load(f)
            for c in cases:
                done[c.name] = record(c, program, tmp)
                print("recorded", c.name, "leaves", done[c.name]["tree"]["num_leaves"])
            ordered = {c.name: done[c.name] for c in C.CASES if c.name in done}
            with open(path, "w") as f:
                f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in ordered.items())
                        + "\n}\n")


if __name__ == "__main__":
    main(sys.argv[1:])
