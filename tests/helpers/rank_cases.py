"""The cases and bounds shared by the host checks (tests/test_rank_refs_host.py, no GPU) and the
device checks (tests/test_rank_ops.py) of the listwise objectives and query metrics against the
float64 references of tests/helpers/rank_refs.py.  References are computed once per process and
shared (functools.lru_cache); callers must not modify what they get.

Bounds (none is tuned to the code under test):

* LambdaRank: a document's gradient is a float sum of m_d float-rounded pair terms, rounded twice
  more by the normalisation and the weight: to first order the error is at most
  (m_d + 3) * 2^-24 * S_d, S_d the sum of the terms' absolute values.  Allowed:
  2 * (m_d + 3) * 2^-24 * S_d + 1e-12 (the factor 2: second-order terms and the last bit of exp in
  the sigmoid table).  Where the reference is exactly 0 the result must be exactly 0.
* XE-NDCG: the gradient is three float roundings and two float adds over the reference's three
  terms: 2^-21 * (|t1| + |t2| + |t3|) + 1e-12.  Hessian: rtol 2^-23.
* NDCG / MAP / AUC-mu: 1e-9 * max(1, |ref|) (tests/test_ops.py's metric tolerance: only the
  summation order differs).
"""
import functools
import itertools

import numpy as np

from helpers import rank_refs

# triangular numbers: a monotone custom gain for the labels 0..30
CUSTOM_GAIN = [float(i * (i + 1) // 2) for i in range(31)]
EVAL_AT = [1, 3, 5, 10, 5000]  # (5000: beyond every query)

LAMBDARANK_COMBOS = list(itertools.product([False, True], [1, 3, 20], [1.0, 2.5], [True, False], [False, True]))
LAMBDARANK_IDS = ["%s-trunc%d-sig%g-%s-%s" % ("gain" if g else "defgain", t, s, "norm" if nm else "nonorm",
                                               "w" if w else "unw") for g, t, s, nm, w in LAMBDARANK_COMBOS]
# the 2048 / 2049 document queries: the defaults, and every option away from its default
LAMBDARANK_BIG_COMBOS = [(False, 20, 1.0, True, False), (True, 3, 2.5, False, True)]
LAMBDARANK_BIG_IDS = ["defaults", "gain-trunc3-sig2.5-nonorm-w"]
XENDCG_COMBOS = list(itertools.product([False, True], [0, 7]))
XENDCG_IDS = ["%s-seed%d" % ("w" if w else "unw", s) for w, s in XENDCG_COMBOS]

STRIDE_LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 300]  # wave (64) and workgroup (128) strides


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def lambdarank_data(big=False):
    """(score, label, group, weight, X): many short queries and the named edge queries; big: a
    query of exactly 2048 documents (the largest LDS staging), one of 2049 (the global-scratch
    kernel) and a short one."""
    rng = np.random.RandomState(21 if big else 20)
    scores, labels, names = [], [], []

    def add(name, s, l):
        scores.append(np.asarray(s, dtype=np.float64))
        labels.append(np.asarray(l, dtype=np.float32))
        names.append(name)

    def rand(n, top=5):
        return 2.0 * rng.randn(n), rng.randint(0, top, n)

    if big:
        for n in (2048, 37, 2049):
            s, l = rand(n)
            s[::7] = np.round(s[::7])  # (some ties)
            add("len%d" % n, s, l)
    else:
        for n in STRIDE_LENGTHS:
            add("len%d" % n, *rand(n))
        for n in rng.randint(4, 40, size=25):
            add("short", *rand(n))
        add("labels_equal", rand(10)[0], np.full(10, 2))
        add("labels_zero", rand(12)[0], np.zeros(12))
        add("scores_tied", np.full(17, 0.75), rand(17)[1])
        for n in (40, 130):
            s, l = rand(n)
            add("heavy_ties", np.round(s * 2) / 2, l)
        s, l = rand(20)
        s[7] = -np.inf
        add("one_min_score", s, l)
        s, l = rand(25)
        s[[3, 24]] = -np.inf
        add("two_min_scores", s, l)
        add("all_min_scores", np.full(6, -np.inf), rand(6)[1])
        add("pair_with_min_score", [0.3, -np.inf], [0, 3])
        # every other score tied: best == worst only if the worst skips the -inf document
        s = np.full(15, -1.25)
        s[4] = -np.inf
        add("tied_but_one_min_score", s, rand(15)[1])
        add("labels_to_30", rand(40)[0], np.concatenate([np.arange(31), rng.randint(0, 31, 9)]))
    group = np.array([len(s) for s in scores], dtype=np.int32)
    score, label = np.concatenate(scores), np.concatenate(labels)
    weight = (rng.rand(len(score)) + 0.5).astype(np.float32)  # per document
    X = rng.randn(len(score), 4).astype(np.float32)
    return _frozen(score, label, group, weight, X) + (tuple(names),)


def lambdarank_params(gain, trunc, sigmoid, norm):
    p = {"objective": "lambdarank", "lambdarank_truncation_level": trunc, "sigmoid": sigmoid,
         "lambdarank_norm": norm, "verbose": -1}
    if gain:
        p["label_gain"] = CUSTOM_GAIN
    return p


@functools.lru_cache(maxsize=None)
def lambdarank_reference(big, gain, trunc, sigmoid, norm, weighted):
    score, label, group, weight, _, _ = lambdarank_data(big)
    ref = rank_refs.lambdarank_ref(score, label, group, weight if weighted else None, sigmoid=sigmoid, norm=norm,
                                   truncation_level=trunc, label_gain=CUSTOM_GAIN if gain else None)
    _frozen(*ref.values())
    return ref


def check_lambdarank(grad, hess, ref, names=None, group=None, what=""):
    """grad / hess (float32) against lambdarank_ref's output at the module's bound."""
    u = 2.0 ** -24
    for got, key, skey in ((grad, "grad", "s_grad"), (hess, "hess", "s_hess")):
        got = np.asarray(got, dtype=np.float64)
        assert np.all(np.isfinite(got)), (what, key)
        err = np.abs(got - ref[key])
        tol = 2.0 * (ref["m"] + 3) * u * ref[skey] + 1e-12
        bad = np.nonzero(err > tol)[0]
        zero = np.nonzero((ref[key] == 0.0) & (got != 0.0))[0]
        print("%s %s: max err / bound %.3g, documents with pairs %d" %
              (what, key, float(np.max(err / tol)), int((ref["m"] > 0).sum())))
        assert len(bad) == 0, (what, key, _where(bad, group, names), got[bad[:5]], ref[key][bad[:5]], tol[bad[:5]])
        assert len(zero) == 0, (what, key, "not exactly 0", _where(zero, group, names), got[zero[:5]])


def _where(rows, group, names):
    if group is None or len(rows) == 0:
        return list(rows[:5])
    b = np.concatenate([[0], np.cumsum(group)])
    out = []
    for r in rows[:5]:
        q = int(np.searchsorted(b, r, side="right") - 1)
        out.append((names[q] if names else q, int(r - b[q])))
    return out


@functools.lru_cache(maxsize=None)
def xendcg_data(big=False):
    """(score of call 1, score of call 2, label, group, weight, X)"""
    rng = np.random.RandomState(31 if big else 30)
    group = np.array([2048, 5, 2049] if big else STRIDE_LENGTHS, dtype=np.int32)
    n = int(group.sum())
    score1, score2 = 2.0 * rng.randn(n), 2.0 * rng.randn(n)
    label = rng.randint(0, 5, n).astype(np.float32)
    weight = (rng.rand(n) + 0.5).astype(np.float32)
    X = rng.randn(n, 4).astype(np.float32)
    return _frozen(score1, score2, label, group, weight, X)


@functools.lru_cache(maxsize=None)
def xendcg_reference(big, weighted, seed, call):
    """the reference of call 1 or 2 on xendcg_data's scores of that call"""
    score1, score2, label, group, weight, _ = xendcg_data(big)
    ref = rank_refs.xendcg_ref(score1 if call == 1 else score2, label, group, weight if weighted else None,
                               seed=seed, draws_done=call - 1)
    _frozen(*ref.values())
    return ref


def check_xendcg(grad, hess, ref, what=""):
    grad, hess = np.asarray(grad, dtype=np.float64), np.asarray(hess, dtype=np.float64)
    assert np.all(np.isfinite(grad)) and np.all(np.isfinite(hess)), what
    tol = 2.0 ** -21 * np.abs(ref["terms"]).sum(axis=0) + 1e-12
    err = np.abs(grad - ref["grad"])
    herr = np.abs(hess - ref["hess"])
    htol = 2.0 ** -23 * np.abs(ref["hess"])
    print("%s: grad max err / bound %.3g, hess max relative err %.3g (allowed %.3g)" %
          (what, float(np.max(err / tol)), float(np.max(herr / np.maximum(np.abs(ref["hess"]), 1e-300))), 2.0 ** -23))
    bad = np.nonzero(err > tol)[0]
    assert len(bad) == 0, (what, bad[:5], grad[bad[:5]], ref["grad"][bad[:5]], tol[bad[:5]])
    bad = np.nonzero(herr > htol)[0]
    assert len(bad) == 0, (what, "hess", bad[:5], hess[bad[:5]], ref["hess"][bad[:5]])


@functools.lru_cache(maxsize=None)
def metric_data():
    """(score, label, group, query_weight, X): the LambdaRank queries with every score rounded to
    0.5 (ties), a query of 2048 and one of 2049 documents.  `labels_zero` has no relevant
    document, in `labels_equal` every document is relevant.  The query weights are powers of two:
    their float32 mean over a query's rows is exact."""
    _, label, group, _, _, names = lambdarank_data(False)
    rng = np.random.RandomState(40)
    extra = [2048, 2049]
    label = np.concatenate([label, rng.randint(0, 5, sum(extra)).astype(np.float32)])
    group = np.concatenate([group, np.array(extra, dtype=np.int32)])
    score = np.round(4.0 * rng.randn(len(label))) / 2
    qw = rng.choice([0.5, 1.0, 2.0, 4.0], size=len(group)).astype(np.float32)
    X = rng.randn(len(label), 4).astype(np.float32)
    assert "labels_zero" in names and "labels_equal" in names
    return _frozen(score, label, group, qw, X)


def metric_tolerance(ref):
    return 1e-9 * np.maximum(1.0, np.abs(np.asarray(ref, dtype=np.float64)))


AUCMU_CASES = [(K, n, cost) for K in (2, 3, 4) for n in (1000, 257) for cost in (False, True)]
AUCMU_IDS = ["K%d-n%d-%s" % (K, n, "cost" if c else "default") for K, n, c in AUCMU_CASES] + ["single_row_class"]
AUCMU_CASES = AUCMU_CASES + [(3, 257, "single")]


def aucmu_cost(K):
    """an integer cost matrix with a zero diagonal (not symmetric)"""
    return np.array([[0 if i == j else 1 + abs(i - j) + (i > j) for j in range(K)] for i in range(K)], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def aucmu_data(K, n, cost):
    """(score [K, n], label, W or None, X): scores are multiples of 1/8, so with integer weights
    the keys t1 * (v . s) are exact in float64 and tie in the same runs however they are summed"""
    rng = np.random.RandomState(50 + K)
    score = np.round(8.0 * rng.randn(K, n)) / 8
    if cost == "single":
        label = rng.randint(0, K - 1, n)
        label[n // 2] = K - 1  # the last class has a single row
        W = None
    else:
        label = rng.randint(0, K, n)
        W = aucmu_cost(K) if cost else None
    X = rng.randn(n, 4).astype(np.float32)
    label = label.astype(np.float32)
    arrays = _frozen(score, label, X)
    return arrays[0], arrays[1], W, arrays[2]
