"""NumPy float64 references of the listwise objectives and the query / AUC-mu metrics, written
from the formulas of the reference project (src/objective/rank_objective.hpp,
src/metric/dcg_calculator.cpp, rank_metric.hpp, map_metric.hpp, multiclass_metric.hpp) and
importing nothing of this project: the host objectives and metrics (tests/test_rank_refs_host.py)
and the device kernels (tests/test_rank_ops.py) are both compared with them.

Conventions: ``group`` holds the query sizes; documents of a query are consecutive rows; the
descending order of a query's scores is stable (ties keep the row order); a score of -inf
(kMinScore) takes a document out of LambdaRank's pairs."""
import numpy as np

SIGMOID_BINS = 1 << 20
MAX_LABEL = 31


def default_label_gain():
    """2^i - 1 for the labels 0..30."""
    return np.array([0.0] + [float((1 << i) - 1) for i in range(1, MAX_LABEL)])


def _bounds(group):
    b = np.zeros(len(group) + 1, dtype=np.int64)
    np.cumsum(np.asarray(group, dtype=np.int64), out=b[1:])
    return b


def _discount(n):
    return 1.0 / np.log2(2.0 + np.arange(n, dtype=np.float64))


def _max_dcg_at(k, labels, gain):
    """DCG of the best order of the first k positions: documents by label, highest first."""
    k = min(int(k), len(labels))
    top = np.sort(labels)[::-1][:k]
    return float(np.sum(_discount(k) * gain[top]))


def _stable_desc(s):
    return np.argsort(-s, kind="stable")


def sigmoid_table_lookup(ds, sigmoid):
    """1 / (1 + exp(x * sigmoid)) read from the objective's table of 2^20 entries over
    [-25 / sigmoid, 25 / sigmoid]: entry floor((ds - min) * factor), the ends clamped."""
    lo = -25.0 / sigmoid
    hi = -lo
    factor = SIGMOID_BINS / (50.0 / sigmoid)
    idx = np.floor((np.clip(ds, lo, hi) - lo) * factor)
    idx = np.where(ds <= lo, 0.0, np.where(ds >= hi, SIGMOID_BINS - 1.0, idx))
    return 1.0 / (1.0 + np.exp((idx / factor + lo) * sigmoid))


def lambdarank_ref(score, label, group, weight=None, sigmoid=1.0, norm=True, truncation_level=20, label_gain=None):
    """LambdaRank-NDCG gradients.  Returns a dict of float64 arrays over the documents: ``grad``,
    ``hess``; ``m``, the number of pair terms added into the document's sums; ``s_grad`` and
    ``s_hess``, the sums of those terms' absolute values after normalisation and weight."""
    score = np.asarray(score, dtype=np.float64)
    lab = np.asarray(label).astype(np.int64)
    gain_tab = default_label_gain() if label_gain is None else np.asarray(label_gain, dtype=np.float64)
    n = len(score)
    out = {k: np.zeros(n) for k in ("grad", "hess", "s_grad", "s_hess")}
    out["m"] = np.zeros(n, dtype=np.int64)
    b = _bounds(group)
    for q in range(len(group)):
        lo, hi = b[q], b[q + 1]
        cnt = hi - lo
        if cnt == 0:
            continue
        s, l = score[lo:hi], lab[lo:hi]
        max_dcg = _max_dcg_at(truncation_level, l, gain_tab)
        inv_max = 1.0 / max_dcg if max_dcg > 0.0 else max_dcg
        order = _stable_desc(s)
        pos = np.empty(cnt, dtype=np.int64)
        pos[order] = np.arange(cnt)
        best = s[order[0]]
        worst_i = cnt - 1
        if worst_i > 0 and s[order[worst_i]] == -np.inf:
            worst_i -= 1
        worst = s[order[worst_i]]
        live = s != -np.inf
        # pair (i, j): i the higher label, j the lower
        valid = (l[:, None] > l[None, :]) & live[:, None] & live[None, :]
        sf = np.where(live, s, 0.0)
        ds = sf[:, None] - sf[None, :]
        gain = gain_tab[l]
        disc = _discount(cnt)[pos]
        dn = (gain[:, None] - gain[None, :]) * np.abs(disc[:, None] - disc[None, :]) * inv_max
        if norm and best != worst:
            dn = dn / (np.float64(np.float32(0.01)) + np.abs(ds))
        p = sigmoid_table_lookup(ds, sigmoid)
        pl = np.where(valid, p * (-sigmoid * dn), 0.0)
        ph = np.where(valid, p * (1.0 - p) * (sigmoid * sigmoid * dn), 0.0)
        g = pl.sum(axis=1) - pl.sum(axis=0)
        h = ph.sum(axis=1) + ph.sum(axis=0)
        sg = np.abs(pl).sum(axis=1) + np.abs(pl).sum(axis=0)
        sh = np.abs(ph).sum(axis=1) + np.abs(ph).sum(axis=0)
        sum_lambdas = -2.0 * pl.sum()
        if norm and sum_lambdas > 0:
            nf = np.log2(1.0 + sum_lambdas) / sum_lambdas
            g, h, sg, sh = g * nf, h * nf, sg * nf, sh * nf
        if weight is not None:
            w = np.asarray(weight, dtype=np.float64)[lo:hi]
            g, h, sg, sh = g * w, h * w, sg * np.abs(w), sh * np.abs(w)
        out["grad"][lo:hi], out["hess"][lo:hi] = g, h
        out["s_grad"][lo:hi], out["s_hess"][lo:hi] = sg, sh
        out["m"][lo:hi] = valid.sum(axis=1) + valid.sum(axis=0)
    return out


def lcg_next(x):
    """One step of the reference's generator; returns (state, the float in [0, 1) it draws)."""
    x = (214013 * int(x) + 2531011) & 0xFFFFFFFF
    return x, ((x >> 16) & 0x7FFF) / 32768.0


def xendcg_states(group, seed, draws_done=0):
    """The per-query generator states Random(seed + q) after ``draws_done`` gradient calls (a call
    draws one number per document of every query of two or more documents)."""
    st = np.zeros(len(group), dtype=np.uint32)
    for q, cnt in enumerate(group):
        x = (int(seed) + q) & 0xFFFFFFFF
        if cnt > 1:
            for _ in range(int(draws_done) * int(cnt)):
                x, _u = lcg_next(x)
        st[q] = x
    return st


def xendcg_ref(score, label, group, weight=None, seed=0, draws_done=0):
    """XE-NDCG gradients of one call that follows ``draws_done`` earlier ones.  Returns a dict:
    ``grad``, ``hess``; ``terms`` ``[3, n]``, the first / second / third order parts of the
    gradient (after the weight); ``states``, the generators after the call (uint32)."""
    score = np.asarray(score, dtype=np.float64)
    lab = np.asarray(label).astype(np.int64)
    n = len(score)
    grad, hess, terms = np.zeros(n), np.zeros(n), np.zeros((3, n))
    states = xendcg_states(group, seed, draws_done)
    b = _bounds(group)
    for q in range(len(group)):
        lo, hi = b[q], b[q + 1]
        cnt = hi - lo
        if cnt <= 1:
            continue
        s = score[lo:hi]
        e = np.exp(s - s.max())
        rho = e / e.sum()
        x = int(states[q])
        u = np.empty(cnt)
        for i in range(cnt):
            x, u[i] = lcg_next(x)
        states[q] = x
        par = np.exp2(lab[lo:hi].astype(np.float64)) - u
        inv_den = 1.0 / max(1e-15, par.sum())
        t1 = -par * inv_den + rho
        par = t1 / (1.0 - rho)
        t2 = rho * (par.sum() - par)
        par = t2 / (1.0 - rho)
        t3 = rho * (par.sum() - par)
        w = 1.0 if weight is None else np.asarray(weight, dtype=np.float64)[lo:hi]
        terms[:, lo:hi] = np.stack([t1, t2, t3]) * w
        grad[lo:hi] = (t1 + t2 + t3) * w
        hess[lo:hi] = rho * (1.0 - rho) * w
    return {"grad": grad, "hess": hess, "terms": terms, "states": states}


def _query_weights(group, query_weight):
    nq = len(group)
    if query_weight is None:
        return None, float(nq)
    qw = np.asarray(query_weight, dtype=np.float64)
    return qw, float(qw.sum())


def ndcg_ref(score, label, group, eval_at, query_weight=None, label_gain=None):
    """NDCG@k for every k of ``eval_at``, averaged over the queries with their weights.  A query
    with no relevant document (max DCG 0) scores 1; with query weights the reference adds that 1
    as it is, not times the query's weight (rank_metric.hpp, the weighted branch of Eval)."""
    score = np.asarray(score, dtype=np.float64)
    lab = np.asarray(label).astype(np.int64)
    gain_tab = default_label_gain() if label_gain is None else np.asarray(label_gain, dtype=np.float64)
    qw, sum_w = _query_weights(group, query_weight)
    total = np.zeros(len(eval_at))
    b = _bounds(group)
    for q in range(len(group)):
        lo, hi = b[q], b[q + 1]
        cnt = hi - lo
        s, l = score[lo:hi], lab[lo:hi]
        max_dcg = [_max_dcg_at(k, l, gain_tab) for k in eval_at]
        if not max_dcg[0] > 0.0:
            total += 1.0
            continue
        g = gain_tab[l[_stable_desc(s)]] * _discount(cnt)
        for j, k in enumerate(eval_at):
            v = float(np.sum(g[:min(int(k), cnt)])) / max_dcg[j]
            total[j] += v * (1.0 if qw is None else qw[q])
    return total / sum_w


def map_ref(score, label, group, eval_at, query_weight=None):
    """MAP@k for every k of ``eval_at`` (ascending): the precisions at the relevant documents
    (label > 0.5) ranked within k, over min(relevant documents, k); a query with no relevant
    document scores 1."""
    score = np.asarray(score, dtype=np.float64)
    label = np.asarray(label, dtype=np.float64)
    qw, sum_w = _query_weights(group, query_weight)
    total = np.zeros(len(eval_at))
    b = _bounds(group)
    for q in range(len(group)):
        lo, hi = b[q], b[q + 1]
        cnt = hi - lo
        rel = label[lo:hi][_stable_desc(score[lo:hi])] > 0.5
        npos = int(rel.sum())
        prec = np.where(rel, np.cumsum(rel) / (np.arange(cnt) + 1.0), 0.0)
        w = 1.0 if qw is None else qw[q]
        for j, k in enumerate(eval_at):
            k = min(int(k), cnt)
            total[j] += (float(prec[:k].sum()) / min(npos, k) if npos > 0 else 1.0) * w
    return total / sum_w


def auc_mu_ref(score, label, W=None):
    """AUC-mu of class-major scores ``[K, n]``: for every class pair i < j the Mann-Whitney
    statistic (ties count one half) of the keys t1 * (v . s), v = W[i] - W[j], t1 = v[i] - v[j],
    class i above class j; averaged over the K (K - 1) / 2 pairs.  W defaults to ones off the
    diagonal."""
    score = np.asarray(score, dtype=np.float64)
    lab = np.asarray(label).astype(np.int64)
    K = score.shape[0]
    W = (1.0 - np.eye(K)) if W is None else np.asarray(W, dtype=np.float64)
    ans = 0.0
    for i in range(K):
        for j in range(i + 1, K):
            v = W[i] - W[j]
            t1 = v[i] - v[j]
            key = t1 * (v @ score)
            ki, kj = key[lab == i], np.sort(key[lab == j])
            below = np.searchsorted(kj, ki, side="left")
            upto = np.searchsorted(kj, ki, side="right")
            s_ij = float(np.sum(below + 0.5 * (upto - below)))
            ans += s_ij / len(ki) / len(kj)
    return 2.0 * ans / K / (K - 1)
