"""The listwise gradient kernels (src/device/rank_kernels.hip: k_lambdarank, k_lambdarank_big,
k_xendcg, k_xendcg_big), the query metrics (QueryMetricBody of src/device/metric_kernels.hip:
NDCG@k / MAP@k, LDS and global-scratch variants) and AUC-mu, reached through lightgbmv1_amd.ops,
against the independent float64 references of tests/helpers/rank_refs.py -- the references the
host objectives and metrics are held to without a GPU (tests/test_rank_refs_host.py), at the same
cases and bounds (tests/helpers/rank_cases.py)."""
import numpy as np
import pytest

from helpers import rank_cases as rc
from helpers import rank_refs

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda")


def _lambdarank(big, gain, trunc, sigmoid, norm, weighted, monkeypatch):
    from lightgbmv1_amd import ops
    score, label, group, weight, _, names = rc.lambdarank_data(big)
    ref = rc.lambdarank_reference(big, gain, trunc, sigmoid, norm, weighted)
    assert np.abs(ref["grad"]).sum() > 0
    params = rc.lambdarank_params(gain, trunc, sigmoid, norm)
    ds = _dev(score)
    # the pair scratch (each pair evaluated once) and, with a budget of 0, without it (twice)
    for pair_mb in (None, "0"):
        if pair_mb is None:
            monkeypatch.delenv("LGBM_AMD_RANK_PAIR_MB", raising=False)
        else:
            monkeypatch.setenv("LGBM_AMD_RANK_PAIR_MB", pair_mb)
        g, h = ops.gradients(params, ds, label, weight if weighted else None, group=group)
        rc.check_lambdarank(g.cpu().numpy(), h.cpu().numpy(), ref, names, group,
                            "device pair_mb=%s" % (pair_mb or "default"))


@pytest.mark.parametrize("gain,trunc,sigmoid,norm,weighted", rc.LAMBDARANK_COMBOS, ids=rc.LAMBDARANK_IDS)
def test_lambdarank_kernel_matches_reference(gain, trunc, sigmoid, norm, weighted, gpu_available, monkeypatch):
    """Short queries at the wave / workgroup strides and the edge queries (no pairs, max DCG 0,
    tied scores, -inf documents, labels to 30), every option combination, with and without the
    pair scratch."""
    _lambdarank(False, gain, trunc, sigmoid, norm, weighted, monkeypatch)


@pytest.mark.parametrize("gain,trunc,sigmoid,norm,weighted", rc.LAMBDARANK_BIG_COMBOS, ids=rc.LAMBDARANK_BIG_IDS)
def test_lambdarank_kernel_at_the_lds_limit(gain, trunc, sigmoid, norm, weighted, gpu_available, monkeypatch):
    """A query of exactly 2048 documents (the 88 KiB LDS staging) and one of 2049
    (k_lambdarank_big over the global scratch)."""
    _lambdarank(True, gain, trunc, sigmoid, norm, weighted, monkeypatch)


def test_lambdarank_with_poisoned_args(gpu_available, monkeypatch):
    """LGBM_AMD_POISON_ARGS=1: a RankArgs field the op forgets to set reads 0xA5 garbage."""
    monkeypatch.setenv("LGBM_AMD_POISON_ARGS", "1")
    _lambdarank(True, False, 20, 1.0, True, True, monkeypatch)


@pytest.mark.parametrize("big", [False, True], ids=["strides", "2048_2049"])
@pytest.mark.parametrize("weighted,seed", rc.XENDCG_COMBOS, ids=rc.XENDCG_IDS)
def test_xendcg_kernel_matches_reference_over_two_calls(weighted, seed, big, gpu_available):
    """Two consecutive calls on one rng_state: gradients, hessians and the generator states
    after each call (a query of one document leaves its state untouched and gets zeros)."""
    from lightgbmv1_amd import ops
    score1, score2, label, group, weight, _ = rc.xendcg_data(big)
    params = {"objective": "rank_xendcg", "objective_seed": seed, "verbose": -1}
    fresh = rank_refs.xendcg_states(group, seed)
    np.testing.assert_array_equal(fresh, (seed + np.arange(len(group))) & 0xFFFFFFFF)
    state = torch.tensor(fresh.view(np.int32), device="cuda")
    w = weight if weighted else None
    for call, score in ((1, score1), (2, score2)):
        ref = rc.xendcg_reference(big, weighted, seed, call)
        g, h = ops.gradients(params, _dev(score), label, w, group=group, rng_state=state)
        got = state.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, ref["states"], err_msg="generator states after call %d" % call)
        g, h = g.cpu().numpy(), h.cpu().numpy()
        rc.check_xendcg(g, h, ref, "device call %d" % call)
        for q in np.nonzero(group <= 1)[0]:
            b = int(group[:q].sum())
            assert g[b] == 0.0 and h[b] == 0.0 and got[q] == fresh[q]
    # without rng_state every call starts from the objective's fresh generators
    g, h = ops.gradients(params, _dev(score1), label, w, group=group)
    rc.check_xendcg(g.cpu().numpy(), h.cpu().numpy(), rc.xendcg_reference(big, weighted, seed, 1), "device fresh")


@pytest.mark.parametrize("gain", [False, True], ids=["defgain", "gain"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unw", "qw"])
def test_ndcg_and_map_kernels_match_reference(weighted, gain, gpu_available):
    """NDCG@k and MAP@k over tied scores, k beyond the query length, queries of 2048 (LDS) and
    2049 (global scratch) documents, a query without and one with only relevant documents."""
    from lightgbmv1_amd import ops
    score, label, group, qw, _ = rc.metric_data()
    q = qw if weighted else None
    params = {"objective": "lambdarank", "eval_at": rc.EVAL_AT, "verbose": -1}
    if gain:
        params["label_gain"] = rc.CUSTOM_GAIN
    ds = _dev(score)
    refs = {"ndcg": rank_refs.ndcg_ref(score, label, group, rc.EVAL_AT, q, rc.CUSTOM_GAIN if gain else None),
            "map": rank_refs.map_ref(score, label, group, rc.EVAL_AT, q)}
    for name, ref in refs.items():
        got = ops.metric(dict(params, metric=name), ds, label, group=group, query_weight=q)
        assert len(got) == len(rc.EVAL_AT)
        for k, v, r in zip(rc.EVAL_AT, got, ref):
            print("%s@%d" % (name, k), v, r)
            assert abs(v - r) <= rc.metric_tolerance(r), (name, k, v, r)


@pytest.mark.parametrize("K,n,cost", rc.AUCMU_CASES, ids=rc.AUCMU_IDS)
def test_auc_mu_kernels_match_reference(K, n, cost, gpu_available):
    from lightgbmv1_amd import ops
    score, label, W, _ = rc.aucmu_data(K, n, cost)
    params = {"objective": "multiclass", "num_class": K, "metric": "auc_mu", "verbose": -1}
    if W is not None:
        params["auc_mu_weights"] = list(W.ravel())
    got = ops.metric(params, _dev(score).contiguous(), label)
    ref = rank_refs.auc_mu_ref(score, label, W)
    print("auc_mu", got, ref)
    assert abs(got - ref) <= rc.metric_tolerance(ref), (got, ref)
