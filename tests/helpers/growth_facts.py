"""Facts for LGBM_AMD_GrowthPlan (src/treelearner/growth_plan.h) as a device learner has them."""
from lightgbmv1_amd import _native as nat

# one process, 8 numerical features
SERIAL = {"kind": "serial", "world": 1, "num_features": 8, "num_categorical": 0, "max_cat_bins": 0, "total_bins": 120}


def learner_plan(params, **facts):
    """The plan a learner comes to, in its three steps: the round width when the data is uploaded,
    the round flags when the round buffers are allocated (six node rows per leaf; none at width
    1), and the tree's plan with that width and those flags as facts."""
    f = dict(SERIAL, **facts)
    width = nat.growth_plan(params, f)["round_width"]
    f.update(round_k=width, split_rows=(6 if width > 1 else 1) * params.get("num_leaves", 31))
    alloc = nat.growth_plan(params, f)
    f.update(round_allocated=width > 1, alloc_bynode=alloc["round_bynode"], alloc_xt=alloc["round_xt"],
             alloc_cegb=alloc["round_cegb"])
    return nat.growth_plan(params, f)
