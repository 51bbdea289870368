"""The best-split rule, once, in plain Python floats (IEEE double), one bin at a time.

Written from the formulas of the reference's feature_histogram.hpp (FindBestThresholdSequentially,
FindBestThresholdCategoricalInner, GetSplitGains, CalculateSplittedLeafOutput, GetLeafGain),
Dataset::FixHistogram and the basic monotone constraints of monotone_constraints.hpp.  Nothing here
is vectorised and nothing calls the library: tests/test_split_ref.py holds it to the reference's
own models, tests/test_split_ref_host.py holds the host finder to it and
tests/test_device_split_ref.py the HIP split scans.

A feature's meta is a dict: num_bin, missing_type (0 none, 1 zero, 2 NaN), default_bin,
most_freq_bin, offset (1 when the most frequent bin is 0: bin 0 is not stored), categorical,
monotone (-1, 0, 1), penalty (feature_contri), real (the real feature index).
A histogram is the stored one: num_bin - offset pairs [g, h]; the entry of a most frequent bin > 0
is rebuilt from the leaf's totals (fix_histogram) whatever it holds.
"""
import math

import numpy as np

K_EPS = float(np.float32(1e-15))  # kEpsilon as the code has it: a float constant
NONE, ZERO, NAN = 0, 1, 2

DEFAULTS = dict(lambda_l1=0.0, lambda_l2=0.0, max_delta_step=0.0, path_smooth=0.0, min_gain_to_split=0.0,
                min_sum_hessian_in_leaf=1e-3, min_data_in_leaf=20, cat_l2=10.0, cat_smooth=10.0,
                max_cat_threshold=32, min_data_per_group=100, max_cat_to_onehot=4, monotone_penalty=0.0,
                use_mc=False, max_depth=-1)


def params(**kw):
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def round_int(x):
    """Common::RoundInt: truncation of x + 0.5"""
    return int(x + 0.5)


def sign(x):
    return (x > 0) - (x < 0)


def threshold_l1(s, l1):
    return sign(s) * max(0.0, abs(s) - l1)


def leaf_output(sg, sh, p, n, parent, l2=None, l1=True, clip=True, smooth=True, cmin=-math.inf, cmax=math.inf):
    """CalculateSplittedLeafOutput: -ThresholdL1(sg) / (sh + l2), clipped to max_delta_step,
    smoothed towards the parent's output by n / path_smooth, clamped to the leaf's range"""
    l2 = p["lambda_l2"] if l2 is None else l2
    if l1 and p["lambda_l1"] > 0:
        r = -threshold_l1(sg, p["lambda_l1"]) / (sh + l2)
    else:
        r = -sg / (sh + l2)
    if clip and p["max_delta_step"] > 0 and abs(r) > p["max_delta_step"]:
        r = sign(r) * p["max_delta_step"]
    if smooth and p["path_smooth"] > K_EPS:
        w = n / p["path_smooth"]
        r = r * w / (w + 1) + parent / (w + 1)
    if p["use_mc"]:
        if r < cmin:
            r = cmin
        elif r > cmax:
            r = cmax
    return r


def gain_given_output(sg, sh, p, out, l2):
    g = threshold_l1(sg, p["lambda_l1"]) if p["lambda_l1"] > 0 else sg
    return -(2.0 * g * out + (sh + l2) * out * out)


def leaf_gain(sg, sh, p, n, parent, l2=None, smooth=True):
    """GetLeafGain (no constraint range: the parent's own gain, or a side without monotone constraints)"""
    l2 = p["lambda_l2"] if l2 is None else l2
    smooth = smooth and p["path_smooth"] > K_EPS
    if not p["max_delta_step"] > 0 and not smooth:
        g = threshold_l1(sg, p["lambda_l1"]) if p["lambda_l1"] > 0 else sg
        return (g * g) / (sh + l2)
    q = dict(p, use_mc=False)
    out = leaf_output(sg, sh, q, n, parent, l2=l2, smooth=smooth)
    return gain_given_output(sg, sh, p, out, l2)


def split_gains(lg, lh, rg, rh, p, l2, cmin, cmax, monotone, lc, rc, parent):
    """GetSplitGains -> (gain, |left gain| + |right gain|)"""
    if not p["use_mc"]:
        a = leaf_gain(lg, lh, p, lc, parent, l2=l2)
        b = leaf_gain(rg, rh, p, rc, parent, l2=l2)
        return a + b, abs(a) + abs(b)
    lo = leaf_output(lg, lh, p, lc, parent, l2=l2, cmin=cmin, cmax=cmax)
    ro = leaf_output(rg, rh, p, rc, parent, l2=l2, cmin=cmin, cmax=cmax)
    if (monotone > 0 and lo > ro) or (monotone < 0 and lo < ro):
        return 0.0, 0.0
    a = gain_given_output(lg, lh, p, lo, l2)
    b = gain_given_output(rg, rh, p, ro, l2)
    return a + b, abs(a) + abs(b)


def monotone_split_penalty(depth, penalization):
    if penalization >= depth + 1.0:
        return K_EPS
    if penalization <= 1.0:
        return 1.0 - penalization / 2.0 ** depth + K_EPS
    return 1.0 - 2.0 ** (penalization - 1.0 - depth) + K_EPS


def fix_histogram(hist, meta, sum_g, sum_h):
    """Dataset::FixHistogram: a most frequent bin > 0 is the leaf's total less every other bin"""
    mfb = meta["most_freq_bin"]
    if mfb <= 0:
        return
    k = mfb - meta["offset"]
    g, h = sum_g, sum_h
    for i in range(len(hist)):
        if i != k:
            g -= hist[i][0]
            h -= hist[i][1]
    hist[k] = [g, h]


def _scan(hist, meta, p, sum_g, sum_h, n, cmin, cmax, parent, min_gain_shift, reverse, skip_default, na, cands):
    """one direction of FindBestThresholdSequentially -> (best or None, any candidate passed)"""
    off, nb = meta["offset"], meta["num_bin"]
    cnt_factor = n / sum_h
    best, any_ok = None, False
    min_n, min_h = p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"]

    def consider(lg, lh, lc, thr):
        nonlocal best, any_ok
        rg, rh, rc = sum_g - lg, sum_h - lh, n - lc
        gain, mag = split_gains(lg, lh, rg, rh, p, p["lambda_l2"], cmin, cmax, meta["monotone"], lc, rc, parent)
        cands.append(dict(threshold=thr, reverse=reverse, gain=gain, mag=mag, passed=gain > min_gain_shift))
        if not gain > min_gain_shift:  # the rule is gain > shift
            return
        any_ok = True
        if best is None or gain > best["gain"]:  # the first met wins ties: reverse the highest, forward the lowest
            best = dict(gain=gain, mag=mag, threshold=thr, lg=lg, lh=lh, lc=lc)

    if reverse:
        rg, rh, rc = 0.0, K_EPS, 0
        t = nb - 1 - off - (1 if na else 0)
        while t >= 1 - off:
            if skip_default and t + off == meta["default_bin"]:
                t -= 1
                continue
            rg += hist[t][0]
            rh += hist[t][1]
            rc += round_int(hist[t][1] * cnt_factor)
            t -= 1
            if rc < min_n or rh < min_h:
                continue
            lc = n - rc
            if lc < min_n:
                break
            lh = sum_h - rh
            if lh < min_h:
                break
            consider(sum_g - rg, lh, lc, t + off)  # (t is already one lower: threshold t_old - 1 + offset)
    else:
        lg, lh, lc = 0.0, K_EPS, 0
        t = 0
        if na and off == 1:  # what is stored nowhere (bin 0) starts on the left
            lg, lh, lc = sum_g, sum_h - K_EPS, n
            for i in range(nb - off):
                lg -= hist[i][0]
                lh -= hist[i][1]
                lc -= round_int(hist[i][1] * cnt_factor)
            t = -1
        while t <= nb - 2 - off:
            if skip_default and t + off == meta["default_bin"]:
                t += 1
                continue
            if t >= 0:
                lg += hist[t][0]
                lh += hist[t][1]
                lc += round_int(hist[t][1] * cnt_factor)
            t += 1
            if lc < min_n or lh < min_h:
                continue
            rc = n - lc
            if rc < min_n:
                break
            if sum_h - lh < min_h:
                break
            consider(lg, lh, lc, t - 1 + off)
    return best, any_ok


def _finish(best, p, l2, sum_g, sum_h, n, cmin, cmax, parent, min_gain_shift, gain_shift):
    lg, lh, lc = best["lg"], best["lh"], best["lc"]
    return dict(gain=best["gain"] - min_gain_shift, mag=best["mag"] + abs(gain_shift),
                left_count=lc, right_count=n - lc,
                left_sum_gradient=lg, left_sum_hessian=lh - K_EPS,
                right_sum_gradient=sum_g - lg, right_sum_hessian=sum_h - lh - K_EPS,
                left_output=leaf_output(lg, lh, p, lc, parent, l2=l2, cmin=cmin, cmax=cmax),
                right_output=leaf_output(sum_g - lg, sum_h - lh, p, n - lc, parent, l2=l2, cmin=cmin, cmax=cmax))


def find_numerical(hist, meta, p, sum_g, sum_h, n, cmin, cmax, parent, cands):
    gain_shift = leaf_gain(sum_g, sum_h, p, n, parent)
    min_gain_shift = gain_shift + p["min_gain_to_split"]
    two = meta["num_bin"] > 2 and meta["missing_type"] != NONE
    if two:
        zero = meta["missing_type"] == ZERO
        plan = [(True, zero, not zero), (False, zero, not zero)]
    else:
        plan = [(True, False, False)]
    out, splittable = None, False
    for reverse, skip_default, na in plan:
        best, ok = _scan(hist, meta, p, sum_g, sum_h, n, cmin, cmax, parent, min_gain_shift, reverse, skip_default,
                         na, cands)
        splittable = splittable or ok
        # forward replaces reverse only when strictly better, against the stored gain with the shift
        # added back (the reference's own comparison, roundings included)
        if splittable and best is not None and (out is None or best["gain"] > out["gain"] + min_gain_shift):
            out = _finish(best, p, p["lambda_l2"], sum_g, sum_h, n, cmin, cmax, parent, min_gain_shift, gain_shift)
            out.update(threshold=best["threshold"], default_left=reverse, cat_bins=None)
    if out is not None and not two and meta["missing_type"] == NAN:
        out["default_left"] = False
    return out, splittable


def find_categorical(hist, meta, p, sum_g, sum_h, n, cmin, cmax, parent, cands):
    off, nb = meta["offset"], meta["num_bin"]
    if p["path_smooth"] > K_EPS:
        gain_shift = gain_given_output(sum_g, sum_h, p, parent, p["lambda_l2"])
    else:
        gain_shift = leaf_gain(sum_g, sum_h, p, n, 0.0, smooth=False)
    min_gain_shift = gain_shift + p["min_gain_to_split"]
    cnt_factor = n / sum_h
    min_n, min_h = p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"]
    l2 = p["lambda_l2"]
    best = None
    if nb <= p["max_cat_to_onehot"]:
        for t in range(1 - off, nb - off):
            g, h = hist[t]
            cnt = round_int(h * cnt_factor)
            if cnt < min_n or h < min_h:
                continue
            other = n - cnt
            if other < min_n:
                continue
            oh = sum_h - h - K_EPS
            if oh < min_h:
                continue
            og = sum_g - g
            gain, mag = split_gains(og, oh, g, h + K_EPS, p, l2, cmin, cmax, 0, other, cnt, parent)
            cands.append(dict(threshold=t + off, reverse=False, gain=gain, mag=mag, passed=gain > min_gain_shift))
            if not gain > min_gain_shift:
                continue
            if best is None or gain > best["gain"]:
                best = dict(gain=gain, mag=mag, lg=g, lh=h + K_EPS, lc=cnt, bins=[t + off])
    else:
        order = [i for i in range(1 - off, nb - off) if round_int(hist[i][1] * cnt_factor) >= p["cat_smooth"]]
        order.sort(key=lambda i: hist[i][0] / (hist[i][1] + p["cat_smooth"]))  # (list.sort is stable)
        used = len(order)
        l2 += p["cat_l2"]
        max_num_cat = min(p["max_cat_threshold"], (used + 1) // 2)
        for direction, start in ((1, 0), (-1, used - 1)):
            pos, group = start, 0
            lg, lh, lc = 0.0, K_EPS, 0
            for i in range(min(used, max_num_cat)):
                t = order[pos]
                pos += direction
                cnt = round_int(hist[t][1] * cnt_factor)
                lg += hist[t][0]
                lh += hist[t][1]
                lc += cnt
                group += cnt
                if lc < min_n or lh < min_h:
                    continue
                rc = n - lc
                if rc < min_n or rc < p["min_data_per_group"]:
                    break
                rh = sum_h - lh
                if rh < min_h:
                    break
                if group < p["min_data_per_group"]:
                    continue
                group = 0
                gain, mag = split_gains(lg, lh, sum_g - lg, rh, p, l2, cmin, cmax, 0, lc, rc, parent)
                cands.append(dict(threshold=i, reverse=direction < 0, gain=gain, mag=mag,
                                  passed=gain > min_gain_shift))
                if not gain > min_gain_shift:
                    continue
                if best is None or gain > best["gain"]:
                    bins = order[:i + 1] if direction > 0 else order[used - 1 - i:][::-1]
                    best = dict(gain=gain, mag=mag, lg=lg, lh=lh, lc=lc, bins=[b + off for b in bins])
    if best is None:
        return None, False
    out = _finish(best, p, l2, sum_g, sum_h, n, cmin, cmax, parent, min_gain_shift, gain_shift)
    out.update(threshold=None, default_left=False, cat_bins=sorted(best["bins"]))
    return out, True


def find_feature(stored_hist, meta, p, sum_g, sum_h, n, cmin=-math.inf, cmax=math.inf, parent=0.0, depth=0):
    """the feature's best split of a leaf -> (split dict or None, splittable, candidates).
    The split's gain carries the feature penalty and, on a monotone feature, the depth penalty;
    mag = |left gain| + |right gain| + |gain shift| of the winner, the scale of the gain's error."""
    hist = [[float(g), float(h)] for g, h in stored_hist]
    assert len(hist) == meta["num_bin"] - meta["offset"]
    fix_histogram(hist, meta, sum_g, sum_h)
    cands = []
    find = find_categorical if meta["categorical"] else find_numerical
    out, splittable = find(hist, meta, p, sum_g, sum_h + 2 * K_EPS, n, cmin, cmax, parent, cands)
    if out is not None:
        out["monotone"] = 0 if meta["categorical"] else meta["monotone"]
        out["gain"] *= meta["penalty"]
        out["mag"] *= abs(meta["penalty"])
        if out["monotone"] != 0:
            out["gain"] *= monotone_split_penalty(depth, p["monotone_penalty"])
            out["mag"] *= monotone_split_penalty(depth, p["monotone_penalty"])
    return out, splittable, cands


def leaf0_parent_output(sum_g, sum_h, n, p, cmin=-math.inf, cmax=math.inf):
    """the "parent output" of a scan of leaf 0 -- the root, and whichever leaf keeps its id: the leaf's
    own output with L1 and max_delta_step, clamped to its range, without smoothing (the reference
    decides by the leaf's index, serial_tree_learner.cpp ComputeBestSplitForFeature).  Every other
    leaf is smoothed towards the output its parent's split gave it"""
    return leaf_output(sum_g, sum_h, dict(p, use_mc=True), n, 0.0, smooth=False, cmin=cmin, cmax=cmax)


def better(a, b):
    """SplitInfo's order: gain, then the lower real feature"""
    if b is None:
        return a is not None
    if a is None:
        return False
    if a["gain"] != b["gain"]:
        return a["gain"] > b["gain"]
    return a["real"] < b["real"]


def leaf_best(hists, metas, p, leaf, allowed=None):
    """best split of a leaf over the features -> (split or None, [splittable per feature])"""
    best, flags = None, []
    for f, meta in enumerate(metas):
        if allowed is not None and not allowed[f]:
            flags.append(False)
            continue
        s, ok, _ = find_feature(hists[f], meta, p, leaf["sum_g"], leaf["sum_h"], leaf["n"], leaf["cmin"],
                                leaf["cmax"], leaf["output"], leaf["depth"])
        flags.append(ok)
        if s is not None:
            s["inner"], s["real"] = f, meta["real"]
            if better(s, best):
                best = s
    return best, flags


def stored_histogram(bins, f, g, h, rows, meta):
    """a leaf's stored histogram of feature f by summation; the most frequent bin is not accumulated"""
    off, mfb = meta["offset"], meta["most_freq_bin"]
    hist = [[0.0, 0.0] for _ in range(meta["num_bin"] - off)]
    for r in rows:
        b = int(bins[r][f])
        if b == mfb:
            continue
        hist[b - off][0] += float(g[r])
        hist[b - off][1] += float(h[r])
    return hist


def goes_left(b, split, meta):
    if split["cat_bins"] is not None:
        return b in split["cat_set"]
    if meta["missing_type"] == ZERO and b == meta["default_bin"]:
        return split["default_left"]
    if meta["missing_type"] == NAN and b == meta["num_bin"] - 1:
        return split["default_left"]
    return b <= split["threshold"]


def grow(bins, g, h, metas, p, num_leaves=4):
    """Best-first growth of up to num_leaves leaves.  bins: [rows][features] feature bins; g, h per
    row.  Each step applies the argmax over the leaves' best splits: gain, then real feature, then
    leaf id.  -> dict(nodes=[applied split + leaf, left, right ids], leaves=[leaf state], scanned=
    [(leaf state, best split, hists) in scan order])"""
    n = len(g)
    rows = list(range(n))
    sg = math.fsum(float(x) for x in g)
    sh = math.fsum(float(x) for x in h)
    root = dict(rows=rows, sum_g=sg, sum_h=sh, n=n, depth=0, cmin=-math.inf, cmax=math.inf, value=0.0,
                output=0.0)
    leaves, best, flags, nodes, scanned = [root], [None], [None], [], []

    def scan(i, allowed):
        lf = leaves[i]
        if i == 0:
            lf["output"] = leaf0_parent_output(lf["sum_g"], lf["sum_h"], lf["n"], p, lf["cmin"], lf["cmax"])
        hists = [stored_histogram(bins, f, g, h, lf["rows"], m) for f, m in enumerate(metas)]
        best[i], flags[i] = leaf_best(hists, metas, p, lf, allowed)
        scanned.append(dict(leaf=i, state=lf, split=best[i], hists=hists))

    scan(0, None)
    while len(leaves) < num_leaves:
        pick = None
        for i, s in enumerate(best):
            if s is not None and (pick is None or better(s, best[pick])):  # the lower leaf id wins ties
                pick = i
        if pick is None or not best[pick]["gain"] > 0.0:
            break
        s, lf = best[pick], leaves[pick]
        meta = metas[s["inner"]]
        s["cat_set"] = set(s["cat_bins"] or ())
        left_rows = [r for r in lf["rows"] if goes_left(int(bins[r][s["inner"]]), s, meta)]
        lset = set(left_rows)
        right_rows = [r for r in lf["rows"] if r not in lset]
        new = len(leaves)
        nodes.append(dict(split=s, leaf=pick, state=lf, left=pick, right=new, internal_value=lf["value"],
                          internal_count=lf["n"], left_actual=len(left_rows), right_actual=len(right_rows)))
        lo, ro = s["left_output"], s["right_output"]
        kids = []
        for side, rws, out in (("left", left_rows, lo), ("right", right_rows, ro)):
            kids.append(dict(rows=rws, sum_g=s[side + "_sum_gradient"], sum_h=s[side + "_sum_hessian"], n=len(rws),
                             depth=lf["depth"] + 1, cmin=lf["cmin"], cmax=lf["cmax"], value=out, output=out))
        if s["cat_bins"] is None and s["monotone"] != 0:  # basic constraints: the children meet at the middle
            mid = (lo + ro) / 2.0
            if s["monotone"] < 0:
                kids[0]["cmin"] = max(kids[0]["cmin"], mid)
                kids[1]["cmax"] = min(kids[1]["cmax"], mid)
            else:
                kids[0]["cmax"] = min(kids[0]["cmax"], mid)
                kids[1]["cmin"] = max(kids[1]["cmin"], mid)
        parent_flags = flags[pick]
        leaves[pick] = kids[0]
        leaves.append(kids[1])
        best.append(None)
        flags.append(None)
        best[pick] = None
        if len(leaves) >= num_leaves:
            break
        md = p["min_data_in_leaf"]
        too_small = kids[0]["n"] < 2 * md and kids[1]["n"] < 2 * md
        too_deep = p["max_depth"] > 0 and kids[0]["depth"] >= p["max_depth"]
        if not too_small and not too_deep:
            scan(pick, parent_flags)   # features the parent could not split on are not scanned again
            scan(new, parent_flags)
    return dict(nodes=nodes, leaves=leaves, scanned=scanned)
