// extra_trees on round growth: the replay's evaluation of a drawn threshold (round_plan.h)
#pragma once

#include "find_stage.h"
#include "round_common.h"

namespace lgbm_amd {
namespace dev {

// extra_trees on round growth (KArgs::round_xt), one lane: feature f's split of node `node` at
// the drawn threshold rthr, from the node's prefix table -- FindNumericalBlock's candidates at
// that threshold (the reverse one at bin rthr + 1 - offset, the forward one at rthr - offset,
// the forward start for a NaN bin without bin 0), the same sums (exact) and selection, then the
// scan's feature and depth penalties.  Returns the splittable flag.
__device__ bool XtEvalNum(const KArgs& a, const Feature& F, int f, int node, const ChildStats& cs, int n, int rthr,
                          FeatureBest* out) {
  const SplitParams& p = a.p.sp;
  const bool simple = SimpleGains(p);
  const XtPre* pre = a.node_pre + static_cast<size_t>(node) * a.p.total_bins + F.hist_offset;
  const int nb = F.num_bin - F.offset, offset = F.offset;
  const bool two = F.num_bin > 2 && F.missing_type != 0;
  const bool skip_def = two && F.missing_type == 1;
  const bool na = two && F.missing_type == 2;
  const int def_t = skip_def ? F.default_bin - offset : -1;
  LeafCtx L;
  L.sg = cs.sum_g;
  L.sh = cs.sum_h + 2 * kEpsilon;
  L.n = n;
  L.c.min = cs.cmin;
  L.c.max = cs.cmax;
  L.parent_out = ScanParentOutput(cs.leaf == 0, cs.output, cs.sum_g, cs.sum_h, n, L.c, p);
  FinishLeafCtx(&L, p);
  // the entries (one batch of loads): the last (every stored bin), the one before it (the NaN
  // bin), the default bin and the one before it (the default bin's own sums, taken out of every
  // prefix past it as the scan leaves it out), the reverse candidate's exclusive prefix and the
  // forward candidate's inclusive one.  P[t]: stored bins <= t, the rebuilt one left out
  const int fix_t = F.mfb > 0 ? F.mfb : -1;
  const int t_r = rthr + 1 - offset, t_f = rthr - offset;
  // (unconditional loads at clamped indices, the unused ones zeroed after: one round trip)
  const XtPre zero = {0.0, 0.0, 0, 0};
  auto at = [&](int t) { return pre[min(max(t, 0), nb - 1)]; };
  const XtPre T = pre[nb - 1];
  XtPre T2 = at(nb - 2), D = at(def_t), D2 = at(def_t - 1), R = at(t_r - 1), W = at(t_f);
  if (nb < 2) T2 = zero;
  if (def_t < 0) D = zero;
  if (def_t < 1) D2 = zero;
  if (!(t_r >= 1 && t_r - 1 < nb)) R = zero;
  if (!(t_f >= 0 && t_f < nb)) W = zero;
  const double dg = D.g - D2.g, dh = D.h - D2.h;  // (exact: grid values)
  const int dc = D.c - D2.c;
  // prefix without the default bin (exact) of the bins <= t
  auto wo_def = [&](const XtPre& e, int t, double* g, double* h, int* c) {
    const bool sub = def_t >= 0 && def_t <= t;
    *g = sub ? e.g - dg : e.g;
    *h = sub ? e.h - dh : e.h;
    *c = sub ? e.c - dc : e.c;
  };
  // FixHistogram: the most frequent bin from the leaf totals (every stored bin: T), added last
  const bool fix_in = fix_t >= 0 && fix_t != def_t;
  double fix_g = 0.0, fix_h = 0.0;
  int fix_c = 0;
  if (fix_t >= 0) {
    fix_g = L.sg - T.g;
    fix_h = (L.sh - 2 * kEpsilon) - T.h;
    fix_c = RoundIntD(fix_h * L.cnt_factor);
  }
  double tot_g, tot_h;
  int tot_c;
  wo_def(T, nb - 1, &tot_g, &tot_h, &tot_c);
  if (fix_in) {
    tot_g += fix_g;
    tot_h += fix_h;
    tot_c += fix_c;
  }
  // (na: no default bin; the NaN bin is the last one -- rebuilt, or the last entry's step)
  const bool nan_fix = fix_t == nb - 1;
  const double ng = !na ? 0.0 : nan_fix ? fix_g : T.g - T2.g;
  const double nh = !na ? 0.0 : nan_fix ? fix_h : T.h - T2.h;
  const int nc = !na ? 0 : nan_fix ? fix_c : T.c - T2.c;
  const int t_start_r = nb - 1 - (na ? 1 : 0), t_end_r = 1 - offset, t_end_f = nb - 2;
  const double pr_g = na ? tot_g - ng : tot_g, pr_h = na ? tot_h - nh : tot_h;
  const int pr_c = na ? tot_c - nc : tot_c;
  const bool minus_one = na && offset == 1;
  const double lg0 = minus_one ? L.sg - T.g : 0.0;
  const double lh0 = minus_one ? L.sh - kEpsilon - T.h : kEpsilon;
  const int lc0 = minus_one ? L.n - tot_c : 0;
  const double min_h = p.min_sum_hessian_in_leaf;
  const int min_n = p.min_data_in_leaf;
  const int8_t mono = static_cast<int8_t>(F.monotone);
  double rb_gain = -INFINITY, fb_gain = -INFINITY, rb_lg = 0.0, rb_lh = 0.0, fb_lg = 0.0, fb_lh = 0.0;
  int rb_thr = -1, fb_thr = 0x7fffffff, rb_lc = 0, fb_lc = 0;
  bool any = false;
  for (int c = 0; c < 3; ++c) {  // 0: the forward start, 1: reverse, 2: forward
    bool ok;
    double xg, xh;
    int xc, thr;
    if (c == 0) {
      ok = minus_one && rthr == offset - 1;
      xg = lg0;
      xh = lh0;
      xc = lc0;
      thr = offset - 1;
    } else if (c == 1) {
      ok = t_r != def_t && t_r >= t_end_r && t_r <= t_start_r;
      double pg, ph;
      int pc;
      wo_def(R, t_r - 1, &pg, &ph, &pc);
      const bool fx = fix_in && fix_t < t_r;
      const double eg = fx ? pg + fix_g : pg, eh = fx ? ph + fix_h : ph;
      const int ec = fx ? pc + fix_c : pc;
      xg = L.sg - (pr_g - eg);
      xh = L.sh - (pr_h - eh + kEpsilon);
      xc = L.n - (pr_c - ec);
      thr = t_r - 1 + offset;
    } else {
      ok = two && t_f >= 0 && t_f != def_t && t_f <= t_end_f;
      double pg, ph;
      int pc;
      wo_def(W, t_f, &pg, &ph, &pc);
      const bool fx = fix_in && fix_t <= t_f;
      xg = lg0 + (fx ? pg + fix_g : pg);
      xh = lh0 + (fx ? ph + fix_h : ph);
      xc = lc0 + (fx ? pc + fix_c : pc);
      thr = t_f + offset;
    }
    if (!ok || xc < min_n || xh < min_h) continue;
    const int rc = L.n - xc;
    const double rh = L.sh - xh;
    if (rc < min_n || rh < min_h) continue;
    const double gain = simple ? GainOf<true>(xg, xh, L.sg - xg, rh, p.lambda_l2, p, L.c, mono, xc, rc, L.parent_out)
                               : GainOf<false>(xg, xh, L.sg - xg, rh, p.lambda_l2, p, L.c, mono, xc, rc, L.parent_out);
    if (!(gain > L.min_gain_shift)) continue;
    any = true;
    if (c == 1) {
      rb_gain = gain;
      rb_thr = thr;
      rb_lg = xg;
      rb_lh = xh;
      rb_lc = xc;
    } else {
      fb_gain = gain;
      fb_thr = thr;
      fb_lg = xg;
      fb_lh = xh;
      fb_lc = xc;
    }
  }
  FeatureBest o = FeatureBestEmpty();
  o.feature = f;
  o.real_feature = F.real_index;
  o.default_left = two ? 1 : (F.missing_type == 2 ? 0 : 1);
  o.mono = F.monotone;
  for (int d = 0; d < (two ? 2 : 1); ++d) {
    const double bg = d == 0 ? rb_gain : fb_gain;
    if (any && bg > o.gain + L.min_gain_shift) {
      const double blg = d == 0 ? rb_lg : fb_lg, blh = d == 0 ? rb_lh : fb_lh;
      const int blc = d == 0 ? rb_lc : fb_lc;
      o.thr = d == 0 ? rb_thr : fb_thr;
      o.lo = simple ? OutputOf<true>(blg, blh, p.lambda_l2, p, L.c, blc, L.parent_out)
                    : OutputOf<false>(blg, blh, p.lambda_l2, p, L.c, blc, L.parent_out);
      o.lc = blc;
      o.lg = blg;
      o.lh = blh - kEpsilon;
      o.ro = simple ? OutputOf<true>(L.sg - blg, L.sh - blh, p.lambda_l2, p, L.c, L.n - blc, L.parent_out)
                    : OutputOf<false>(L.sg - blg, L.sh - blh, p.lambda_l2, p, L.c, L.n - blc, L.parent_out);
      o.rc = L.n - blc;
      o.rg = L.sg - blg;
      o.rh = L.sh - blh - kEpsilon;
      o.gain = bg - L.min_gain_shift;
      o.default_left = d == 1 ? 0 : (!two && F.missing_type == 2 ? 0 : 1);
    }
  }
  o.gain *= F.penalty;
  if (!simple && F.monotone != 0) o.gain *= MonotonePenalty(cs.depth, a.p.monotone_penalty);
  if (o.gain == -INFINITY) o.feature = -1;
  *out = o;
  return any;
}

// (extra_trees: draw k of a feature's generator, k >= 1, as the step scans draw)
__device__ __forceinline__ int XtThreshold(const KArgs& a, const Feature& F, int f, int k) {
  const uint32_t x = LcgSkip(a.xt_base[f], k);
  return static_cast<int>(x & 0x7fffffffu) % (F.num_bin - 2);
}

}  // namespace dev
}  // namespace lgbm_amd
