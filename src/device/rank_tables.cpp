// Host-side planning of a listwise gradient launch (see rank_tables.h).
#include "rank_tables.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

#include "lgbm_amd/dcg.h"
#include "lgbm_amd/log.h"
#include "lgbm_amd/tuning.h"

#define RANKCHECK(x)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) Log::Fatal("HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); \
  } while (0)

namespace lgbm_amd {
namespace dev {

namespace {

template <typename T>
T* Upload(const RankAlloc& alloc, const T* host, size_t n) {
  T* d = static_cast<T*>(alloc(std::max<size_t>(1, n) * sizeof(T)));
  if (n > 0) RANKCHECK(hipMemcpy(d, host, sizeof(T) * n, hipMemcpyHostToDevice));
  return d;
}

}  // namespace

// query boundaries, 1 / max DCG, label gains and position discounts (lambdarank) or the
// per-query generators (xendcg; from here on they advance on the device)
RankTables UploadRankTables(const DeviceRankSpec& r, DeviceGradKind kind, int64_t num_data, const RankAlloc& alloc) {
  RankTables t;
  const size_t nq = static_cast<size_t>(r.num_queries);
  {
    std::vector<int32_t> qb(r.query_boundaries, r.query_boundaries + nq + 1);
    t.qb = Upload(alloc, qb.data(), qb.size());
  }
  if (kind == DeviceGradKind::Lambdarank) {
    t.inv_max_dcg = Upload(alloc, r.inv_max_dcg, nq);
    t.label_gain = Upload(alloc, r.label_gain, static_cast<size_t>(r.num_label_gain));
    std::vector<double> disc(std::max<data_size_t>(1, r.max_query_docs));
    for (size_t i = 0; i < disc.size(); ++i) disc[i] = DCG::Discount(static_cast<data_size_t>(i));
    t.discount = Upload(alloc, disc.data(), disc.size());
    if (r.sig_table == nullptr || r.sig_bins != kRankSigmoidBins) {
      Log::Fatal("device lambdarank: the objective's sigmoid table (%lld entries) is not the device's (%d)",
                 static_cast<long long>(r.sig_bins), kRankSigmoidBins);
    }
    t.sig_table = Upload(alloc, r.sig_table, static_cast<size_t>(r.sig_bins));
  } else if (r.rng_states != nullptr) {
    t.rng = Upload(alloc, r.rng_states, nq);
  }
  // queries longer than the LDS staging: one 1024-thread workgroup each over a global scratch;
  // the others' LDS is sized to the longest of them.  Lambdarank: the pair scratch of every
  // LDS-staged query (cnt^2 float pairs each), within a memory budget
  std::vector<int32_t> big;
  std::vector<int64_t> pair_off(nq, 0);
  int64_t pair_total = 0;
  t.max_docs = 1;
  for (size_t q = 0; q < nq; ++q) {
    const int64_t cnt = r.query_boundaries[q + 1] - r.query_boundaries[q];
    if (cnt > kRankMaxDocs) {
      big.push_back(static_cast<int32_t>(q));
      continue;
    }
    t.max_docs = std::max<int32_t>(t.max_docs, static_cast<int32_t>(cnt));
    pair_off[q] = pair_total;
    pair_total += cnt * cnt;
  }
  // budget: a share of the free memory (the histograms and round buffers are already resident),
  // capped; LGBM_AMD_RANK_PAIR_MB overrides it
  int64_t pair_budget = int64_t{tuning::kRankPairCapMb} << 20;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    pair_budget = std::min<int64_t>(pair_budget, static_cast<int64_t>(tuning::kRankPairFreeShare * free_b));
  } else {
    (void)hipGetLastError();
  }
  pair_budget = static_cast<int64_t>(tuning::Int(tuning::Knob::RankPairMb, static_cast<int>(pair_budget >> 20))) << 20;
  const int64_t pair_bytes = pair_total * static_cast<int64_t>(sizeof(float2));
  if (kind == DeviceGradKind::Lambdarank && pair_total > 0 && pair_bytes > pair_budget) {
    Log::Info("device lambdarank: pair scratch of %.1f MiB is over its %.1f MiB budget; each pair is evaluated "
              "from both of its documents", pair_bytes / 1048576.0, pair_budget / 1048576.0);
  }
  if (kind == DeviceGradKind::Lambdarank && pair_total > 0 && pair_bytes <= pair_budget) {
    t.pairs = static_cast<float2*>(alloc(static_cast<size_t>(pair_total) * sizeof(float2)));
    t.pair_off = Upload(alloc, pair_off.data(), nq);
  }
  t.num_big = static_cast<int32_t>(big.size());
  if (!big.empty()) {
    const size_t n = static_cast<size_t>(std::max<int64_t>(1, num_data));
    t.big_q = Upload(alloc, big.data(), big.size());
    t.big_d0 = static_cast<double*>(alloc(n * sizeof(double)));
    t.big_d1 = static_cast<double*>(alloc(n * sizeof(double)));
    t.big_dh = static_cast<double*>(alloc(n * sizeof(double)));
    t.big_f = static_cast<float*>(alloc(n * sizeof(float)));
    t.big_i0 = static_cast<int32_t*>(alloc(n * sizeof(int32_t)));
    t.big_i1 = static_cast<int32_t*>(alloc(n * sizeof(int32_t)));
    t.big_i2 = static_cast<int32_t*>(alloc(n * sizeof(int32_t)));
    Log::Debug("device %s: %d queries of more than %d documents in global scratch",
               kind == DeviceGradKind::Lambdarank ? "lambdarank" : "rank_xendcg", t.num_big, kRankMaxDocs);
  }
  return t;
}

MetricQueryInputs UploadMetricQueryInputs(const DeviceMetricSpec& spec, int64_t num_data, const RankAlloc& alloc) {
  MetricQueryInputs qi;
  std::vector<int32_t> qb(spec.qb, spec.qb + spec.nq + 1);
  qi.qb = Upload(alloc, qb.data(), qb.size());
  if (spec.qw != nullptr) qi.qw = Upload(alloc, spec.qw, static_cast<size_t>(spec.nq));
  std::vector<int32_t> at(spec.eval_at.begin(), spec.eval_at.end());
  qi.eval_at = Upload(alloc, at.data(), at.size());
  qi.qconst = Upload(alloc, spec.qconst.data(), spec.qconst.size());
  qi.label_gain = Upload(alloc, spec.label_gain.data(), spec.label_gain.size());
  qi.discount = Upload(alloc, spec.discount.data(), spec.discount.size());
  qi.big = spec.max_query_docs > kRankMaxDocs;
  qi.scratch = alloc(MetricScratchBytes(qi.big ? num_data : 0, static_cast<int64_t>(spec.nq) * spec.eval_at.size()));
  return qi;
}

void SetMetricQueryArgs(MetricArgs* m, const DeviceMetricSpec& spec, const MetricQueryInputs& qi) {
  m->nq = spec.nq;
  m->nk = static_cast<int32_t>(spec.eval_at.size());
  m->qb = qi.qb;
  m->qw = qi.qw;
  m->eval_at = qi.eval_at;
  m->qconst = qi.qconst;
  m->label_gain = qi.label_gain;
  m->discount = qi.discount;
  m->scratch = qi.scratch;
  m->big = qi.big ? 1 : 0;
}

}  // namespace dev
}  // namespace lgbm_amd
