// Host-side planning of a listwise gradient launch (src/device/rank_kernels.hip), shared by
// the device learner (GPUTreeLearner::ComputeGradients) and the stand-alone op
// (LGBMAMD_OpGradients): the query tables uploaded once per dataset, the queries too long for
// the LDS staging and their global scratch, and lambdarank's pair scratch within its budget.
// Likewise the query inputs of the NDCG / MAP metric kernels (GPUTreeLearner::ValidEval and
// LGBMAMD_OpMetric).
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>

#include "kernels.h"
#include "lgbm_amd/metric.h"
#include "lgbm_amd/objective.h"

namespace lgbm_amd {
namespace dev {

// device copies of a DeviceRankSpec and the launch plan over them (the RankArgs fields that do
// not change between iterations)
struct RankTables {
  int32_t* qb = nullptr;           // [num_queries + 1]
  double* inv_max_dcg = nullptr;   // lambdarank
  double* label_gain = nullptr;    // lambdarank
  double* discount = nullptr;      // lambdarank: [max(1, max_query_docs)]
  double* sig_table = nullptr;     // lambdarank: the objective's sigmoid table
  uint32_t* rng = nullptr;         // xendcg: [num_queries] LCG states, advanced on the device from here on
  // queries of more than kRankMaxDocs documents and their [num_data] scratch (RankArgs::big_*)
  int32_t* big_q = nullptr;
  int32_t num_big = 0;
  double *big_d0 = nullptr, *big_d1 = nullptr, *big_dh = nullptr;
  float* big_f = nullptr;
  int32_t *big_i0 = nullptr, *big_i1 = nullptr, *big_i2 = nullptr;
  int32_t max_docs = 0;            // most documents of a query staged in LDS
  float2* pairs = nullptr;         // lambdarank pair scratch (RankArgs::pair_buf), or null
  int64_t* pair_off = nullptr;
};

// device memory of `bytes` bytes (at least 1) that the caller owns and frees
using RankAlloc = std::function<void*(size_t bytes)>;

// Uploads r's tables and plans the launch for `kind` (Lambdarank / RankXendcg) over num_data
// rows (the size of the long queries' scratch arrays).
RankTables UploadRankTables(const DeviceRankSpec& r, DeviceGradKind kind, int64_t num_data, const RankAlloc& alloc);

// one query metric's device inputs (NDCG / MAP): the copies of a DeviceMetricSpec's query fields
struct MetricQueryInputs {
  int32_t* qb = nullptr;
  float* qw = nullptr;
  int32_t* eval_at = nullptr;
  double* qconst = nullptr;
  double* label_gain = nullptr;
  double* discount = nullptr;
  void* scratch = nullptr;
  bool big = false;  // a query longer than the LDS staging
};

// Uploads the query fields of an NDCG / MAP spec over num_data rows and allocates the kernel's
// scratch (MetricScratchBytes(num_data if a query is over kRankMaxDocs else 0, nq * nk)).
MetricQueryInputs UploadMetricQueryInputs(const DeviceMetricSpec& spec, int64_t num_data, const RankAlloc& alloc);
// the query fields of m (nq, nk, qb, qw, eval_at, qconst, label_gain, discount, scratch, big)
void SetMetricQueryArgs(MetricArgs* m, const DeviceMetricSpec& spec, const MetricQueryInputs& qi);

}  // namespace dev
}  // namespace lgbm_amd
