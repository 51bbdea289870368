// Stand-alone device ops over caller-owned device buffers (torch tensors on cuda), exposed
// for lightgbmv1_amd.ops: the same HIP kernels the device learner runs each iteration --
// point-wise objective gradients (src/device/objective_kernels.hip), validation metrics
// (src/device/metric_kernels.hip) and the bagging / GOSS row sampler
// (src/device/sample_kernels.hip), and with query sizes the listwise ranking gradients
// (src/device/rank_kernels.hip) and the NDCG / MAP metrics -- callable one at a time so that
// their numerics can be checked against plain PyTorch / NumPy references (tests/test_ops.py,
// tests/test_rank_ops.py); a booster's forest prediction (scores, leaf indices, SHAP
// contributions) on a matrix that already is on the device; and the two per-tree passes of a
// device refit (src/device/refit_kernels.hip: per-leaf sums, score update; tests/test_device_refit.py);
// the CSR / CSC binning kernels under a dataset's bin mappers (src/device/csr_bin_kernels.hip,
// src/device/csc_bin_kernels.hip); and the two kernels behind custom objectives and metrics on
// device tensors (src/device/custom_kernels.hip: score export with an objective's output
// transform, gradient ingest; tests/test_device_custom_objective.py).
//
// Objectives and metrics are created from a parameter string exactly as training creates
// them (reference objective_function.cpp:16-56, metric.cpp:16-63), so the kernels see the
// same DeviceGradSpec / DeviceMetricSpec.  Every op runs on the null stream and returns
// after it finished (the caller synchronises its own stream before the call).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../device/kernels.h"
#include "../device/rank_tables.h"
#include "../device/refit_quant.h"
#include "booster_device_buffers.h"
#include "lgbm_amd/c_api.h"
#include "lgbm_amd/config.h"
#include "lgbm_amd/dataset.h"
#include "lgbm_amd/device_binning.h"
#include "lgbm_amd/log.h"
#include "lgbm_amd/tuning.h"
#include "lgbm_amd/metric.h"
#include "lgbm_amd/objective.h"

using namespace lgbm_amd;

namespace {

thread_local std::string g_op_error = "Everything is fine";

#define OPCHECK(x)                                                                                  \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) Log::Fatal("HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); \
  } while (0)

template <typename F>
int Guard(F&& f) {
  try {
    f();
    return 0;
  } catch (std::exception& e) {
    g_op_error = e.what();
  } catch (...) {
    g_op_error = "unknown exception";
  }
  return -1;
}

// device scratch freed at scope exit
struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  T* Upload(const T* host, size_t n) {
    if (host == nullptr) return nullptr;
    T* p = Alloc<T>(n);
    OPCHECK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }
  template <typename T>
  T* Alloc(size_t n) {
    void* p = nullptr;
    OPCHECK(hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T)));
    ptrs.push_back(p);
    return static_cast<T*>(p);
  }
};

Config ParseConfig(const char* params) {
  Config c;
  c.Set(Config::Str2Map(params ? params : ""));
  return c;
}

void FillMetadata(Metadata* md, const float* label, const float* weight, int32_t n, const int32_t* group = nullptr,
                  int32_t num_group = 0) {
  md->Init(n, weight != nullptr, false);
  md->SetLabel(label, n);
  if (weight != nullptr) md->SetWeights(weight, n);
  if (group != nullptr && num_group > 0) md->SetQuery(group, num_group);
}

// listwise gradients (LambdaRank-NDCG / XE-NDCG) with the learner's launch plan
// (dev::UploadRankTables) over the op's own scratch; d_rng: the caller's xendcg generator
// states (advanced in place), or null for the objective's fresh ones
void RankGradientsOp(const DeviceGradSpec& spec, int32_t n, const double* d_score, float* d_grad, float* d_hess,
                     uint32_t* d_rng) {
  if (spec.rank.query_boundaries == nullptr || spec.rank.num_queries <= 0) {
    Log::Fatal("op gradients: a ranking objective needs the query sizes (group)");
  }
  Scratch sc;
  const dev::RankTables rt = dev::UploadRankTables(spec.rank, spec.kind, n, [&sc](size_t bytes) -> void* {
    return sc.Alloc<char>(bytes);
  });
  dev::PrepareRankKernels(dev::RankMaxLds());
  dev::RankArgs ra{};
  tuning::PoisonArgs(&ra);  // (every field set below)
  ra.kind = spec.kind == DeviceGradKind::Lambdarank ? dev::kRankKindLambdarank : dev::kRankKindXendcg;
  ra.num_queries = spec.rank.num_queries;
  ra.qb = rt.qb;
  ra.label = sc.Upload(spec.label, n);
  ra.weights = sc.Upload(spec.weights, n);
  ra.score = d_score;
  ra.grad = d_grad;
  ra.hess = d_hess;
  ra.inv_max_dcg = rt.inv_max_dcg;
  ra.label_gain = rt.label_gain;
  ra.discount = rt.discount;
  ra.sigmoid = spec.rank.sigmoid;
  ra.sig_min = spec.rank.sig_min;
  ra.sig_max = spec.rank.sig_max;
  ra.sig_factor = spec.rank.sig_factor;
  ra.sig_table = rt.sig_table;
  ra.norm = spec.rank.norm ? 1 : 0;
  ra.rng = d_rng != nullptr ? d_rng : rt.rng;
  ra.big_q = rt.big_q;
  ra.num_big = rt.num_big;
  ra.big_d0 = rt.big_d0;
  ra.big_d1 = rt.big_d1;
  ra.big_dh = rt.big_dh;
  ra.big_f = rt.big_f;
  ra.big_i0 = rt.big_i0;
  ra.big_i1 = rt.big_i1;
  ra.big_i2 = rt.big_i2;
  ra.max_docs = rt.max_docs;
  ra.pair_buf = rt.pairs;
  ra.pair_off = rt.pair_off;
  dev::RankGradients(ra, nullptr);
  OPCHECK(hipGetLastError());
  OPCHECK(hipDeviceSynchronize());
}

}  // namespace

LIGHTGBM_C_EXPORT const char* LGBMAMD_OpLastError() { return g_op_error.c_str(); }

// a booster's forest on a row-major float32 / float64 matrix in device memory: raw scores
// [nrow][classes], leaf indices [nrow][trees] or SHAP contributions [nrow][classes * (F + 1)]
// (predict_type: C_API_PREDICT_RAW_SCORE / LEAF_INDEX / CONTRIB) into out_len doubles of device
// memory, with the kernels of LGBM_BoosterPredictForMat's device path
LIGHTGBM_C_EXPORT int LGBMAMD_OpForestPredict(BoosterHandle handle, const void* d_data, int data_type, int64_t nrow,
                                              int32_t ncol, int predict_type, int start_iteration, int num_iteration,
                                              double* d_out, int64_t out_len) {
  return Guard([&] {
    BoosterPredictDeviceBuffers(handle, d_data, data_type, nrow, ncol, predict_type, start_iteration, num_iteration,
                                d_out, out_len);
  });
}

// the same predictions of nrow CSR rows in device memory (d_indptr: nrow + 1 int32 / int64
// entries, indptr_type C_API_DTYPE_INT32 / INT64; d_indices: int32 columns; d_data: nelem float32
// / float64 values): the rows are scattered into a compact matrix of the features the trees
// split on (src/device/csr_kernels.hip), which the forest kernels walk.  Absent entries are 0
LIGHTGBM_C_EXPORT int LGBMAMD_OpForestPredictCSR(BoosterHandle handle, const void* d_indptr, int indptr_type,
                                                 const int32_t* d_indices, const void* d_data, int data_type,
                                                 int64_t nrow, int64_t nelem, int predict_type, int start_iteration,
                                                 int num_iteration, double* d_out, int64_t out_len) {
  return Guard([&] {
    BoosterPredictCSRDeviceBuffers(handle, d_indptr, indptr_type, d_indices, d_data, data_type, nrow, nelem,
                                   predict_type, start_iteration, num_iteration, d_out, out_len);
  });
}

// ... and of the nrow rows of a CSC matrix in device memory (d_col_ptr: ncol + 1 int32 / int64
// entries; d_indices: the int32 row of each of the nelem entries; d_data: float32 / float64
// values): the columns the trees split on are scattered into the compact matrix
// (src/device/csc_kernels.hip).  An entry whose row is outside [0, nrow) is dropped
LIGHTGBM_C_EXPORT int LGBMAMD_OpForestPredictCSC(BoosterHandle handle, const void* d_col_ptr, int col_ptr_type,
                                                 const int32_t* d_indices, const void* d_data, int data_type,
                                                 int64_t ncol, int64_t nelem, int64_t nrow, int predict_type,
                                                 int start_iteration, int num_iteration, double* d_out,
                                                 int64_t out_len) {
  return Guard([&] {
    BoosterPredictCSCDeviceBuffers(handle, d_col_ptr, col_ptr_type, d_indices, d_data, data_type, ncol, nelem, nrow,
                                   predict_type, start_iteration, num_iteration, d_out, out_len);
  });
}

// the group bins of nrow CSR rows in device memory under a constructed dataset's bin mappers, by
// the kernel of LGBM_DatasetCreateFromCSR's device path (src/device/csr_bin_kernels.hip
// k_csr_to_group_bins): d_bins (device, int32) is row-major [nrow][groups of the dataset], -1 in
// the columns of groups with a categorical member -- the matrix of LGBM_AMD_CsrToGroupBins
LIGHTGBM_C_EXPORT int LGBMAMD_OpCsrGroupBins(DatasetHandle handle, const void* d_indptr, int indptr_type,
                                             const int32_t* d_indices, const void* d_data, int data_type,
                                             int64_t nrow, int64_t nelem, int32_t* d_bins) {
  return Guard([&] {
    CsrGroupBinsOnDevice(*static_cast<const Dataset*>(handle), d_indptr, indptr_type, d_indices, d_data, data_type,
                         nrow, nelem, d_bins);
  });
}

// ... and of the num_row rows of a CSC matrix in device memory (d_col_ptr: ncol_ptr int32 / int64
// entries; d_indices: the int32 row of each of the nelem entries), by the kernels of
// LGBM_DatasetCreateFromCSC's device path (src/device/csc_bin_kernels.hip) -- the matrix of
// LGBM_AMD_CscToGroupBins
LIGHTGBM_C_EXPORT int LGBMAMD_OpCscGroupBins(DatasetHandle handle, const void* d_col_ptr, int col_ptr_type,
                                             const int32_t* d_indices, const void* d_data, int data_type,
                                             int64_t ncol_ptr, int64_t nelem, int64_t num_row, int32_t* d_bins) {
  return Guard([&] {
    CscGroupBinsOnDevice(*static_cast<const Dataset*>(handle), d_col_ptr, col_ptr_type, d_indices, d_data, data_type,
                         ncol_ptr, nelem, num_row, d_bins);
  });
}

// gradients / hessians of an objective: score [num_class][n] (device, float64), grad / hess
// [num_class][n] (device, float32); label / weight / group are host arrays (the objective's
// Init reads them: label checks, MAPE weights, class counts, query boundaries).  The listwise
// objectives (lambdarank, rank_xendcg) need group, the num_group query sizes; d_rng (device,
// [num_group], or null) holds XE-NDCG's per-query generator states and is advanced in place
LIGHTGBM_C_EXPORT int LGBMAMD_OpGradients(const char* params, const float* label, const float* weight, int32_t n,
                                          const int32_t* group, int32_t num_group, const double* d_score,
                                          float* d_grad, float* d_hess, uint32_t* d_rng) {
  return Guard([&] {
    Config c = ParseConfig(params);
    std::unique_ptr<ObjectiveFunction> obj(ObjectiveFunction::CreateObjectiveFunction(c.objective, c));
    if (!obj) Log::Fatal("op gradients: no objective '%s'", c.objective.c_str());
    Metadata md;
    FillMetadata(&md, label, weight, n, group, num_group);
    obj->Init(md, n);
    const DeviceGradSpec spec = obj->DeviceSpec();
    if (spec.kind == DeviceGradKind::Lambdarank || spec.kind == DeviceGradKind::RankXendcg) {
      RankGradientsOp(spec, n, d_score, d_grad, d_hess, d_rng);
      return;
    }
    if (spec.kind == DeviceGradKind::None || spec.kind == DeviceGradKind::MulticlassOVA) {
      Log::Fatal("op gradients: objective '%s' has no device kernel", c.objective.c_str());
    }
    Scratch sc;
    dev::GradArgs g{};
    tuning::PoisonArgs(&g);  // (every field set below)
    g.kind = static_cast<int32_t>(spec.kind);
    g.num_class = spec.kind == DeviceGradKind::MulticlassSoftmax ? obj->NumModelPerIteration() : 1;
    g.num_data = n;
    g.p0 = spec.p0;
    g.p1 = spec.p1;
    g.p2 = spec.p2;
    g.lw0 = spec.label_weight[0];
    g.lw1 = spec.label_weight[1];
    g.label = sc.Upload(spec.label, n);
    g.weights = sc.Upload(spec.weights, n);
    g.label_weight = sc.Upload(spec.label_weight_arr, n);
    g.score = d_score;
    g.grad = d_grad;
    g.hess = d_hess;
    g.write_split = 1;
    g.gh = nullptr;
    g.gh_stride = 1;
    g.max_parts = nullptr;
    g.root_parts = nullptr;
    dev::Gradients(g, nullptr);
    OPCHECK(hipGetLastError());
    OPCHECK(hipDeviceSynchronize());
  });
}

// a validation metric of raw scores (device, float64, one model per iteration); params
// name the metric and the objective whose output transform applies.  NDCG / MAP need group (the
// num_group query sizes) and give one value per eval_at entry; query_weight ([num_group], or
// null) reaches them as the reference derives query weights: the float mean of the query's row
// weights, every row of a query carrying the query's weight.  out receives *out_count <= out_cap
// values
LIGHTGBM_C_EXPORT int LGBMAMD_OpMetric(const char* params, const float* label, const float* weight, int32_t n,
                                       const int32_t* group, int32_t num_group, const float* query_weight,
                                       const double* d_score, double* out, int32_t out_cap, int32_t* out_count) {
  return Guard([&] {
    Config c = ParseConfig(params);
    if (c.metric.empty()) Log::Fatal("op metric: no metric given");
    std::unique_ptr<Metric> m(Metric::CreateMetric(c.metric[0], c));
    if (!m) Log::Fatal("op metric: unknown metric '%s'", c.metric[0].c_str());
    std::unique_ptr<ObjectiveFunction> obj;
    if (!c.objective.empty() && c.objective != "none") {
      obj.reset(ObjectiveFunction::CreateObjectiveFunction(c.objective, c));
    }
    std::vector<float> row_qw;
    if (query_weight != nullptr) {
      if (group == nullptr || weight != nullptr) Log::Fatal("op metric: query weights need group and no row weights");
      for (int32_t q = 0; q < num_group; ++q) {
        row_qw.insert(row_qw.end(), static_cast<size_t>(group[q]), query_weight[q]);
      }
      if (static_cast<int64_t>(row_qw.size()) != n) Log::Fatal("op metric: the query sizes do not add up to the rows");
      weight = row_qw.data();
    }
    Metadata md;
    FillMetadata(&md, label, weight, n, group, num_group);
    m->Init(md, n);
    if (obj) obj->Init(md, n);
    const DeviceMetricSpec spec = m->DeviceSpec(obj.get());
    if (spec.kind == 0) Log::Fatal("op metric: '%s' has no device kernel for this objective", c.metric[0].c_str());
    auto give = [&](const std::vector<double>& v) {
      if (static_cast<int32_t>(v.size()) > out_cap) {
        Log::Fatal("op metric: %d values, room for %d", static_cast<int>(v.size()), out_cap);
      }
      for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
      *out_count = static_cast<int32_t>(v.size());
    };
    bool negative_weight = false;
    for (int32_t i = 0; weight != nullptr && i < n && !negative_weight; ++i) negative_weight = weight[i] < 0.0f;
    if (spec.kind == dev::kMetricAUC && negative_weight) {
      // the device AUC carries the class in the weight's sign: evaluate these rows on the host
      std::vector<double> hs(static_cast<size_t>(std::max(0, n)));
      OPCHECK(hipMemcpy(hs.data(), d_score, sizeof(double) * hs.size(), hipMemcpyDeviceToHost));
      give({m->Eval(hs.data(), obj.get())[0]});
      return;
    }
    const bool query = spec.kind == dev::kMetricNDCG || spec.kind == dev::kMetricMAP;
    if (query && (spec.qb == nullptr || spec.nq <= 0 || spec.eval_at.empty())) {
      Log::Fatal("op metric: query metrics need the query sizes (group)");
    }
    if (query && spec.max_query_docs > tuning::kQueryMetricDeviceMaxDocs) {
      Log::Fatal("op metric: a query of %d documents is over the device kernel's %d",
                 static_cast<int>(spec.max_query_docs), tuning::kQueryMetricDeviceMaxDocs);
    }
    Scratch sc;
    dev::MetricArgs a{};
    a.kind = spec.kind;
    a.convert = spec.convert;
    a.sigmoid = spec.sigmoid;
    a.param = spec.param;
    a.num_class = spec.num_class;
    a.top_k = spec.top_k;
    a.n = n;
    a.score = d_score;
    a.label = sc.Upload(spec.label, n);
    a.weights = sc.Upload(spec.weights, n);
    if (query) {
      const dev::MetricQueryInputs qi = dev::UploadMetricQueryInputs(spec, n, [&sc](size_t bytes) -> void* {
        return sc.Alloc<char>(bytes);
      });
      dev::SetMetricQueryArgs(&a, spec, qi);
    } else {
      // (AUC-mu: the class weight matrix)
      if (spec.kind == dev::kMetricAucMu) a.qconst = sc.Upload(spec.qconst.data(), spec.qconst.size());
      a.scratch = sc.Alloc<char>(dev::MetricScratchBytes(n));
    }
    const size_t nout = static_cast<size_t>(std::max(2, spec.nout));
    a.out = sc.Alloc<double>(nout);
    dev::EvalMetric(a, nullptr);
    OPCHECK(hipGetLastError());
    std::vector<double> h(nout, 0.0);
    OPCHECK(hipMemcpy(h.data(), a.out, sizeof(double) * nout, hipMemcpyDeviceToHost));
    give(m->FinishDevice(h));
  });
}

namespace {

// a caller's leaf ids (device, int32 [n]) as a staged column of a tree of num_leaves leaves
// (uint16, or int32 above 65536 leaves), through the refit's staging kernel: every id is
// checked there, and an id outside the tree is an error before any kernel indexes with it
const void* StageLeafColumn(Scratch* sc, const int32_t* d_leaf, int64_t n, int32_t num_leaves, bool* wide) {
  if (n < 0 || num_leaves <= 0) Log::Fatal("refit op: need n >= 0 rows and num_leaves > 0");
  *wide = num_leaves > 65536;
  void* column = sc->Alloc<char>(static_cast<size_t>(n) * (*wide ? sizeof(int32_t) : sizeof(uint16_t)));
  const uint32_t flags0[2] = {0u, 0xffffffffu};
  dev::RefitStageArgs a{};
  tuning::PoisonArgs(&a);  // (every field set below)
  a.src = d_leaf;
  a.src_stride = 1;
  a.rows = n;
  a.row0 = 0;
  a.num_rows = n;
  a.cols = 1;
  a.wide = *wide ? 1 : 0;
  a.num_leaves = sc->Upload(&num_leaves, 1);
  a.out = column;
  a.bad = sc->Upload(flags0, 2);
  dev::RefitStage(a, nullptr);
  OPCHECK(hipGetLastError());
  uint32_t bad = 0u;
  OPCHECK(hipMemcpy(&bad, a.bad, sizeof(bad), hipMemcpyDeviceToHost));
  if (bad != 0u) Log::Fatal("refit op: %u leaf ids are outside [0, %d)", bad, num_leaves);
  return column;
}

}  // namespace

// the launch shape of the refit kernels (tests size their inputs from it): out[0] the most
// leaves whose sums a workgroup keeps in LDS, out[1] the most workgroups of the leaf-sum pass,
// out[2] its threads per workgroup, out[3] rows in flight per thread (a thread's rows are
// out[1] * out[2] apart), out[4] the most leaves whose values the score update stages in LDS
LIGHTGBM_C_EXPORT int LGBMAMD_OpRefitLaunchInfo(int64_t* out) {
  return Guard([&] {
    out[0] = dev::kRefitLdsLeaves;
    out[1] = dev::RefitSumGrid(int64_t(1) << 40);
    out[2] = dev::kRefitThreads;
    out[3] = dev::kRefitUnroll;
    out[4] = dev::kRefitValueLdsLeaves;
  });
}

// per-leaf sums of grad / hess (device, float32 [n]) and row counts over leaf ids (device, int32
// [n]) with the refit's kernels (src/device/refit_kernels.hip): out_sums[2 * num_leaves] (host)
// receives sum g then sum h, dequantised; out_counts[num_leaves]; out_scale_exp[2]
LIGHTGBM_C_EXPORT int LGBMAMD_OpLeafSums(const int32_t* d_leaf, const float* d_grad, const float* d_hess, int64_t n,
                                         int32_t num_leaves, double* out_sums, int64_t* out_counts,
                                         int32_t* out_scale_exp) {
  return Guard([&] {
    Scratch sc;
    bool wide = false;
    const void* column = StageLeafColumn(&sc, d_leaf, n, num_leaves, &wide);
    const size_t L = static_cast<size_t>(num_leaves);
    dev::RefitSumArgs a{};
    tuning::PoisonArgs(&a);  // (every field set below)
    a.leaf = column;
    a.wide = wide ? 1 : 0;
    a.num_leaves = num_leaves;
    a.n = n;
    a.grad = d_grad;
    a.hess = d_hess;
    a.absmax = sc.Alloc<uint32_t>(2);
    a.table = sc.Alloc<long long>(3 * L + 2);
    dev::RefitLeafSums(a, nullptr);
    OPCHECK(hipGetLastError());
    std::vector<long long> t(3 * L + 2);
    OPCHECK(hipMemcpy(t.data(), a.table, sizeof(long long) * t.size(), hipMemcpyDeviceToHost));
    const int eg = static_cast<int>(t[3 * L]), eh = static_cast<int>(t[3 * L + 1]);
    const double ig = dev::RefitScale(-eg), ih = dev::RefitScale(-eh);
    for (size_t l = 0; l < L; ++l) {
      out_sums[l] = static_cast<double>(t[l]) * ig;
      out_sums[L + l] = static_cast<double>(t[L + l]) * ih;
      out_counts[l] = t[2 * L + l];
    }
    out_scale_exp[0] = eg;
    out_scale_exp[1] = eh;
  });
}

// d_score[i] += d_values[leaf[i]] in place (device: float64 [n], int32 [n], float64 [num_leaves])
LIGHTGBM_C_EXPORT int LGBMAMD_OpAddLeafValues(double* d_score, const int32_t* d_leaf, const double* d_values,
                                              int64_t n, int32_t num_leaves) {
  return Guard([&] {
    Scratch sc;
    bool wide = false;
    const void* column = StageLeafColumn(&sc, d_leaf, n, num_leaves, &wide);
    dev::RefitAddArgs a{};
    tuning::PoisonArgs(&a);  // (every field set below)
    a.leaf = column;
    a.wide = wide ? 1 : 0;
    a.num_leaves = num_leaves;
    a.n = n;
    a.values = d_values;
    a.score = d_score;
    dev::RefitAddLeafValues(a, nullptr);
    OPCHECK(hipGetLastError());
    OPCHECK(hipDeviceSynchronize());
  });
}

// one bagging (goss = 0) or GOSS (goss = 1) draw with fresh generators Random(seed + block):
// d_bag receives the in-bag rows ascending, d_oob the others; GOSS rescales the sampled
// small-gradient rows of d_grad / d_hess ([num_class][n]) in place.  label (host, [n], or null):
// balanced bagging, rows of label > 0 kept with pos_fraction and the others with neg_fraction
LIGHTGBM_C_EXPORT int LGBMAMD_OpSampleRows(int64_t n, int32_t seed, int32_t goss, int32_t num_class,
                                           double fraction, double top_rate, double other_rate, float* d_grad,
                                           float* d_hess, const float* label, double pos_fraction,
                                           double neg_fraction, int32_t* d_bag, int32_t* d_oob,
                                           int32_t* out_count) {
  return Guard([&] {
    Scratch sc;
    const int64_t nb = dev::SampleBlocks(n);
    std::vector<uint32_t> st(nb);
    for (int64_t b = 0; b < nb; ++b) st[b] = static_cast<uint32_t>(seed + static_cast<int>(b));
    dev::SampleArgs s{};
    tuning::PoisonArgs(&s);
    s.num_data = n;
    s.num_blocks = nb;
    s.goss = goss;
    s.balanced = label != nullptr ? 1 : 0;
    s.num_class = num_class;
    s.fraction = fraction;
    s.pos_fraction = pos_fraction;
    s.neg_fraction = neg_fraction;
    s.top_rate = top_rate;
    s.other_rate = other_rate;
    s.label = sc.Upload(label, static_cast<size_t>(n));
    s.grad = d_grad;
    s.hess = d_hess;
    s.rng = sc.Upload(st.data(), st.size());
    s.codes = sc.Alloc<uint8_t>(n);
    s.block_cnt = sc.Alloc<int32_t>(nb);
    s.block_off = sc.Alloc<int32_t>(nb);
    s.bag = d_bag;
    s.oob = d_oob;
    s.bag_count = sc.Alloc<int32_t>(1);
    dev::SampleRows(s, nullptr);
    OPCHECK(hipGetLastError());
    OPCHECK(hipMemcpy(out_count, s.bag_count, sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

// the output transform of objective `params` on raw scores, by the kernel that exports a
// booster's scores to a marked custom metric (src/device/custom_kernels.hip k_export_scores):
// d_score / d_out (device, float64) are class-major [num_class][n]; out_kind / out_param receive
// the transform (ObjectiveFunction::DeviceOutputKind; LGBM_AMD_ConvertScores evaluates it on the
// host).  No objective ("none"): a raw copy, kind 0
LIGHTGBM_C_EXPORT int LGBMAMD_OpConvertScores(const char* params, const double* d_score, int32_t num_class, int64_t n,
                                              double* d_out, int32_t* out_kind, double* out_param) {
  return Guard([&] {
    Config c = ParseConfig(params);
    std::unique_ptr<ObjectiveFunction> obj;
    // ("none" reaches here under its canonical name "custom")
    if (!c.objective.empty() && c.objective != "none" && c.objective != "custom") {
      obj.reset(ObjectiveFunction::CreateObjectiveFunction(c.objective, c));
      if (!obj) Log::Fatal("op convert_scores: no objective '%s'", c.objective.c_str());
    }
    double param = 0.0;
    const int kind = obj ? obj->DeviceOutputKind(&param) : 0;
    if (kind < 0 || kind > 5) {
      Log::Fatal("op convert_scores: the output transform of '%s' has no device kernel", c.objective.c_str());
    }
    if (num_class < 1 || n < 0) Log::Fatal("op convert_scores: need num_class >= 1 and n >= 0");
    if (obj && obj->NumModelPerIteration() != num_class) {
      Log::Fatal("op convert_scores: '%s' has %d scores per row, the tensor has %d", c.objective.c_str(),
                 obj->NumModelPerIteration(), num_class);
    }
    dev::ExportArgs e{};
    tuning::PoisonArgs(&e);  // (every field set below)
    e.score = d_score;
    e.out = d_out;
    e.n = n;
    e.num_class = num_class;
    e.convert = obj ? 1 : 0;
    e.kind = kind;
    e.param = param;
    dev::ExportScores(e, nullptr);
    OPCHECK(hipGetLastError());
    OPCHECK(hipDeviceSynchronize());
    if (out_kind != nullptr) *out_kind = kind;
    if (out_param != nullptr) *out_param = param;
  });
}

// len gradients and hessians (device, contiguous; dtype 0 float32, 1 float64, 2 float16,
// 3 bfloat16) into float32 d_out_grad / d_out_hess by the kernel that takes a marked custom
// objective's tensors (k_ingest_gradients)
LIGHTGBM_C_EXPORT int LGBMAMD_OpCastGradients(const void* d_grad, const void* d_hess, int32_t dtype, int64_t len,
                                              float* d_out_grad, float* d_out_hess) {
  return Guard([&] {
    if (len < 0) Log::Fatal("op cast_gradients: need len >= 0");
    dev::IngestArgs g{};
    tuning::PoisonArgs(&g);  // (every field set below)
    g.grad = d_grad;
    g.hess = d_hess;
    g.out_grad = d_out_grad;
    g.out_hess = d_out_hess;
    g.len = len;
    g.dtype = dtype;
    if (!dev::IngestGradients(g, nullptr)) Log::Fatal("op cast_gradients: dtype %d is not one of 0..3", dtype);
    OPCHECK(hipGetLastError());
    OPCHECK(hipDeviceSynchronize());
  });
}

// the launch shape of the two kernels (tests size their inputs from it): out[0] threads per
// workgroup, out[1] elements per thread and loop trip (a thread's elements are grid * out[0]
// apart), out[2] the most workgroups of a launch
LIGHTGBM_C_EXPORT int LGBMAMD_OpCustomLaunchInfo(int64_t* out) {
  return Guard([&] {
    out[0] = dev::kCustomThreads;
    out[1] = dev::kCustomPerThread;
    out[2] = dev::CustomGridCap();
  });
}
