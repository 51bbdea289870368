// Boosting drivers: GBDT and its DART / GOSS / RF variants.
// Interface and semantics follow reference include/LightGBM/boosting.h:27-315 and
// src/boosting/{gbdt,dart,goss,rf}.*: BoostFromAverage, per-class trees, bagging with
// one LCG per 1024-row block (seed bagging_seed + block), shrinkage, leaf renewal,
// early stopping on validation metrics, snapshots, text/JSON/if-else model IO.
// With device_type=gpu the training scores and gradients live in HBM, owned by the
// device learner (DeviceTreeLearner); the host keeps only trees and metric mirrors.
#pragma once

#include <fstream>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "lgbm_amd/config.h"
#include "lgbm_amd/dataset.h"
#include "lgbm_amd/device_learner.h"
#include "lgbm_amd/metric.h"
#include "lgbm_amd/objective.h"
#include "lgbm_amd/random.h"
#include "lgbm_amd/tree.h"
#include "lgbm_amd/tree_learner.h"

namespace lgbm_amd {

struct PredictionEarlyStopConfig {
  int round_period = 10;
  double margin_threshold = 10.0;
};

struct PredictionEarlyStopInstance {
  std::function<bool(const double*, int)> callback;
  int round_period = std::numeric_limits<int>::max();
};

PredictionEarlyStopInstance CreatePredictionEarlyStopInstance(const std::string& type,
                                                              const PredictionEarlyStopConfig& cfg);

// host score buffer for one dataset (class-major, num_tree_per_iteration x num_data)
class ScoreUpdater {
 public:
  ScoreUpdater(const Dataset* data, int num_tree_per_iteration);
  // a validation updater may hand its scores to the device learner (slot): updates then run
  // on the device and the host copy is refreshed when it is read
  void AttachDevice(DeviceTreeLearner* dl, int slot);
  int device_slot() const { return device_ != nullptr ? device_slot_ : -1; }
  double* score() {
    SyncFromDevice();
    return score_.data();
  }
  const double* score() const {
    const_cast<ScoreUpdater*>(this)->SyncFromDevice();
    return score_.data();
  }
  data_size_t num_data() const { return num_data_; }
  bool has_init_score() const { return has_init_score_; }
  void AddScore(double v, int tree_id);
  void MultiplyScore(double v, int tree_id);
  void AddScore(const Tree* tree, int tree_id);  // traversal of binned rows
  void AddScore(const Tree* tree, const data_size_t* idx, data_size_t n, int tree_id);
  void AddScore(const TreeLearner* learner, const Tree* tree, int tree_id);
  const Dataset* data() const { return data_; }

 private:
  void SyncFromDevice();
  const Dataset* data_;
  data_size_t num_data_;
  int num_tree_per_iteration_ = 1;
  std::vector<double> score_;
  bool has_init_score_ = false;
  DeviceTreeLearner* device_ = nullptr;
  int device_slot_ = -1;
  bool host_stale_ = false;
};

// what a device prediction computes (GBDT::PredictDenseOnDevice)
enum class DevicePredictKind { Normal, Raw, Leaf, Contrib };

class GBDT {
 public:
  GBDT();
  virtual ~GBDT();

  // ---- training
  virtual void Init(const Config* config, const Dataset* train_data, const ObjectiveFunction* objective,
                    const std::vector<const Metric*>& training_metrics);
  virtual void ResetTrainingData(const Dataset* train_data, const ObjectiveFunction* objective,
                                 const std::vector<const Metric*>& training_metrics);
  virtual void ResetConfig(const Config* config);
  virtual void AddValidDataset(const Dataset* valid_data, const std::vector<const Metric*>& valid_metrics);
  void Train(int snapshot_freq, const std::string& model_output_path);
  virtual bool TrainOneIter(const score_t* gradients, const score_t* hessians);
  // one iteration from a custom objective's gradients / hessians in device memory (len =
  // num_data * num_tree_per_iteration of dtype 0 float32 / 1 float64 / 2 float16 / 3 bfloat16,
  // class-major and contiguous): the device learner converts them into its own arrays
  // (DeviceTreeLearner::IngestGradients) and the iteration runs as TrainOneIter does with a
  // custom objective's host gradients, without their upload.  Needs a device learner
  virtual bool TrainOneIterDevice(const void* d_grad, const void* d_hess, int dtype, int64_t len);
  virtual void RollbackOneIter();
  // new leaf values for every tree from the training data's leaf matrix (row-major
  // [nrow][ncol], one column per tree: the C API's layout); the vector form wraps it
  void RefitTree(const int32_t* tree_leaf_prediction, int32_t nrow, int32_t ncol);
  void RefitTree(const std::vector<std::vector<int>>& tree_leaf_prediction);
  virtual bool EvalAndCheckEarlyStopping();
  int GetCurrentIteration() const { return static_cast<int>(models_.size()) / num_tree_per_iteration_; }
  void MergeFrom(const GBDT* other);
  void ShuffleModels(int start_iter, int end_iter);

  // ---- evaluation
  std::vector<double> GetEvalAt(int data_idx);
  virtual const double* GetTrainingScore(int64_t* out_len);
  void GetPredictAt(int data_idx, double* out, int64_t* out_len);
  // GetPredictAt into out_len = GetNumPredictAt(data_idx) doubles of device memory (convert:
  // through the objective's output transform where GetPredictAt applies it, else raw).  The
  // training scores and the validation sets that live on the device are exported from HBM
  // (src/device/custom_kernels.hip); a validation set kept on the host, or an objective whose
  // transform has no device form, is evaluated on the host and uploaded.  Needs a device learner
  void GetPredictAtDevice(int data_idx, bool convert, double* d_out, int64_t out_len);
  int DeviceLearnerId() const;  // the HIP device of the device learner, or -1
  // process-wide: scores exported by the kernel / gradients ingested (tests: the device path ran)
  static void DeviceCustomStats(int64_t* exports, int64_t* ingests);
  int64_t GetNumPredictAt(int data_idx) const;
  int GetEvalCounts() const;
  std::vector<std::string> GetEvalNames() const;

  // ---- prediction
  void InitPredict(int start_iteration, int num_iteration, bool is_pred_contrib);
  // InitPredict(start_iteration, num_iteration, false) would change nothing
  bool PredictRangeIs(int start_iteration, int num_iteration) const;
  // predictions of a dense float32 / float64 matrix on the MI355X: normal / raw scores and leaf
  // indices as the host predictor gives them, contributions from per-leaf path tables (equal to
  // the host's recursion up to rounding).  Rows pass through the device in chunks that fit its
  // free memory (src/boosting/predict_chunks.h is the rule, for the CSR and CSC entries below
  // too).  false if not applicable: no device, too many classes, not even one tile of rows fits
  // the free memory, or for contributions a path longer than the kernel holds or a node without
  // data_count (the host then predicts)
  bool PredictDenseOnDevice(const void* data, bool is_double, int64_t nrow, int ncol, bool row_major,
                            int start_iteration, int num_iteration, DevicePredictKind kind, double* out);
  // the same kernels on a row-major matrix in device memory, into out_len doubles of device
  // memory (raw scores, leaf indices or contributions); what is not applicable is an error
  void PredictDeviceBuffers(const void* d_data, bool is_double, int64_t nrow, int ncol, int start_iteration,
                            int num_iteration, DevicePredictKind kind, double* d_out, int64_t out_len);
  // the same predictions of the rows of a host CSR matrix (indptr int32 / int64, nindptr = rows +
  // 1 entries): each chunk of rows is scattered on the device into a compact matrix of the
  // features the window's trees split on, which the same kernels walk.  Absent entries are 0,
  // columns the model does not have are ignored, the last stored entry of a column wins.  false
  // as for the dense matrix, or when indptr does not ascend within nelem
  bool PredictCSROnDevice(const void* indptr, bool indptr_is_64, const int32_t* indices, const void* data,
                          bool is_double, int64_t nindptr, int64_t nelem, int start_iteration, int num_iteration,
                          DevicePredictKind kind, double* out);
  // ... and of CSR arrays in device memory into out_len doubles of device memory; what is not
  // applicable is an error
  void PredictCSRDeviceBuffers(const void* d_indptr, bool indptr_is_64, const int32_t* d_indices, const void* d_data,
                               bool is_double, int64_t nrow, int64_t nelem, int start_iteration, int num_iteration,
                               DevicePredictKind kind, double* d_out, int64_t out_len);
  // the compact matrix of host CSR rows evaluated on the host (tests; needs no device): the
  // sorted features the window's trees split on into `used` (room for every feature, or null) and
  // their count into *num_used; with `matrix` (row-major [rows][*num_used], of the data's type)
  // the rows' values of those features
  void CsrToSlotsOnHost(const void* indptr, bool indptr_is_64, const int32_t* indices, const void* data,
                        bool is_double, int64_t nindptr, int64_t nelem, int start_iteration, int num_iteration,
                        int32_t* num_used, int32_t* used, void* matrix);
  // the same predictions of the num_row rows of a host CSC matrix (col_ptr int32 / int64, ncol_ptr
  // = columns + 1 entries; indices: the row of each entry): only the stored entries of the columns
  // the window's trees split on go to the device, where they stay for the call, and each chunk of
  // rows is scattered from them into the compact matrix.  Absent entries are 0, columns the model
  // does not have are ignored, an entry whose row is outside the matrix is dropped, and of several
  // stored entries on one cell the last stored one wins.  false as for the CSR matrix (the resident
  // entries count against the free memory)
  bool PredictCSCOnDevice(const void* col_ptr, bool col_ptr_is_64, const int32_t* indices, const void* data,
                          bool is_double, int64_t ncol_ptr, int64_t nelem, int64_t num_row, int start_iteration,
                          int num_iteration, DevicePredictKind kind, double* out);
  // ... and of CSC arrays in device memory (the pointer of all ncol columns) into out_len doubles
  // of device memory; what is not applicable is an error
  void PredictCSCDeviceBuffers(const void* d_col_ptr, bool col_ptr_is_64, const int32_t* d_indices,
                               const void* d_data, bool is_double, int64_t ncol, int64_t nelem, int64_t nrow,
                               int start_iteration, int num_iteration, DevicePredictKind kind, double* d_out,
                               int64_t out_len);
  // the compact matrix of the rows [row0, row0 + rows) of a host CSC matrix evaluated on the host
  // (tests; needs no device), as CsrToSlotsOnHost gives it for CSR rows
  void CscToSlotsOnHost(const void* col_ptr, bool col_ptr_is_64, const int32_t* indices, const void* data,
                        bool is_double, int64_t ncol_ptr, int64_t nelem, int64_t row0, int64_t rows,
                        int start_iteration, int num_iteration, int32_t* num_used, int32_t* used, void* matrix);
  // predictions this process has computed on the device (tests: which path a call took)
  static int64_t DevicePredictions();
  // contributions of row-major float64 host rows from the path tables the device kernel reads,
  // evaluated on the host with the kernel's arithmetic (tests; needs no device)
  void ContribFromPathTables(const double* data, int64_t nrow, int ncol, int start_iteration, int num_iteration,
                             double* out);
  int NumPredictOneRow(int start_iteration, int num_iteration, bool is_pred_leaf, bool is_pred_contrib) const;
  void PredictRaw(const double* features, double* output, const PredictionEarlyStopInstance* es) const;
  void Predict(const double* features, double* output, const PredictionEarlyStopInstance* es) const;
  void PredictLeafIndex(const double* features, double* output) const;
  void PredictContrib(const double* features, double* output) const;
  void PredictRawByMap(const std::unordered_map<int, double>& f, double* output,
                       const PredictionEarlyStopInstance* es) const;
  void PredictByMap(const std::unordered_map<int, double>& f, double* output,
                    const PredictionEarlyStopInstance* es) const;
  void PredictLeafIndexByMap(const std::unordered_map<int, double>& f, double* output) const;
  void PredictContribByMap(const std::unordered_map<int, double>& f,
                           std::vector<std::unordered_map<int, double>>* output) const;

  // ---- model IO
  std::string SaveModelToString(int start_iteration, int num_iteration, int importance_type) const;
  bool SaveModelToFile(int start_iteration, int num_iteration, int importance_type, const char* filename) const;
  bool LoadModelFromString(const char* buffer, size_t len);
  std::string DumpModel(int start_iteration, int num_iteration, int importance_type) const;
  std::string ModelToIfElse(int num_iteration) const;
  bool SaveModelToIfElse(int num_iteration, const char* filename) const;
  std::vector<double> FeatureImportance(int num_iteration, int importance_type) const;
  double GetUpperBoundValue() const;
  double GetLowerBoundValue() const;
  double GetLeafValue(int tree_idx, int leaf_idx) const;
  void SetLeafValue(int tree_idx, int leaf_idx, double val);

  // ---- introspection
  int NumberOfTotalModel() const { return static_cast<int>(models_.size()); }
  int NumModelPerIteration() const { return num_tree_per_iteration_; }
  int NumberOfClasses() const { return num_class_; }
  int MaxFeatureIdx() const { return max_feature_idx_; }
  int LabelIdx() const { return label_idx_; }
  const std::vector<std::string>& FeatureNames() const { return feature_names_; }
  const std::vector<std::string>& FeatureInfos() const { return feature_infos_; }
  const Tree* model(int i) const { return models_[i].get(); }
  DeviceTreeLearner* device_learner() const { return device_learner_; }
  bool average_output() const { return average_output_; }
  const ObjectiveFunction* objective() const { return objective_; }
  std::string SubModelName() const { return "tree"; }
  const char* Name() const { return name_.c_str(); }
  const std::string& loaded_parameter() const { return loaded_parameter_; }
  bool NeedAccuratePrediction() const {
    return objective_ == nullptr || objective_->NeedAccuratePrediction();
  }

  static GBDT* CreateBoosting(const std::string& type, const char* model_filename);

 protected:
  // hook run before gradients are computed from the training score (DART drops trees here)
  virtual void PrepareScoreForGradients() {}
  virtual void Boosting();
  // TrainOneIter; ingested: the gradients are the device learner's own arrays, already filled
  bool TrainOneIterBody(const score_t* gradients, const score_t* hessians, bool ingested);
  virtual void Bagging(int iter);
  virtual data_size_t BaggingHelper(data_size_t start, data_size_t cnt, data_size_t* buffer);
  void ResetBaggingConfig(const Config* config, bool is_change_dataset);
  double BoostFromAverage(int class_id, bool update_scorer);
  void UpdateScore(const Tree* tree, int cur_tree_id);
  std::string OutputMetric(int iter);
  virtual bool GetIsConstHessian(const ObjectiveFunction* obj) { return obj != nullptr && obj->IsConstantHessian(); }
  // training score helpers (host or device resident)
  void TrainScoreAdd(double v, int tree_id);
  void TrainScoreMultiply(double v, int tree_id);
  void TrainScoreAddTree(const Tree* tree, int tree_id);
  double* HostTrainScore();
  // RefitTree on the device learner (one process); false: the learner can not, nothing changed
  bool RefitTreeOnDevice(const int32_t* leaf_pred, int32_t nrow, int32_t ncol);
  void MarkHostScoreStale() { host_score_fresh_ = false; }
  // run the bagging pass over all rows with `helper`, filling bag_data_indices_
  data_size_t RunBagging(const std::function<data_size_t(data_size_t, data_size_t, data_size_t*)>& helper);

  std::string name_ = "gbdt";
  int iter_ = 0;
  const Dataset* train_data_ = nullptr;
  std::unique_ptr<Config> config_;
  std::unique_ptr<TreeLearner> tree_learner_;
  // LGBM_AMD_ITER_LOG=<path>: one JSON line per boosting iteration (phase times, trees, device
  // collectives); distributed ranks write <path>.rank<r>
  std::unique_ptr<std::ofstream> iter_log_;
  double growth_stats_[7] = {0, 0, 0, 0, 0, 0, 0};
  bool iter_log_checked_ = false;
  void LogIteration(double grad_ms, double bag_ms, const std::vector<double>& tree_ms, double renew_ms,
                    double score_ms, double total_ms, const std::vector<int>& leaves, const std::vector<int>& device,
                    const std::vector<int>& rounds, const std::vector<int>& expansions, const std::vector<int>& graphs,
                    double coll_bytes);
  DeviceTreeLearner* device_learner_ = nullptr;
  // whether the device learner may launch the next iteration's tree before it is asked for:
  // plain boosting whose next tree depends on nothing but this tree's score update -- no
  // bagging, leaf renewal, custom gradients or dropped trees (DART / GOSS / RF: false)
  virtual bool SpeculationSafe(bool own_gradients) const;
  const ObjectiveFunction* objective_ = nullptr;
  std::unique_ptr<ObjectiveFunction> loaded_objective_;
  std::vector<const Metric*> training_metrics_;
  std::vector<std::vector<const Metric*>> valid_metrics_;
  std::unique_ptr<ScoreUpdater> train_score_updater_;
  bool host_score_fresh_ = true;
  std::vector<std::unique_ptr<ScoreUpdater>> valid_score_updater_;
  std::vector<std::vector<double>> best_score_;
  std::vector<std::vector<int>> best_iter_;
  std::vector<std::vector<std::string>> best_msg_;
  std::vector<std::unique_ptr<Tree>> models_;
  int early_stopping_round_ = 0;
  bool es_first_metric_only_ = false;
  int max_feature_idx_ = 0;
  int label_idx_ = 0;
  int num_class_ = 1;
  int num_tree_per_iteration_ = 1;
  data_size_t num_data_ = 0;
  double shrinkage_rate_ = 0.1;
  int num_iteration_for_pred_ = 0;
  int start_iteration_for_pred_ = 0;
  // InitPredict, then the trees of the prediction window in model order
  std::vector<const Tree*> PredictWindowTrees(int start_iteration, int num_iteration);
  // what the three Predict*OnDevice entries share (src/boosting/device_predict.cpp, where the row
  // sources of the input layouts are): device probe, forest upload, the chunk plan, the loop over
  // the chunks, the output transform
  template <typename Source>
  bool PredictChunksOnDevice(Source* src, int64_t nrow, int start_iteration, int num_iteration,
                             DevicePredictKind kind, double* out);
  // ... and the three Predict*DeviceBuffers entries: the window's forest on the null stream, after
  // the checks of kind, class count and out_len
  template <typename Forest>
  void UploadForDeviceBuffers(Forest* forest, DevicePredictKind kind, bool slots, int64_t nrow, int64_t out_len,
                              int start_iteration, int num_iteration);
  int num_init_iteration_ = 0;
  std::vector<std::string> feature_names_;
  std::vector<std::string> feature_infos_;
  std::vector<int8_t> monotone_constraints_;
  std::vector<score_t> gradients_, hessians_;

 public:
  // the host learner's gradients of the last iteration (tests: device vs host objectives)
  const std::vector<score_t>& host_gradients() const { return gradients_; }
  // LGBM_AMD_BoosterGrowthStats: [trees, device-resident, rounds, expansions, splits, collective bytes,
  // trees launched speculatively]
  const double* growth_stats() const { return growth_stats_; }
  const std::vector<score_t>& host_hessians() const { return hessians_; }
  data_size_t train_num_data() const { return num_data_; }

 protected:
  std::vector<data_size_t> bag_data_indices_;
  data_size_t bag_data_cnt_ = 0;
  std::vector<Random> bagging_rands_;
  static constexpr data_size_t kBaggingRandBlock = 1024;
  bool balanced_bagging_ = false;
  bool need_re_bagging_ = false;
  // device bagging / GOSS: the device generators restart (seed + block) when the host's would
  bool device_sampler_reset_ = true;
  int device_sampler_seed_ = 0;
  // a device draw of the bag (or -1: draw on the host)
  data_size_t DeviceBagging(bool goss);
  // metric j of validation set i: on the device when its scores live there, else on the host
  std::vector<double> EvalValid(int i, int j) const;
  std::vector<double> EvalTrain(const Metric* m);  // device-resident training scores when possible
  std::vector<bool> class_need_train_;
  bool is_constant_hessian_ = false;
  bool average_output_ = false;
  std::string loaded_parameter_;
  std::string forced_splits_text_;
};

class DART : public GBDT {
 public:
  DART() { name_ = "dart"; }
  bool SpeculationSafe(bool) const override { return false; }
  void Init(const Config* config, const Dataset* train_data, const ObjectiveFunction* objective,
            const std::vector<const Metric*>& training_metrics) override;
  void ResetConfig(const Config* config) override;
  bool TrainOneIter(const score_t* gradients, const score_t* hessians) override;
  bool TrainOneIterDevice(const void* d_grad, const void* d_hess, int dtype, int64_t len) override;
  const double* GetTrainingScore(int64_t* out_len) override;
  bool EvalAndCheckEarlyStopping() override;

 protected:
  void PrepareScoreForGradients() override;

 private:
  void DroppingTrees();
  void Normalize();
  std::vector<double> tree_weight_;
  double sum_weight_ = 0;
  std::vector<int> drop_index_;
  Random random_for_drop_;
  bool is_update_score_cur_iter_ = false;
};

class GOSS : public GBDT {
 public:
  GOSS() { name_ = "goss"; }
  bool SpeculationSafe(bool) const override { return false; }
  void Init(const Config* config, const Dataset* train_data, const ObjectiveFunction* objective,
            const std::vector<const Metric*>& training_metrics) override;
  void ResetTrainingData(const Dataset* train_data, const ObjectiveFunction* objective,
                         const std::vector<const Metric*>& training_metrics) override;
  void ResetConfig(const Config* config) override;
  bool TrainOneIter(const score_t* gradients, const score_t* hessians) override;

 protected:
  void Bagging(int iter) override;
  data_size_t BaggingHelper(data_size_t start, data_size_t cnt, data_size_t* buffer) override;
  bool GetIsConstHessian(const ObjectiveFunction*) override { return false; }

 private:
  void ResetGoss();
};

class RF : public GBDT {
 public:
  bool SpeculationSafe(bool) const override { return false; }
  RF() {
    name_ = "rf";
    average_output_ = true;
  }
  void Init(const Config* config, const Dataset* train_data, const ObjectiveFunction* objective,
            const std::vector<const Metric*>& training_metrics) override;
  void ResetConfig(const Config* config) override;
  void ResetTrainingData(const Dataset* train_data, const ObjectiveFunction* objective,
                         const std::vector<const Metric*>& training_metrics) override;
  bool TrainOneIter(const score_t* gradients, const score_t* hessians) override;
  bool TrainOneIterDevice(const void* d_grad, const void* d_hess, int dtype, int64_t len) override;
  void RollbackOneIter() override;
  void AddValidDataset(const Dataset* valid_data, const std::vector<const Metric*>& valid_metrics) override;

 protected:
  void Boosting() override;

 private:
  void MultiplyScore(int cur_tree_id, double val);
  std::vector<double> init_scores_;
};

}  // namespace lgbm_amd
