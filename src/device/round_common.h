// Round growth: speculative multi-leaf expansion of leaf-wise trees (device_types.h Round).
//
// The reference grows a tree one split at a time (serial_tree_learner.cpp:152-202: argmax over
// the leaves' best splits, split it, histogram + scan its children).  On the device every such
// step is a chain of dependent kernels whose latency (~50 us) does not shrink with the leaf, so
// a 63-leaf tree was 62 latency chains.  Expanding a leaf -- partitioning its rows by its best
// split, histogramming and scanning both children -- depends on that leaf's rows only, so a
// round expands the round_k current leaves of highest gain at once:
//
//   k_round_split   the fused partition + smaller-child histogram of every expansion; the
//                   round's rows are dealt out in row blocks of one common size, each block
//                   belongs to one expansion (partition_kernels.hip k_split, per expansion)
//   k_round_reduce  exact int64 sums of the partials of expansions with many row blocks
//   k_round_find    split scans of both children of every expansion, grid (features, 2 x
//                   round_k); the last workgroup of each child folds its per-feature results
//                   into the child's best split (cbest)
//   k_round_plan    one workgroup replays the sequential best-first order over the leaves:
//                   while the argmax leaf is expanded its split is accepted (split record,
//                   children become leaves 'leaf' and s + 1 with the expansion's statistics);
//                   the first argmax leaf that is not expanded ends the replay.  Then the next
//                   round's expansions are planned: the current unexpanded leaves of highest
//                   gain (the one that ended the replay first).  The plan runs in the last
//                   workgroup of k_round_find on one process; in distributed rounds the
//                   per-feature results are gathered first, and the last workgroup of
//                   k_round_childbest (the fold of the gathered results) runs it.
//
// The accepted sequence is the sequential one: a leaf's best split and its children's results
// depend only on its own rows, and the replay uses the host loop's argmax order (gain, real
// feature, leaf id).  Expansions not accepted before the tree is full cost work only.
// Pending expansions stay valid across rounds (leaves are only ever split by their best
// split), so no expansion is computed twice.
//
// The files: round_split.hip holds k_round_split, its unfused pair k_round_part / k_round_hist
// and k_round_reduce; round_find.hip holds k_round_find, k_round_childbest and k_round_plan;
// round_plan.h holds the plan itself (the three kernels of round_find.hip run it) and
// round_xt.h its extra_trees evaluation.  This header holds what more than one stage uses.
#pragma once

#include "hist_common.h"
#include "split_scan.h"

namespace lgbm_amd {
namespace dev {

constexpr unsigned kRoundFlatMax = 128;  // split-scan grid rows up to this size count on one counter
constexpr int kRPartWaves = kPartThreads / kWave;
constexpr int kRGatherNarrow = 2, kRGatherWide = 8, kRGatherNarrowMaxWords = 8;
constexpr int kPlanThreads = 256;

__device__ __forceinline__ long long* RoundScratch(const KArgs& a, int parity, int j) {
  return a.scratch + (static_cast<size_t>(parity & 1) * a.round_k + j) * 2 * static_cast<size_t>(a.p.total_bins);
}

// a workgroup barrier ordering LDS only: nothing in the round's split kernel reads another
// wave's global stores, so the partition's stores (and the prefetched loads queued behind them
// on vmcnt) stay in flight across it -- __syncthreads' workgroup fence would drain them
__device__ __forceinline__ void LdsBarrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the split column's bin of a row without branches (ColBin's source / width branches compile
// to divergent blocks whose waits drain every load in flight): one aligned dword load and a
// shift, from the column copy or the row-major matrix
struct ColSrc {
  const uint32_t* base;  // 4-byte aligned allocation (column copy or row-major matrix)
  int64_t off0;          // byte offset of row 0's bin
  int64_t stride;        // bytes between rows
  uint32_t mask;
  uint32_t shift;        // 4-bit groups in the row-major matrix: 4 for the high half of the byte
};
__device__ __forceinline__ ColSrc ColSource(const KArgs& a, int gbyte, int gwide, int64_t col_off) {
  ColSrc c;
  const bool col = a.bins_col != nullptr;
  c.base = col ? reinterpret_cast<const uint32_t*>(a.bins_col) : static_cast<const uint32_t*>(a.bins);
  c.off0 = col ? col_off : gbyte;
  c.stride = col ? (gwide == 1 ? 2 : 1) : 4 * static_cast<int64_t>(a.row_words);
  c.mask = gwide == 1 ? 0xffffu : (gwide >= 2 && !col ? 0xfu : 0xffu);
  c.shift = gwide == 3 && !col ? 4u : 0u;
  return c;
}
// (row < 0: none -- row 0 is read and the result dropped, so the load is unconditional)
__device__ __forceinline__ uint32_t ColBinNB(const ColSrc& c, int row) {
  const int64_t off = c.off0 + static_cast<int64_t>(max(row, 0)) * c.stride;
  const uint32_t wd = c.base[off >> 2];
  const uint32_t v = (wd >> ((static_cast<uint32_t>(off) & 3u) * 8u + c.shift)) & c.mask;
  return row < 0 ? 0u : v;
}

__device__ __forceinline__ int RValidInWave(int valid, int k, int w) {
  return min(kWave, max(0, valid - k * kPartThreads - w * kWave));
}

// per-expansion constants of the split kernel, staged in LDS once per workgroup
struct SplitExp {
  int pb, pc, src, dst, blk_off, nblk, hl, single;
  int fbyte, fwide;
  int sub_lo, sub_hi, offset, mfb;
  long long fcol;
  SplitRule r;
};

// the rows of expansion j's histogrammed child after the partition: a range of the other
// index buffer
__device__ __forceinline__ int RoundHistRows(const Round* rd, int j, int* begin) {
  const ExpPlan& e = rd->e[j];
  const int tl = rd->cur[j][0];
  *begin = e.part_begin + (e.hist_left ? 0 : tl);
  return e.hist_left ? tl : e.part_count - tl;
}
// row blocks of expansion j's histogram (fused: blocks of the parent's rows)
__device__ __forceinline__ int RoundHistBlocks(const KArgs& a, const Round* rd, int j) {
  if (a.round_fused) return rd->e[j].nblk;
  int b;
  const int h = RoundHistRows(rd, j, &b);
  return (h + rd->rpb - 1) / rd->rpb;
}

// per-feature result slot of child y, inner feature f (distributed: rank-major blocks)
__device__ __forceinline__ size_t RoundFbIndex(const KArgs& a, int y, int f) {
  if (!a.round_dist || a.round_vote) return static_cast<size_t>(y) * a.p.num_features + f;
  const int fi = a.fb_index[f], per = 2 * a.max_owned;
  const int owner = fi / per, local = fi - owner * per;
  return (static_cast<size_t>(owner) * 2 * a.round_k + y) * a.max_owned + local;
}

// the round_split.hip kernels' share of PrepareRoundKernels
void PrepareRoundSplitKernels(int max_lds);

}  // namespace dev
}  // namespace lgbm_amd
