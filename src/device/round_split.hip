// Round growth, stage 1 (round_common.h): the fused partition + histogram kernel k_round_split,
// the unfused pair k_round_part / k_round_hist, and k_round_reduce.
#include "round_common.h"

namespace lgbm_amd {
namespace dev {

#ifndef LGBM_ORACLE_SEQ
#define LGBM_ORACLE_SEQ 0  // A/B timing oracles only: 1 sequential (g, h) gathers, 2 also sequential row words
#endif

// ---------------------------------------------------------------------------- k_round_split
// grid (split_grid, hist_tiles) of 1024-thread workgroups.  Row block kb of the round belongs
// to the expansion j with blk_off[j] <= kb < blk_off[j] + nblk[j]; it holds rows
// [(kb - blk_off[j]) * rpb, +rpb) of the expansion's parent range, processed in sub-tiles of
// kSplitSub rows exactly like k_split: sides by the split rule, per-wave ballots, one
// reservation per side and sub-tile on the expansion's cursors (lefts from the front of the
// range, rights from its back, in the other index buffer), the histogrammed child's rows
// compacted into an LDS row list and gathered into the tile's LDS histogram, stored as
// partial kb.  Only column tile 0 writes the partition.
#ifndef LGBM_SPLIT_WAVES
#define LGBM_SPLIT_WAVES 1  // waves per SIMD the register budget targets (A/B: 8 = two workgroups per CU)
#endif
template <int GPW, int UNITS, int GR, bool VOTE = false>
__global__ __launch_bounds__(kPartThreads) __attribute__((amdgpu_waves_per_eu(LGBM_SPLIT_WAVES))) void k_round_split(KArgs a) {
  extern __shared__ unsigned long long lds[];  // [UNITS * tile_bins] histogram, then the row list
  __shared__ SplitExp ex[kMaxRoundExp];
  __shared__ uint32_t cat_bits[kMaxRoundExp][kMaxCatWords];
  __shared__ int wl[kSplitRows][kRPartWaves];
  __shared__ int lpre[kSplitRows][kRPartWaves];
  __shared__ int hpre[kSplitRows][kRPartWaves];
  __shared__ int base[2];
  __shared__ int nh_s;
  Round* rd = a.rd;
  const int done = rd->done;
  const int nexp = rd->nexp, nblk = rd->nblk, rpb = rd->rpb;
  TileCtx t;
  InitTile<GPW>(a, &t);
  // the expansions' plans are loaded in the same batch as the round record (a slot past nexp
  // holds a stale plan that is never staged)
  SplitExp x;
  if (threadIdx.x < static_cast<unsigned>(kMaxRoundExp)) {
    const ExpPlan& e = rd->e[threadIdx.x];
    x.pb = e.part_begin;
    x.pc = e.part_count;
    x.src = e.src_buf;
    x.dst = e.dst_buf;
    x.blk_off = e.blk_off;
    x.nblk = e.nblk;
    x.hl = e.hist_left;
    x.single = e.nblk == 1 && e.part_count <= kSplitSub;
    x.fbyte = e.feat.gbyte;
    x.fwide = e.feat.gwide;
    x.fcol = e.feat.col_off;
    x.sub_lo = e.feat.sub_lo;
    x.sub_hi = e.feat.sub_hi;
    x.offset = e.feat.offset;
    x.mfb = e.feat.mfb;
    x.r.threshold = e.split.threshold;
    x.r.default_left = e.split.default_left;
    x.r.is_cat = e.split.is_categorical;
    x.r.missing_type = e.feat.missing_type;
    x.r.default_bin = e.feat.default_bin;
    x.r.max_bin = e.feat.num_bin - 1;
  }
  if (done || nexp <= 0 || static_cast<int>(blockIdx.x) >= nblk) return;
  if (threadIdx.x < static_cast<unsigned>(nexp)) ex[threadIdx.x] = x;
  for (int i = threadIdx.x; i < nexp * kMaxCatWords; i += kPartThreads) {
    const int j = i / kMaxCatWords;
    cat_bits[j][i % kMaxCatWords] = rd->e[j].split.is_categorical ? rd->e[j].split.cat_bits[i % kMaxCatWords] : 0u;
  }
  LdsBarrier();
  // LGBM_AMD_KTRACE: phase times of workgroup (0, 0) per round (wall clock, 10 ns ticks):
  // [stage, side, reserve, write, gather, tail, store, sub-tiles, rows, total]
  const bool tr = a.ktrace != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && rd->round < a.p.num_leaves;
  long long tacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  long long tprev = 0, tstart = 0;
  if (tr) {
    tstart = wall_clock64();
    tprev = tstart;
  }
  auto stamp = [&](int k) {
    if (tr) {
      const long long now = wall_clock64();
      tacc[k] += now - tprev;
      tprev = now;
    }
  };
  stamp(0);
  // the expansion of row block kb
  auto exp_of = [&](int kb) {
    int j = 0;
    while (j + 1 < nexp && kb >= ex[j + 1].blk_off) ++j;
    return j;
  };
  int* rowlist = reinterpret_cast<int*>(lds + static_cast<size_t>(UNITS) * a.tile_bins);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const bool writer = blockIdx.y == 0;
  // voting-parallel: the histogrammed rows' fixed-point (g, h), summed per row block by the
  // threads of word 0 of column tile 0 (each row once) -- that child's local sums
  // (a template flag: the accumulators cost the other variants registers -- Epsilon-shaped
  // wide rows 10.6 vs 11.8 ms/iter with a run-time flag)
  const bool loc_sums = VOTE && writer;
  long long loc_g = 0, loc_h = 0;
  int row[kSplitRows];
  uint32_t gb[kSplitRows];
  auto load_rows = [&](int jn, int t0n, int r1n, int* rr) {
    const int vn = min(kSplitSub, r1n - t0n);
    const int32_t* s = RowBuf(a, ex[jn].src);
    const int pbn = ex[jn].pb;
#pragma unroll
    for (int k = 0; k < kSplitRows; ++k) {
      const int i = k * kPartThreads + threadIdx.x;
      rr[k] = i < vn ? s[pbn + t0n + i] : -1;
    }
  };
  auto col_bins = [&](int jn, const int* rr, uint32_t* g) {
    const ColSrc c = ColSource(a, ex[jn].fbyte, ex[jn].fwide, ex[jn].fcol);
#pragma unroll
    for (int k = 0; k < kSplitRows; ++k) g[k] = ColBinNB(c, rr[k]);
  };
  {
    const int j = exp_of(blockIdx.x);
    const int r0 = (blockIdx.x - ex[j].blk_off) * rpb;
    load_rows(j, r0, min(ex[j].pc, r0 + rpb), row);
    col_bins(j, row, gb);
  }
  for (int kb = blockIdx.x; kb < nblk; kb += gridDim.x) {
    const int j = exp_of(kb);
    const SplitExp& X = ex[j];
    const int r0 = (kb - X.blk_off) * rpb, r1 = min(X.pc, r0 + rpb);
    const bool hl = X.hl != 0;
    Feature F;
    F.sub_lo = X.sub_lo;
    F.sub_hi = X.sub_hi;
    F.offset = X.offset;
    F.mfb = X.mfb;
    const SplitRule r = X.r;
    const uint32_t* cb = cat_bits[j];
    int32_t* dst = RowBuf(a, X.dst);
    for (int t0 = r0; t0 < r1; t0 += kSplitSub) {
      const int valid = min(kSplitSub, r1 - t0);
      // the next sub-tile of this workgroup: this block's next one, or the next block's first
      int nj = j, nt0 = t0 + kSplitSub, nr1 = r1;
      if (nt0 >= r1) {
        const int nkb = kb + gridDim.x;
        if (nkb < nblk) {
          nj = exp_of(nkb);
          nt0 = (nkb - ex[nj].blk_off) * rpb;
          nr1 = min(ex[nj].pc, nt0 + rpb);
        } else {
          nt0 = nr1 = 0;
        }
      }
      int nrow[kSplitRows];
      load_rows(nj, nt0, nr1, nrow);
      if (t0 == r0) {
        LdsBarrier();  // the previous block's partial was stored from this LDS
        for (int i = threadIdx.x; i < UNITS * t.nbins; i += kPartThreads) lds[i] = 0ull;
      }
      // ---- sides (this sub-tile's split-column bins were loaded during the previous one)
      bool left[kSplitRows];
      unsigned long long mask[kSplitRows];
#pragma unroll
      for (int k = 0; k < kSplitRows; ++k) {
        left[k] = row[k] >= 0 && GoesLeft(r, cb, FeatureBinOf(F, gb[k]));
        mask[k] = __ballot(left[k]);
      }
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kSplitRows; ++k) wl[k][w] = __popcll(mask[k]);
      }
      LdsBarrier();
      stamp(1);
      if (tr) {
        tacc[7] += 1;
        tacc[8] += valid;
      }
      // ---- prefixes; the reservation is issued now and consumed after the gathers (its round
      // trip overlaps them)
      int res_l = 0, res_r = 0;
      int nl_w0 = 0;
      if (w == 0) {
        const int k = lane / kRPartWaves, jj = lane % kRPartWaves;
        const int c = wl[k][jj];
        const int hc = hl ? c : RValidInWave(valid, k, jj) - c;
        const int ci = WavePrefixIncl(c), hi = WavePrefixIncl(hc);
        lpre[k][jj] = ci - c;
        hpre[k][jj] = hi - hc;
        nl_w0 = __shfl(ci, kWave - 1, kWave);
        if (lane == kWave - 1) nh_s = hi;
      }
      LdsBarrier();
      stamp(2);
      const int nh = nh_s;
#pragma unroll
      for (int k = 0; k < kSplitRows; ++k) {
        const unsigned long long vm = __ballot(row[k] >= 0);
        const unsigned long long hm = hl ? mask[k] : (~mask[k] & vm);
        if (row[k] >= 0 && left[k] == hl) rowlist[hpre[k][w] + __popcll(hm & lt)] = row[k];
      }
      // the next sub-tile's split-column bins: in flight during the gathers
      uint32_t ngb[kSplitRows];
      col_bins(nj, nrow, ngb);
      // (issued after the column loads: a wait for those would otherwise cover the atomics)
      if (w == 0 && lane == 0 && writer && !X.single) {
        res_l = atomicAdd(&rd->cur[j][0], nl_w0);
        res_r = atomicAdd(&rd->cur[j][1], valid - nl_w0);
      }
      LdsBarrier();  // the row list is complete
      stamp(3);
      if (t.rs < t.rpp) {
        const int wi = t.w0 + t.q;
        const uint32_t* bins32 = static_cast<const uint32_t*>(a.bins);
        const int64_t wpr = a.row_words;
        if constexpr (GPW == kSparseGPW) {
          for (int j0 = t.rs; j0 < nh; j0 += GR * t.rpp) {
            int rr[GR];
#pragma unroll
            for (int k = 0; k < GR; ++k) {
              const int jr = j0 + k * t.rpp;
              rr[k] = jr < nh ? rowlist[jr] : -1;
            }
            float2 v[GR];
#pragma unroll
            for (int k = 0; k < GR; ++k) v[k] = GhAt(a, rr[k] >= 0 ? rr[k] : 0);
            AddSparseRows<GR, UNITS>(a, lds, t, rr, v);
            if (loc_sums && t.q == 0) {
#pragma unroll
              for (int k = 0; k < GR; ++k) {
                if (rr[k] >= 0) {
                  loc_g += __float2ll_rn(v[k].x * t.sg);
                  loc_h += __float2ll_rn(v[k].y * t.sh);
                }
              }
            }
          }
        } else {
          // software-pipelined: the next batch's row words and (g, h) are in flight while this
          // batch's LDS atomics run
          const int step = GR * t.rpp;
          uint32_t wd[GR];
          float2 v[GR];
          auto fetch = [&](int j0, uint32_t* w_, float2* v_) {
#pragma unroll
            for (int k = 0; k < GR; ++k) {
              const int jr = j0 + k * t.rpp;
              const int x = jr < nh ? rowlist[jr] : -1;
#if LGBM_ORACLE_SEQ
              // timing oracle (wrong histograms): the gathers read the parent range's positions
              // instead of the rows, i.e. leaf-ordered copies that cost nothing to maintain
              const int xp = X.pb + t0 + jr;
              v_[k] = GhAt(a, x >= 0 ? xp : 0);
              w_[k] = x >= 0 ? bins32[static_cast<int64_t>(LGBM_ORACLE_SEQ >= 2 ? xp : x) * wpr + wi] : 0u;
#else
              v_[k] = GhAt(a, x >= 0 ? x : 0);
              w_[k] = x >= 0 ? bins32[static_cast<int64_t>(x) * wpr + wi] : 0u;  // word 0: every bin skipped
#endif
            }
          };
          if (t.rs < nh) fetch(t.rs, wd, v);
          for (int j0 = t.rs; j0 < nh; j0 += step) {
            uint32_t wn[GR];
            float2 vn[GR];
            if (j0 + step < nh) fetch(j0 + step, wn, vn);
#pragma unroll
            for (int k = 0; k < GR; ++k) AddRow<GPW, UNITS>(lds, t.goff, t.bits, wd[k], v[k], t.sg, t.sh);
            if (loc_sums && t.q == 0) {
#pragma unroll
              for (int k = 0; k < GR; ++k) {
                if (j0 + k * t.rpp < nh) {
                  loc_g += __float2ll_rn(v[k].x * t.sg);
                  loc_h += __float2ll_rn(v[k].y * t.sh);
                }
              }
            }
#pragma unroll
            for (int k = 0; k < GR; ++k) {
              wd[k] = wn[k];
              v[k] = vn[k];
            }
          }
        }
      }
      stamp(4);
      // ---- the partition (column tile 0): slots from the reservation
      if (w == 0 && lane == 0 && writer) {
        if (X.single) {
          base[0] = base[1] = 0;
          rd->cur[j][0] = nl_w0;
          rd->cur[j][1] = valid - nl_w0;
        } else {
          base[0] = res_l;
          base[1] = res_r;
        }
      }
      LdsBarrier();
      if (writer) {
        const int lbase = X.pb + base[0];
        const int rbase = X.pb + X.pc - 1 - base[1];
#pragma unroll
        for (int k = 0; k < kSplitRows; ++k) {
          if (row[k] >= 0) {
            const int lpos = lpre[k][w] + __popcll(mask[k] & lt);
            const int pos = k * kPartThreads + threadIdx.x;
            if (left[k]) dst[lbase + lpos] = row[k];
            else dst[rbase - (pos - lpos)] = row[k];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kSplitRows; ++k) {
        row[k] = nrow[k];
        gb[k] = ngb[k];
      }
      LdsBarrier();  // row list, wave counts, prefixes and bases are rewritten by the next sub-tile
      stamp(5);
    }
    if (r0 >= r1) {  // (an empty block still stores a zero partial)
      LdsBarrier();
      for (int i = threadIdx.x; i < UNITS * t.nbins; i += kPartThreads) lds[i] = 0ull;
      LdsBarrier();
    }
    unsigned long long* out = a.partials + static_cast<size_t>(kb) * UNITS * a.p.total_bins +
                              static_cast<size_t>(UNITS) * t.lo_bin;
    for (int i = threadIdx.x; i < UNITS * t.nbins; i += kPartThreads) out[i] = lds[i];
    if (loc_sums) {  // (uniform: every lane of every wave takes part in the sums)
      const long long bg = WaveSum(loc_g), bh = WaveSum(loc_h);
      if (lane == 0 && (bg != 0 || bh != 0)) {
        atomicAdd(&rd->loc_acc[j][0], static_cast<unsigned long long>(bg));
        atomicAdd(&rd->loc_acc[j][1], static_cast<unsigned long long>(bh));
      }
      loc_g = loc_h = 0;
    }
    stamp(6);
  }
  if (tr) {
    tacc[9] = wall_clock64() - tstart;
    long long* o = a.ktrace + static_cast<size_t>(rd->round) * kTraceSlots;
    for (int k = 0; k < 10; ++k) o[k] = tacc[k];
    o[10] = nexp;
    o[11] = nblk;
  }
}

// ----------------------------------------------------------------- k_round_part / k_round_hist
// The same round as k_round_split in two streaming kernels (KArgs::round_fused = 0): the
// partition alone (index + split-column byte per row, ballots, one reservation per side and
// sub-tile, no LDS histogram), then the histograms of the histogrammed children, whose rows
// are now one contiguous range of the other index buffer each (RoundHistRows) -- row blocks of
// rpb rows read with kRowsInFlight independent gathers per thread, like the root histogram.
// Block k of expansion j's child is partial blk_off[j] + k (blk_off reserves ceil(parent rows
// / rpb)).
__global__ __launch_bounds__(kPartThreads) void k_round_part(KArgs a) {
  __shared__ SplitExp ex[kMaxRoundExp];
  __shared__ uint32_t cat_bits[kMaxRoundExp][kMaxCatWords];
  __shared__ int wl[kSplitRows][kRPartWaves];
  __shared__ int lpre[kSplitRows][kRPartWaves];
  __shared__ int base[2];
  Round* rd = a.rd;
  const int done = rd->done;
  const int nexp = rd->nexp, nblk = rd->nblk, rpb = rd->rpb;
  if (done || nexp <= 0 || static_cast<int>(blockIdx.x) >= nblk) return;
  if (threadIdx.x < static_cast<unsigned>(nexp)) {
    const ExpPlan& e = rd->e[threadIdx.x];
    SplitExp x;
    x.pb = e.part_begin;
    x.pc = e.part_count;
    x.src = e.src_buf;
    x.dst = e.dst_buf;
    x.blk_off = e.blk_off;
    x.nblk = e.nblk;
    x.hl = e.hist_left;
    x.single = e.nblk == 1 && e.part_count <= kSplitSub;
    x.fbyte = e.feat.gbyte;
    x.fwide = e.feat.gwide;
    x.fcol = e.feat.col_off;
    x.sub_lo = e.feat.sub_lo;
    x.sub_hi = e.feat.sub_hi;
    x.offset = e.feat.offset;
    x.mfb = e.feat.mfb;
    x.r.threshold = e.split.threshold;
    x.r.default_left = e.split.default_left;
    x.r.is_cat = e.split.is_categorical;
    x.r.missing_type = e.feat.missing_type;
    x.r.default_bin = e.feat.default_bin;
    x.r.max_bin = e.feat.num_bin - 1;
    ex[threadIdx.x] = x;
  }
  for (int i = threadIdx.x; i < nexp * kMaxCatWords; i += kPartThreads) {
    const int j = i / kMaxCatWords;
    cat_bits[j][i % kMaxCatWords] = rd->e[j].split.is_categorical ? rd->e[j].split.cat_bits[i % kMaxCatWords] : 0u;
  }
  __syncthreads();
  auto exp_of = [&](int kb) {
    int j = 0;
    while (j + 1 < nexp && kb >= ex[j + 1].blk_off) ++j;
    return j;
  };
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int row[kSplitRows];
  uint32_t gb[kSplitRows];
  auto load_rows = [&](int jn, int t0n, int r1n, int* rr) {
    const int vn = min(kSplitSub, r1n - t0n);
    const int32_t* s = RowBuf(a, ex[jn].src);
    const int pbn = ex[jn].pb;
#pragma unroll
    for (int k = 0; k < kSplitRows; ++k) {
      const int i = k * kPartThreads + threadIdx.x;
      rr[k] = i < vn ? s[pbn + t0n + i] : -1;
    }
  };
  auto col_bins = [&](int jn, const int* rr, uint32_t* g) {
    const ColSrc c = ColSource(a, ex[jn].fbyte, ex[jn].fwide, ex[jn].fcol);
#pragma unroll
    for (int k = 0; k < kSplitRows; ++k) g[k] = ColBinNB(c, rr[k]);
  };
  {
    const int j = exp_of(blockIdx.x);
    const int r0 = (blockIdx.x - ex[j].blk_off) * rpb;
    load_rows(j, r0, min(ex[j].pc, r0 + rpb), row);
    col_bins(j, row, gb);
  }
  for (int kb = blockIdx.x; kb < nblk; kb += gridDim.x) {
    const int j = exp_of(kb);
    const SplitExp& X = ex[j];
    const int r0 = (kb - X.blk_off) * rpb, r1 = min(X.pc, r0 + rpb);
    Feature F;
    F.sub_lo = X.sub_lo;
    F.sub_hi = X.sub_hi;
    F.offset = X.offset;
    F.mfb = X.mfb;
    const SplitRule r = X.r;
    const uint32_t* cb = cat_bits[j];
    int32_t* dst = RowBuf(a, X.dst);
    for (int t0 = r0; t0 < r1; t0 += kSplitSub) {
      const int valid = min(kSplitSub, r1 - t0);
      int nj = j, nt0 = t0 + kSplitSub, nr1 = r1;
      if (nt0 >= r1) {
        const int nkb = kb + gridDim.x;
        if (nkb < nblk) {
          nj = exp_of(nkb);
          nt0 = (nkb - ex[nj].blk_off) * rpb;
          nr1 = min(ex[nj].pc, nt0 + rpb);
        } else {
          nt0 = nr1 = 0;
        }
      }
      int nrow[kSplitRows];
      load_rows(nj, nt0, nr1, nrow);
      bool left[kSplitRows];
      unsigned long long mask[kSplitRows];
#pragma unroll
      for (int k = 0; k < kSplitRows; ++k) {
        left[k] = row[k] >= 0 && GoesLeft(r, cb, FeatureBinOf(F, gb[k]));
        mask[k] = __ballot(left[k]);
      }
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kSplitRows; ++k) wl[k][w] = __popcll(mask[k]);
      }
      __syncthreads();
      if (w == 0) {
        const int k = lane / kRPartWaves, jj = lane % kRPartWaves;
        const int c = wl[k][jj];
        const int ci = WavePrefixIncl(c);
        lpre[k][jj] = ci - c;
        const int nl = __shfl(ci, kWave - 1, kWave);
        if (lane == 0) {
          if (X.single) {
            base[0] = base[1] = 0;
            rd->cur[j][0] = nl;
            rd->cur[j][1] = valid - nl;
          } else {
            base[0] = atomicAdd(&rd->cur[j][0], nl);
            base[1] = atomicAdd(&rd->cur[j][1], valid - nl);
          }
        }
      }
      __syncthreads();
      const int lbase = X.pb + base[0];
      const int rbase = X.pb + X.pc - 1 - base[1];
#pragma unroll
      for (int k = 0; k < kSplitRows; ++k) {
        if (row[k] >= 0) {
          const int lpos = lpre[k][w] + __popcll(mask[k] & lt);
          const int pos = k * kPartThreads + threadIdx.x;
          if (left[k]) dst[lbase + lpos] = row[k];
          else dst[rbase - (pos - lpos)] = row[k];
        }
      }
#pragma unroll
      for (int k = 0; k < kSplitRows; ++k) row[k] = nrow[k];
      col_bins(nj, row, gb);
      __syncthreads();  // wave counts and bases are rewritten by the next sub-tile
    }
  }
}

template <int GPW, int UNITS>
__global__ __launch_bounds__(kHistThreads) void k_round_hist(KArgs a) {
  extern __shared__ unsigned long long lds[];
  __shared__ int s_off[kMaxRoundExp + 1], s_beg[kMaxRoundExp], s_rows[kMaxRoundExp], s_buf[kMaxRoundExp],
      s_cap[kMaxRoundExp];
  const Round* rd = a.rd;
  if (rd->done) return;
  const int nexp = rd->nexp, rpb = rd->rpb;
  if (nexp <= 0) return;
  TileCtx t;
  InitTile<GPW>(a, &t);
  if (threadIdx.x == 0) {
    int off = 0;
    for (int j = 0; j < nexp; ++j) {
      int b;
      const int h = RoundHistRows(rd, j, &b);
      s_off[j] = off;
      s_beg[j] = b;
      s_rows[j] = h;
      s_buf[j] = rd->e[j].dst_buf;
      s_cap[j] = rd->e[j].blk_off;
      off += (h + rpb - 1) / rpb;
    }
    s_off[nexp] = off;
  }
  __syncthreads();
  const int total = s_off[nexp];
  const size_t pstride = static_cast<size_t>(UNITS) * a.p.total_bins;
  for (int kb = blockIdx.x; kb < total; kb += gridDim.x) {
    int j = 0;
    while (j + 1 < nexp && kb >= s_off[j + 1]) ++j;
    const int k = kb - s_off[j];
    const int r0 = s_beg[j] + k * rpb, r1 = min(s_beg[j] + s_rows[j], r0 + rpb);
    HistBlock<false, GPW, UNITS>(a, lds, RowBuf(a, s_buf[j]), r0, r1, t,
                                 a.partials + static_cast<size_t>(s_cap[j] + k) * pstride + static_cast<size_t>(UNITS) * t.lo_bin);
  }
}

// --------------------------------------------------------------------------- k_round_reduce
// grid (bins / 256, kReduceRows, round_k): the partials of expansion blockIdx.z with more than
// kDirectChunk row blocks summed into its reduce buffer (pre-zeroed by the previous round's
// split scans when the chunks combine with atomics)
template <int UNITS>
__global__ __launch_bounds__(256) void k_round_reduce(KArgs a) {
  const Round* rd = a.rd;
  if (rd->done) return;
  const int j = blockIdx.z;
  if (j >= rd->nexp) return;
  const int nblk = RoundHistBlocks(a, rd, j);
  // data-parallel: every expansion reduced, into the owner-major send buffer (voting keeps
  // rank-local histograms: the single-process layout)
  const bool dp = a.p.data_parallel != 0 && !a.round_vote;
  if (!dp && nblk <= kDirectChunk) return;  // summed by the split scan
  if (static_cast<int>(blockIdx.y) * kReduceChunk >= nblk) return;
  const int bin = blockIdx.x * blockDim.x + threadIdx.x;
  const int nb = a.p.total_bins;
  if (bin >= nb) return;
  const size_t pstride = static_cast<size_t>(UNITS) * nb;
  const unsigned long long* part = a.partials + static_cast<size_t>(rd->e[j].blk_off) * pstride;
  long long g = 0, h = 0;
  for (int k0 = blockIdx.y * kReduceChunk; k0 < nblk; k0 += gridDim.y * kReduceChunk) {
    const unsigned long long* p = part + k0 * pstride + static_cast<size_t>(UNITS) * bin;
    const int kn = min(kReduceChunk, nblk - k0);
    unsigned long long v0[kReduceChunk], v1[kReduceChunk];
#pragma unroll
    for (int k = 0; k < kReduceChunk; ++k) {
      v0[k] = k < kn ? p[k * pstride] : 0ull;
      v1[k] = (UNITS == 2 && k < kn) ? p[k * pstride + 1] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < kReduceChunk; ++k) {
      long long pg, ph;
      UnpackPartial(v0[k], v1[k], UNITS, &pg, &ph);
      g += pg;
      h += ph;
    }
  }
  long long* out = RoundScratch(a, rd->round, j);
  int pos = bin;
  if (dp) {
    const int rp = a.rs_pos[bin], owner = rp / a.rs_block;
    if (rp < 0) return;  // (a group no rank scans this tree)
    out = a.round_send;
    pos = (owner * a.round_k + j) * a.rs_block + (rp - owner * a.rs_block);
  }
  if (nblk <= kReduceChunk) {
    out[2 * pos] = g;
    out[2 * pos + 1] = h;
  } else {
    atomicAdd(reinterpret_cast<unsigned long long*>(&out[2 * pos]), static_cast<unsigned long long>(g));
    atomicAdd(reinterpret_cast<unsigned long long*>(&out[2 * pos + 1]), static_cast<unsigned long long>(h));
  }
}

namespace {

template <int GR, bool VOTE = false>
void LaunchRoundSplit(const KArgs& a, hipStream_t s) {
  const dim3 grid(a.round_grid, a.hist_tiles);
  const size_t lds = sizeof(unsigned long long) * a.hist_units * static_cast<size_t>(a.tile_bins) + sizeof(int) * kSplitSub;
  DispatchBinLayout(a, [&](auto gpw, auto units) {
    hipLaunchKernelGGL((k_round_split<decltype(gpw)::value, decltype(units)::value, GR, VOTE>), grid, dim3(kPartThreads), lds, s, a);
  });
}

}  // namespace

void PrepareRoundSplitKernels(int max_lds) {
  ForEachBinLayout([max_lds](auto gpw, auto units) {
    constexpr int G = decltype(gpw)::value, U = decltype(units)::value;
    AllowLds(k_round_hist<G, U>, max_lds);
    AllowLds(k_round_split<G, U, 2>, max_lds);
    AllowLds(k_round_split<G, U, 4>, max_lds);
    AllowLds(k_round_split<G, U, 8>, max_lds);
    AllowLds(k_round_split<G, U, 2, true>, max_lds);
  });
}

void RoundSplitReduce(const KArgs& a, hipStream_t s) {
  if (a.round_fused) {
    const int gr = a.round_gr > 0 ? a.round_gr
                   : ((a.sp_ptr != nullptr || a.tile_words <= kRGatherNarrowMaxWords) ? kRGatherNarrow : kRGatherWide);
    if (a.round_vote) LaunchRoundSplit<2, true>(a, s);  // (voting: the local sums' variant)
    else if (gr >= 8) LaunchRoundSplit<8>(a, s);
    else if (gr >= 4) LaunchRoundSplit<4>(a, s);
    else LaunchRoundSplit<2>(a, s);
  } else {
    hipLaunchKernelGGL(k_round_part, dim3(a.round_grid), dim3(kPartThreads), 0, s, a);
    const dim3 grid(a.root_grid, a.hist_tiles);
    const size_t lds = sizeof(unsigned long long) * a.hist_units * static_cast<size_t>(a.tile_bins);
    DispatchBinLayout(a, [&](auto gpw, auto units) {
      hipLaunchKernelGGL((k_round_hist<decltype(gpw)::value, decltype(units)::value>), grid, dim3(kHistThreads), lds, s, a);
    });
  }
  const dim3 rgrid((a.p.total_bins + 255) / 256,
                   std::min(4, (a.hist_max_blocks + kReduceChunk - 1) / kReduceChunk), a.round_k);
  if (a.hist_units == 1) hipLaunchKernelGGL((k_round_reduce<1>), rgrid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_round_reduce<2>), rgrid, dim3(256), 0, s, a);
}

}  // namespace dev
}  // namespace lgbm_amd
