// partition_masked.hpp — the partition pass of a routed insert whose row set lives on the device
// (rpt_bf_insert_bits_ws, rpt_bf_insert_sel_ws, rpt_bf_transfer_insert_ws): the masked twin of partition_kernel
// (partitioned.hpp). The partitioned insert's geometry depends on the row count the host knows (n / max_rows) only:
// tiles of kTileRows * TM rows, and per tile and slice a run of records with its true length. A row that is not
// selected emits no record, so runs_transpose_kernel and slice_insert_kernel run as they are over shorter runs.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// Output: partition_kernel's, without the row map (inserts need none): recs in the padded tile layout
// (tile_cap_for), runs_tm[tile][slice] = padded start << 16 | true count. Dynamic LDS: partition_lds_bytes.
//   SEL = false  row i < n of the column (row i, or a.row_sel[i]) is selected iff bit i of `bits` is set
//                (rpt_bf_probe_bits's layout; bits at positions >= n are ignored). A 512-row segment without a set
//                bit loads no key (the ballot on load_alive_word, as insert_bits_kernel).
//   SEL = true   the rows are a.row_sel[0 .. min(*count_dev, n)) (a selection vector: the general mapping). The
//                workgroup reads the count once (a uniform load; the kernel that wrote it is earlier on the stream);
//                the grid comes from n = max_rows, and every read of the selection is bounded by the clamped count.
// A tile without a selected row (all its bit words zero, or wholly past the count) loads no key and stores no
// record, but still writes its runs_tm row, as zeros: the workspace holds anything on entry, and the transposed run
// table of every tile is read by the slice kernel.
// The key min/max covers the selected, valid (non-NULL), in-range rows (a selected NULL row inserts NULL_HASH); HASH
// columns fold nothing. It is published once per workgroup, as partition_kernel does.
// Records are always parked in LDS between the passes (partition_kernel's NOPARK tuning and its non-temporal stores
// are not carried over: the pass reads bit words and skips rows, its balance differs and was not measured).
template <int K, bool DENSE, bool SEL, int TM, int SP = 0>
__global__ __launch_bounds__(kTileThreads, TM == 1 ? RPT_PARTITION_MIN_WAVES : 4) void partition_masked_kernel(
    KeyArgs a, uint64_t n, uint32_t slice_mask, uint32_t* __restrict__ recs, uint32_t* __restrict__ runs_tm,
    int64_t* __restrict__ stats, const uint64_t* __restrict__ bits, const uint64_t* __restrict__ count_dev) {
  static_assert(!(SEL && DENSE), "a selection vector is the general mapping");
  static_assert(SP == 0 || TM == 1, "the few-slice counters exist for 16 Ki-row tiles");
  constexpr bool PAD = TM == 1;
  constexpr bool MM = KeyTraits<K>::kValues;
  constexpr uint64_t kTR = kTileRows * TM;  // rows of this tile
  constexpr int kRPT = static_cast<int>(kTR / kTileThreads), kSPW = kRPT / 8;
  static_assert(kRPT <= 32, "a lane's selected-row flags are one 32-bit word");
  extern __shared__ uint32_t s_dyn[];
  const uint32_t n_slices = slice_mask + 1;
  const uint64_t tile_cap = tile_cap_for(n_slices, TM);
  uint32_t* s_rec = s_dyn;
  uint32_t* s_cnt = s_dyn + (PAD ? tile_cap : kTR);  // selected rows per slice in this tile
  uint32_t* s_cur = s_cnt + n_slices;        // run start (padded if PAD), then scatter cursor (start + count)
  uint32_t* s_delta = s_cur + n_slices;      // !PAD: padded start - unpadded start
  uint16_t* s_gslice = reinterpret_cast<uint16_t*>(s_delta + n_slices);  // slice of each kRunPad group
  __shared__ int64_t s_mm[kTileThreads / 64][2];  // each wave's key min / max
  __shared__ uint32_t s_total;                    // selected rows of the tile
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t tile = blockIdx.x;
  const uint64_t tile_base = tile * kTR;
  uint32_t* const my_runs = runs_tm + tile * n_slices;
  uint64_t n_rows = n;
  if constexpr (SEL) {
    const uint64_t stored = *count_dev;
    n_rows = stored < n ? stored : n;
  }
  if (tile_base >= n_rows) {  // uniform: a tile wholly past the count
    for (uint32_t i = threadIdx.x; i < n_slices; i += kTileThreads) my_runs[i] = 0u;
    return;
  }
  for (uint32_t i = threadIdx.x; i < n_slices; i += kTileThreads) s_cnt[i] = 0;
  __syncthreads();
  // pass 1: hash the selected rows, stage their records in LDS, count them per slice; the 16-bit slice ids
  // and the selected-row flags stay in registers
  // (16 bits each; 2 bits with the few-slice counters, whose registers the int64 kernel needs: 64 VGPRs, no scratch)
  constexpr int kSlBits = SP > 0 ? 2 : 16, kSlPerWord = 32 / kSlBits;
  static_assert(kMaxSliceCount <= 65536 && SP <= (1 << 2), "slice ids are packed as 16 (SP: 2) bits");
  uint32_t sl2[(kRPT + kSlPerWord - 1) / kSlPerWord] = {};
  uint32_t okbits = 0;                                 // bit sg * 8 + j: this lane's row j of segment sg is inserted
  [[maybe_unused]] uint32_t lc[SP > 0 ? SP : 1] = {};  // SP: this lane's rows per slice
  int64_t wmn = kMinInit, wmx = kMaxInit;  // wave-uniform: the key min/max stays out of VGPRs
#pragma unroll
  for (int sg = 0; sg < kSPW; sg++) {
    const uint32_t seg_local = wave * (kSPW * kSegRows) + sg * kSegRows;
    const uint64_t base = tile_base + seg_local;
    if (base >= n_rows) continue;  // uniform: past the last row (no bit word exists for such a segment)
    uint64_t hh[8];
    bool oo[8];
    int64_t mm[2] = {kMinInit, kMaxInit};
    if constexpr (SEL) {
      load_hashes<K, false, MM>(a, base, n_rows, lane, hh, oo, mm);
    } else {
      const uint64_t mine = load_alive_word(bits, base / kSegRows, lane);
      if (ballot64(mine != 0) == 0) continue;  // uniform: a dead segment
      bool alive[8];
      alive_flags<K, DENSE>(mine, lane, alive);
      if constexpr (DENSE) load_dense_alive<K>(a, base, n_rows, lane, alive, hh, oo, mm);
      else load_general_alive<K>(a, base, n_rows, lane, alive, hh, oo, mm);
    }
    if constexpr (MM) {
      wave_minmax(mm[0], mm[1]);
      wmn = min(wmn, mm[0]);
      wmx = max(wmx, mm[1]);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t sl = static_cast<uint32_t>(hh[j] >> (kLogNumMasks + 6 + kSliceLog)) & slice_mask;
      s_rec[seg_local + park_slot(j, lane)] = slice_record(hh[j]);
      sl2[(sg * 8 + j) / kSlPerWord] |= sl << (kSlBits * ((sg * 8 + j) % kSlPerWord));
      okbits |= (oo[j] ? 1u : 0u) << (sg * 8 + j);
      if constexpr (SP > 0) {
#pragma unroll
        for (int q = 0; q < SP; q++) lc[q] += (oo[j] && sl == static_cast<uint32_t>(q)) ? 1u : 0u;
      } else {
        if (oo[j]) atomicAdd(&s_cnt[sl], 1u);
      }
    }
  }
  if constexpr (MM) {  // published once per workgroup at the end
    if (lane == 0) {
      s_mm[wave][0] = wmn;
      s_mm[wave][1] = wmx;
    }
  }
  [[maybe_unused]] uint32_t lofs[SP > 0 ? SP : 1], wtot[SP > 0 ? SP : 1];
  if constexpr (SP > 0) {  // one atomic per wave and slice
#pragma unroll
    for (int q = 0; q < SP; q++) {
      const uint32_t inc = wave_inclusive_sum(lc[q]);
      lofs[q] = inc - lc[q];
      wtot[q] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(inc), 63));
      if (lane == 0 && wtot[q] != 0) atomicAdd(&s_cnt[q], wtot[q]);
    }
  }
  __syncthreads();
  if (wave == 0) {  // exclusive scans of the slice counts, unpadded and padded to kRunPad: kMaxSliceCount/64 per lane
    constexpr int kPer = kMaxSliceCount / 64;
    uint32_t c[kPer], t = 0, tp = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++) {
      const uint32_t idx = lane * kPer + i;
      c[i] = idx < n_slices ? s_cnt[idx] : 0u;
      t += c[i];
      tp += pad_run(c[i]);
    }
    const uint32_t inc = wave_inclusive_sum(t);
    uint32_t off = inc - t, poff = wave_inclusive_sum(tp) - tp;
    if (lane == 63) s_total = inc;
#pragma unroll
    for (int i = 0; i < kPer; i++) {
      const uint32_t idx = lane * kPer + i;
      if (idx < n_slices) {
        if constexpr (PAD) {
          s_cur[idx] = poff;
        } else {
          s_cur[idx] = off;
          s_delta[idx] = poff - off;
        }
      }
      off += c[i];
      poff += pad_run(c[i]);
    }
  }
  // pass 2: pull this thread's records back out of the row-ordered staging (a skipped segment's slots hold
  // whatever LDS held: never scattered) ...
  uint32_t rec[kRPT];
#pragma unroll
  for (int sg = 0; sg < kSPW; sg++) {
    const uint32_t seg_local = wave * (kSPW * kSegRows) + sg * kSegRows;
#pragma unroll
    for (int j = 0; j < 8; j++) rec[sg * 8 + j] = s_rec[seg_local + park_slot(j, lane)];
  }
  __syncthreads();
  if (s_total == 0) {  // uniform: no selected row in this tile: no record, an all-zero run row
    for (uint32_t i = threadIdx.x; i < n_slices; i += kTileThreads) my_runs[i] = 0u;
    return;
  }
  [[maybe_unused]] uint32_t cur[SP > 0 ? SP : 1];
  if constexpr (SP > 0) {  // this lane's first position per slice: the wave's base + earlier lanes' rows
#pragma unroll
    for (int q = 0; q < SP; q++) {
      uint32_t wb = 0;
      if (lane == 0 && wtot[q] != 0) wb = atomicAdd(&s_cur[q], wtot[q]);
      cur[q] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wb))) + lofs[q];
    }
  }
  // ... and scatter the selected ones to their slice-sorted LDS positions
#pragma unroll
  for (int jj = 0; jj < kRPT; jj++) {
    const uint32_t sl = (sl2[jj / kSlPerWord] >> (kSlBits * (jj % kSlPerWord))) & ((1u << kSlBits) - 1);
    if ((okbits >> jj) & 1u) {
      uint32_t q;
      if constexpr (SP > 0) {
        q = cur[0];
#pragma unroll
        for (int t = 1; t < SP; t++) q = sl == static_cast<uint32_t>(t) ? cur[t] : q;
#pragma unroll
        for (int t = 0; t < SP; t++) cur[t] += sl == static_cast<uint32_t>(t) ? 1u : 0u;
      } else {
        q = atomicAdd(&s_cur[sl], 1u);
      }
      s_rec[q] = rec[jj];
    }
  }
  __syncthreads();
  // records of the tile in the padded layout, 16 B per thread and step (pad slots hold stale values: never
  // read back, the slice insert walks true counts); the scatter left s_cur[i] = start_i + count_i
  u32x4* dst = reinterpret_cast<u32x4*>(recs + tile * tile_cap);
  if constexpr (PAD) {
    const uint32_t used = s_cur[slice_mask] - s_cnt[slice_mask] + pad_run(s_cnt[slice_mask]);
    const u32x4* src = reinterpret_cast<const u32x4*>(s_rec);
    for (uint32_t i = threadIdx.x; i < used / 4; i += kTileThreads) dst[i] = src[i];
    for (uint32_t i = threadIdx.x; i < n_slices; i += kTileThreads)
      my_runs[i] = ((s_cur[i] - s_cnt[i]) << 16) | s_cnt[i];  // padded start | true count
  } else {
    // each slice owns the kRunPad-record groups of its padded run
    for (uint32_t i = threadIdx.x; i < n_slices; i += kTileThreads) {
      const uint32_t c = s_cnt[i], pst = s_cur[i] - c + s_delta[i];
      for (uint32_t g = pst / kRunPad; g < (pst + pad_run(c)) / kRunPad; g++) s_gslice[g] = static_cast<uint16_t>(i);
    }
    __syncthreads();
    const uint32_t used = s_cur[slice_mask] + s_delta[slice_mask] - s_cnt[slice_mask] + pad_run(s_cnt[slice_mask]);
    for (uint32_t i = threadIdx.x; i < used / 4; i += kTileThreads) {
      const uint32_t q = 4 * i - s_delta[s_gslice[(4 * i) / kRunPad]];  // unpadded position of the piece
      u32x4 v;
#pragma unroll
      for (int e = 0; e < 4; e++) v[e] = s_rec[min(q + e, static_cast<uint32_t>(kTR) - 1)];
      dst[i] = v;
    }
    for (uint32_t i = threadIdx.x; i < n_slices; i += kTileThreads)
      my_runs[i] = ((s_cur[i] - s_cnt[i] + s_delta[i]) << 16) | s_cnt[i];  // padded start | true count
  }
  if constexpr (MM) {
    // one no-return atomic pair per workgroup (s_mm was written before pass 1's barrier)
    if (threadIdx.x == 0) {
      int64_t mn = kMinInit, mx = kMaxInit;
      for (int w = 0; w < kTileThreads / 64; w++) {
        mn = min(mn, s_mm[w][0]);
        mx = max(mx, s_mm[w][1]);
      }
      if (mn != kMinInit) (void)__hip_atomic_fetch_min(stats, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (mx != kMaxInit) (void)__hip_atomic_fetch_max(stats + 1, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace rpt
