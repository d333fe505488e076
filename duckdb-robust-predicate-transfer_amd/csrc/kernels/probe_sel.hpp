// probe_sel.hpp — the first stage of a device-counted chain (rpt_bf_probe_chain_sel_ws, rpt_bf_transfer_sel_ws):
// probe_bits_body's general loop (probe_direct.hpp) over a selection vector whose length lives in device memory, so
// the survivors of an earlier probe are probed again without their count reaching the host.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// Where probe_bits_sel_kernel reads the filter: gathered from global memory / L2, the whole filter staged in LDS
// (<= 128 KiB), or the first 128 KiB staged and the rest gathered (the hybrid of probe_direct.hpp).
constexpr int kSelGather = 0, kSelLds = 1, kSelHybrid = 2;
template <int MODE>
constexpr int sel_probe_threads() { return MODE == kSelGather ? kBlockThreads : kLdsProbeThreads; }

// The rows are a.row_sel[0 .. min(*count_dev, max_rows)) of the column (a selection vector: always the general
// mapping, so there is no DENSE argument). Every workgroup reads the count once (a uniform load; the kernel that wrote
// it is earlier on the stream) and clamps it to max_rows, the capacity of the selection; the grid and n_segs =
// ceil(max_rows / 512) come from max_rows on the host, as in partition_masked_kernel<SEL = true>.
// * A 512-row segment wholly past the clamped count stores its 8 zero words and a zero count and loads nothing: the
//   later stages and the tail read every segment's words and count, and the workspace holds anything on entry. A
//   workgroup all of whose segments lie past the count does not stage the filter either.
// * Any other segment is probe_bits_body's general loop: load_hashes<K, false> bounded by the clamped count (no
//   selection entry at or past it is read), probe8, store_segment_bits.
// Each lane makes 8 dependent sel -> (key_sel ->) key gathers per segment; nothing is prefetched.
template <int K, int MODE>
__global__ __launch_bounds__(sel_probe_threads<MODE>()) void probe_bits_sel_kernel(
    const uint64_t* __restrict__ words, uint64_t block_mask, KeyArgs a, const uint64_t* __restrict__ count_dev,
    uint64_t max_rows, uint64_t n_segs, uint64_t* __restrict__ out_bits, uint32_t* __restrict__ seg_counts) {
  constexpr bool FILTER_IN_LDS = MODE != kSelGather, HYBRID = MODE == kSelHybrid;
  constexpr uint32_t kWaves = sel_probe_threads<MODE>() / 64;
  __shared__ uint64_t s_masks[kNumMasks];
  extern __shared__ uint64_t s_filter[];
  const uint64_t stored = *count_dev;
  const uint64_t n = stored < max_rows ? stored : max_rows;
  fill_mask_table(s_masks);
  // the workgroup's first segment is its lowest: past the count, no segment of it probes anything (uniform)
  const bool live = static_cast<uint64_t>(blockIdx.x) * kWaves * kSegRows < n;
  if constexpr (FILTER_IN_LDS) {
    if (live) {
      const uint64_t staged = HYBRID ? kHybridWords - 1 : block_mask;
      for (uint64_t i = threadIdx.x; i <= staged; i += blockDim.x) s_filter[i] = words[i];
    }
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWaves +
                 static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
  for (; seg < n_segs; seg += total_waves) {
    if (seg * kSegRows >= n) {  // uniform: wholly past the count
      if (lane < kWordsPerSeg) out_bits[seg * kWordsPerSeg + lane] = 0ULL;
      if (lane == 0) seg_counts[seg] = 0u;
      continue;
    }
    uint64_t h[8];
    bool ok[8], pass[8];
    load_hashes<K, false>(a, seg * kSegRows, n, lane, h, ok);
    probe8<FILTER_IN_LDS, HYBRID>(words, s_filter, s_masks, block_mask, h, ok, pass);
    store_segment_bits<K, false>(pass, lane, seg, out_bits, seg_counts);
  }
}

}  // namespace rpt
