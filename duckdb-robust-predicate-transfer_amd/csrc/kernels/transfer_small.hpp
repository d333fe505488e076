// transfer_small.hpp — the one-launch forward step and the one-launch sink for one DuckDB-sized vector
// (rpt_bf_transfer, rpt_bf_transfer_range, rpt_bf_insert_multi): the row-list twin of probe_chain_range_small_kernel's
// transfer (probe_sel_range.hpp), whose row count comes from the host, and the sink of one vector into several
// filters with no probe before it. One workgroup, one launch, no workspace: scan → USE_BF → CREATE_BF, or scan →
// CREATE_BF into one filter per build column.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// PROBED: probe_chain_range_small_kernel<false, true>'s schedule over positions 0 .. n of the column, or of the
// nullable row_sel (every column's row_sel): the (filter, segment) items over the waves (RANGED: chain_probe_range for
// a filter flagged in r.mask, chain_probe for any other; !RANGED: r.mask and r.stats are not looked at), the AND, the
// per-segment counts, the tail, then the survivors into the d.n outgoing filters.
// !PROBED (rpt_bf_insert_multi): no filter is probed and neither out_sel nor out_count is written; every position
// below n is a survivor and only the inserts run.
// One workgroup of kSmallThreads; 0 < n <= kSmallRows. No row_sel entry at or past n is read: every row_sel read of the
// probes and of the inserts is bounded by n, the AND words hold no bit at or past n, and the tail reads row_sel only
// where a bit is set. The inserts read row_sel after the tail has begun to store out_sel: the host refuses ranges that
// overlap.
template <bool RANGED, bool PROBED>
__global__ __launch_bounds__(kSmallThreads) void transfer_small_kernel(RangeChainArgs r, DstArgs d,
                                                                       const uint32_t* __restrict__ row_sel, uint64_t n,
                                                                       uint32_t* __restrict__ out_sel,
                                                                       uint64_t* __restrict__ out_count) {
  static_assert(PROBED || !RANGED, "a range belongs to a probed filter");
  constexpr uint32_t kSegs = kSmallRows / kSegRows;
  constexpr uint32_t kWaves = kSmallThreads / 64;
  __shared__ uint64_t s_masks[kNumMasks];
  __shared__ uint64_t s_words[kSegs * kWordsPerSeg];
  fill_mask_table(s_masks);
  const uint32_t n_segs = static_cast<uint32_t>((n + kSegRows - 1) / kSegRows);
  if constexpr (PROBED) {
    __shared__ uint64_t s_pass[kMaxChain][kSegs * kWordsPerSeg];  // each filter's position-ordered pass words
    __shared__ uint32_t s_cnt[kSegs];
    const ChainArgs& c = r.c;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t it = wave; it < c.k * n_segs; it += kWaves) {
      const uint32_t f = it / n_segs, seg = it - f * n_segs;  // uniform
      const uint64_t base = static_cast<uint64_t>(seg) * kSegRows;
      bool flagged = false;  // uniform; the host refuses a flagged HASH column
      if constexpr (RANGED) flagged = (r.mask >> f) & 1u;
      bool pass[8];
      if (c.key_type[f] == kKeyI64) {
        if (flagged) chain_probe_range<kKeyI64>(c.a[f], c.words[f], c.block_mask[f], r.stats[f], s_masks, base, n, lane, pass);
        else chain_probe<kKeyI64>(c.a[f], c.words[f], c.block_mask[f], s_masks, base, n, lane, pass);
      } else if (c.key_type[f] == kKeyI32) {
        if (flagged) chain_probe_range<kKeyI32>(c.a[f], c.words[f], c.block_mask[f], r.stats[f], s_masks, base, n, lane, pass);
        else chain_probe<kKeyI32>(c.a[f], c.words[f], c.block_mask[f], s_masks, base, n, lane, pass);
      } else {
        chain_probe<kKeyHash>(c.a[f], c.words[f], c.block_mask[f], s_masks, base, n, lane, pass);
      }
      store_segment_bits<kKeyI64, false>(pass, lane, seg, s_pass[f], nullptr);
    }
    __syncthreads();
    // the AND over the filters, word by word; then each segment's survivor count
    for (uint32_t w = threadIdx.x; w < n_segs * kWordsPerSeg; w += kSmallThreads) {
      uint64_t x = s_pass[0][w];
      for (uint32_t f = 1; f < c.k; f++) x &= s_pass[f][w];
      s_words[w] = x;
    }
    __syncthreads();
    for (uint32_t seg = wave; seg < n_segs; seg += kWaves) {
      const uint32_t pc = lane < kWordsPerSeg ? static_cast<uint32_t>(__popcll(s_words[seg * kWordsPerSeg + lane])) : 0u;
      const uint32_t t = wave_sum(pc);
      if (lane == 0) s_cnt[seg] = t;
    }
    __syncthreads();
    // the tail and the inserts only read s_words: the tail first, so its out_sel stores are in flight while the
    // atomics issue
    small_sel_tail(s_words, s_cnt, n_segs, row_sel, out_sel, out_count);
  } else {
    // every position below n survives: word w holds positions 64 w .. 64 w + 63
    for (uint32_t w = threadIdx.x; w < n_segs * kWordsPerSeg; w += kSmallThreads) {
      const uint64_t first = static_cast<uint64_t>(w) * 64;
      s_words[w] = first + 64 <= n ? ~0ULL : first < n ? (1ULL << (n - first)) - 1 : 0ULL;
    }
    __syncthreads();
  }
  for (uint32_t j = 0; j < d.n; j++) {  // uniform
    if (d.key_type[j] == kKeyI64)
      small_insert_dst<kKeyI64>(d.words[j], d.block_mask[j], d.a[j], d.stats[j], s_masks, s_words, n_segs, n);
    else if (d.key_type[j] == kKeyI32)
      small_insert_dst<kKeyI32>(d.words[j], d.block_mask[j], d.a[j], d.stats[j], s_masks, s_words, n_segs, n);
    else
      small_insert_dst<kKeyHash>(d.words[j], d.block_mask[j], d.a[j], d.stats[j], s_masks, s_words, n_segs, n);
  }
}

}  // namespace rpt
