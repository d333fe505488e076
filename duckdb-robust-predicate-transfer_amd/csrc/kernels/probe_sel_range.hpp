// probe_sel_range.hpp — a filter's min/max range (range.hpp) in the device-counted probes and in the one-launch
// chains: stage 0 of a ranged device-counted workspace call (rpt_bf_probe_chain_sel_range_ws and its transfers), and
// the one-launch chain / transfer whose flagged filters test range and Bloom bits from one key load
// (rpt_bf_probe_chain_range, rpt_bf_probe_chain_sel_range, rpt_bf_transfer_sel_range).
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// range_bits_kernel<K, false, false> over a.row_sel[0 .. min(*count_dev, max_rows)), in the shape of
// probe_bits_sel_kernel (probe_sel.hpp): every workgroup reads the count once (a uniform load) and clamps it to
// max_rows; the grid and n_segs = ceil(max_rows / 512) come from max_rows on the host.
// * A 512-row segment wholly past the clamped count stores its 8 zero words and a zero count and loads nothing.
// * Any other segment loads its key values in the general mapping bounded by the clamped count (no selection entry at
//   or past it is read), applies range_bits_kernel's test against stats = {min, max} (read when the kernel runs) and
//   stores the segment's words and count.
template <int K>
__global__ __launch_bounds__(kBlockThreads) void range_bits_sel_kernel(const int64_t* __restrict__ stats, KeyArgs a,
                                                                       const uint64_t* __restrict__ count_dev,
                                                                       uint64_t max_rows, uint64_t n_segs,
                                                                       uint64_t* __restrict__ out_bits,
                                                                       uint32_t* __restrict__ seg_counts) {
  const uint64_t stored = *count_dev;
  const uint64_t n = stored < max_rows ? stored : max_rows;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock +
                 static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
  const int64_t mn = stats[0], mx = stats[1];
  const bool no_value = mn > mx;
  for (; seg < n_segs; seg += total_waves) {
    if (seg * kSegRows >= n) {  // uniform: wholly past the count
      if (lane < kWordsPerSeg) out_bits[seg * kWordsPerSeg + lane] = 0ULL;
      if (lane == 0) seg_counts[seg] = 0u;
      continue;
    }
    bool want[8];
#pragma unroll
    for (int j = 0; j < 8; j++) want[j] = true;
    int64_t v[8];
    bool in[8], valid[8], pass[8];
    load_values<K, false>(a, seg * kSegRows, n, lane, want, v, in, valid);
#pragma unroll
    for (int j = 0; j < 8; j++) pass[j] = in[j] && (no_value || (valid[j] && v[j] >= mn && v[j] <= mx));
    store_segment_bits<K, false>(pass, lane, seg, out_bits, seg_counts);
  }
}

// The one-launch chain's filters with, per filter, where its {min, max} live, and the mask of the flagged ones.
struct RangeChainArgs {
  ChainArgs c;
  const int64_t* stats[kMaxChain];
  uint32_t mask;
};

// chain_probe (probe_direct.hpp) for a flagged filter: one key load feeds both halves of the dynamic filter. The 8
// rows' loads are issued level by level, back to back, as chain_hashes issues them (positions past n read position
// `base` and are discarded); the key values and validity are kept, the filter's {min, max} is one uniform load, and a
// row outside the range gathers no filter word. The range test is range_bits_kernel's: with a value (min <= max) a row
// passes iff its key is not NULL and min <= key <= max (I32 sign-extended); without one every row passes, NULL rows
// included.
template <int K>
__device__ __forceinline__ void chain_probe_range(const KeyArgs& a, const uint64_t* __restrict__ words,
                                                  uint64_t block_mask, const int64_t* __restrict__ stats,
                                                  const uint64_t* s_masks, uint64_t base, uint64_t n, uint32_t lane,
                                                  bool (&pass)[8]) {
  using Tr = KeyTraits<K>;
  using T = typename Tr::T;
  static_assert(Tr::kValues, "a range test needs key values: I64 or I32 columns");
  const uint32_t rem = static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows);  // base < n
  const int64_t mn = stats[0], mx = stats[1];
  const bool no_value = mn > mx;
  uint64_t idx[8];
  bool ok[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const uint32_t off = static_cast<uint32_t>(c * 64) + lane;
    ok[c] = off < rem;
    idx[c] = base + (ok[c] ? off : 0u);  // positions past n read position `base` (in range) and are discarded
  }
  if (a.row_sel != nullptr) {
#pragma unroll
    for (int c = 0; c < 8; c++) idx[c] = a.row_sel[idx[c]];
  }
  if (a.key_sel != nullptr) {
#pragma unroll
    for (int c = 0; c < 8; c++) idx[c] = a.key_sel[idx[c]];
  }
  const T* keys = static_cast<const T*>(a.keys);
  T kv[8];
#pragma unroll
  for (int c = 0; c < 8; c++) kv[c] = keys[idx[c]];
  uint64_t vw[8];
#pragma unroll
  for (int c = 0; c < 8; c++) vw[c] = ~0ULL;
  if (a.validity != nullptr) {
#pragma unroll
    for (int c = 0; c < 8; c++) vw[c] = a.validity[idx[c] >> 6];
  }
  uint64_t h[8];
  bool go[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const bool valid = (vw[c] >> (idx[c] & 63)) & 1ULL;
    const int64_t v = static_cast<int64_t>(kv[c]);
    h[c] = valid ? Tr::hash(kv[c]) : kNullHash;
    go[c] = ok[c] && (no_value || (valid && v >= mn && v <= mx));
  }
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const uint64_t m = mask_of(s_masks, h[c]);
    const uint64_t w = go[c] ? words[block_of(h[c], block_mask)] : 0ULL;
    pass[c] = go[c] && (w & m) == m;
  }
}

// probe_chain_small_kernel (COUNTED = false: positions 0 .. n of the column, or of the nullable row_sel `sel`; n =
// max_rows > 0) or probe_chain_sel_small_kernel (COUNTED = true: positions 0 .. min(*count_dev, max_rows) of `sel`;
// TRANSFER: then the survivors into the d.n outgoing filters) with the range of every filter flagged in r.mask applied
// to its own column. One workgroup of kSmallThreads; max_rows <= kSmallRows; the LDS of the twins. An item of a flagged
// filter is chain_probe_range, any other chain_probe as it is. COUNTED: no sel entry at or past the clamped count is
// read, for the twin's reasons: every row_sel read is bounded by n, the AND words hold no bit at or past n, and the tail
// and the inserts read sel only where a bit is set.
template <bool COUNTED, bool TRANSFER>
__global__ __launch_bounds__(kSmallThreads) void probe_chain_range_small_kernel(RangeChainArgs r, DstArgs d,
                                                                                const uint32_t* __restrict__ sel,
                                                                                const uint64_t* count_dev,
                                                                                uint64_t max_rows,
                                                                                uint32_t* __restrict__ out_sel,
                                                                                uint64_t* out_count) {
  static_assert(COUNTED || !TRANSFER, "there is no one-launch row-list transfer");
  constexpr uint32_t kSegs = kSmallRows / kSegRows;
  constexpr uint32_t kWaves = kSmallThreads / 64;
  __shared__ uint64_t s_masks[kNumMasks];
  __shared__ uint64_t s_pass[kMaxChain][kSegs * kWordsPerSeg];  // each filter's position-ordered pass words
  __shared__ uint64_t s_words[kSegs * kWordsPerSeg];
  __shared__ uint32_t s_cnt[kSegs];
  const ChainArgs& c = r.c;
  uint64_t n = max_rows;
  if constexpr (COUNTED) {
    // Every thread reads the count here, before the kernel's first barrier; *out_count is written by thread 0 in
    // small_sel_tail, behind three more barriers: out_count == count_dev is legal, as in probe_chain_sel_small_kernel.
    const uint64_t stored = *count_dev;
    n = stored < max_rows ? stored : max_rows;
    if (n == 0) {  // uniform: nothing else is read or written
      if (threadIdx.x == 0) *out_count = 0;
      return;
    }
  }
  fill_mask_table(s_masks);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n_segs = static_cast<uint32_t>((n + kSegRows - 1) / kSegRows);
  for (uint32_t it = wave; it < c.k * n_segs; it += kWaves) {
    const uint32_t f = it / n_segs, seg = it - f * n_segs;  // uniform
    const uint64_t base = static_cast<uint64_t>(seg) * kSegRows;
    const bool flagged = (r.mask >> f) & 1u;  // uniform; the host refuses a flagged HASH column
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
  small_sel_tail(s_words, s_cnt, n_segs, sel, out_sel, out_count);
  if constexpr (TRANSFER) {
    for (uint32_t j = 0; j < d.n; j++) {  // uniform
      if (d.key_type[j] == kKeyI64)
        small_insert_dst<kKeyI64>(d.words[j], d.block_mask[j], d.a[j], d.stats[j], s_masks, s_words, n_segs, n);
      else if (d.key_type[j] == kKeyI32)
        small_insert_dst<kKeyI32>(d.words[j], d.block_mask[j], d.a[j], d.stats[j], s_masks, s_words, n_segs, n);
      else
        small_insert_dst<kKeyHash>(d.words[j], d.block_mask[j], d.a[j], d.stats[j], s_masks, s_words, n_segs, n);
    }
  }
}

}  // namespace rpt
