// probe_sel_small.hpp — the device-counted chain and transfer for small batches (rpt_bf_probe_chain_sel,
// rpt_bf_transfer_sel): the twin of probe_chain_small_kernel (probe_direct.hpp) that reads its row count from the
// device, and, for a transfer, inserts the survivors into the outgoing filters before it ends. One workgroup, one
// launch, no workspace: a whole backward step of predicate transfer over one DuckDB-sized vector (USE_BF chain,
// then CREATE_BF sink) that an earlier probe feeds without its count reaching the host.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// The filters a transfer sends its survivors on to: rpt_bf_transfer_sel's dst_filters / dst_cols (a.row_sel = sel).
struct DstArgs {
  uint64_t* words[kMaxChain];
  uint64_t block_mask[kMaxChain];
  KeyArgs a[kMaxChain];
  int32_t key_type[kMaxChain];
  int64_t* stats[kMaxChain];
  uint32_t n;
};

// chain_hashes (probe_direct.hpp: every level's 8 loads back to back, positions past n read position `base`) for an
// insert: ins[c] = position in range and alive, and the min/max of the alive valid keys folded into mm as
// load_general_alive (insert_masked.hpp) folds them. Columns without values (HASH) are chain_hashes itself.
template <int K>
__device__ __forceinline__ void chain_hashes_alive(const KeyArgs& a, uint64_t base, uint64_t n, uint32_t lane,
                                                   const bool (&alive)[8], uint64_t (&h)[8], bool (&ins)[8],
                                                   int64_t (&mm)[2]) {
  using Tr = KeyTraits<K>;
  using T = typename Tr::T;
  if constexpr (!Tr::kValues) {
    chain_hashes<K>(a, base, n, lane, h, ins);
#pragma unroll
    for (int c = 0; c < 8; c++) ins[c] = ins[c] && alive[c];
  } else {
    const uint32_t rem = static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows);  // base < n
    uint64_t idx[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint32_t off = static_cast<uint32_t>(c * 64) + lane;
      const bool ok = off < rem;
      ins[c] = ok && alive[c];
      idx[c] = base + (ok ? off : 0u);  // positions past n read position `base` (in range) and are discarded
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
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const bool valid = (vw[c] >> (idx[c] & 63)) & 1ULL;
      h[c] = valid ? Tr::hash(kv[c]) : kNullHash;
      if (ins[c] && valid) {
        mm[0] = min(mm[0], static_cast<int64_t>(kv[c]));
        mm[1] = max(mm[1], static_cast<int64_t>(kv[c]));
      }
    }
  }
}

// One destination of a transfer: the positions whose bit is set in s_words (the AND over the probed filters, 8 words
// per 512-position segment) into `words`, as insert_sel_kernel (insert_masked.hpp) inserts a selection: insert8's
// atomic ORs (a repeated key is dropped before its atomic), NULL_HASH for a selected NULL row, and the wave's min/max
// published once after its segments. A segment without a survivor (a ballot over its words) loads no key.
template <int K>
__device__ __forceinline__ void small_insert_dst(uint64_t* __restrict__ words, uint64_t block_mask, const KeyArgs& a,
                                                 int64_t* __restrict__ stats, const uint64_t* s_masks,
                                                 const uint64_t* s_words, uint32_t n_segs, uint64_t n) {
  constexpr uint32_t kWaves = kSmallThreads / 64;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t mm[2] = {kMinInit, kMaxInit};
  for (uint32_t seg = wave; seg < n_segs; seg += kWaves) {
    const uint64_t mine = s_words[seg * kWordsPerSeg + (lane & 7)];  // lane w < 8 holds word w (load_alive_word)
    if (ballot64(mine != 0) == 0) continue;                          // uniform: a dead segment
    uint64_t h[8];
    bool alive[8], ins[8];
    alive_flags<K, false>(mine, lane, alive);
    chain_hashes_alive<K>(a, static_cast<uint64_t>(seg) * kSegRows, n, lane, alive, h, ins, mm);
    insert8<K, false>(words, block_mask, s_masks, h, ins, lane);
  }
  if constexpr (KeyTraits<K>::kValues) {
    wave_minmax(mm[0], mm[1]);
    publish_minmax(mm[0], mm[1], stats);
  }
}

// probe_chain_small_kernel over positions 0 .. min(*count_dev, max_rows) of `sel` (every column's row_sel), then,
// TRANSFER, the survivors into the d.n outgoing filters. One workgroup of kSmallThreads; max_rows <= kSmallRows.
// No sel entry at or past the clamped count is read: chain_hashes bounds every row_sel read by n, the AND words hold
// no bit at or past n, and the tail and the inserts read sel only where a bit is set.
template <bool TRANSFER>
__global__ __launch_bounds__(kSmallThreads) void probe_chain_sel_small_kernel(ChainArgs c, DstArgs d,
                                                                              const uint32_t* __restrict__ sel,
                                                                              const uint64_t* count_dev,
                                                                              uint64_t max_rows,
                                                                              uint32_t* __restrict__ out_sel,
                                                                              uint64_t* out_count) {
  constexpr uint32_t kSegs = kSmallRows / kSegRows;
  constexpr uint32_t kWaves = kSmallThreads / 64;
  __shared__ uint64_t s_masks[kNumMasks];
  __shared__ uint64_t s_pass[kMaxChain][kSegs * kWordsPerSeg];  // each filter's position-ordered pass words
  __shared__ uint64_t s_words[kSegs * kWordsPerSeg];
  __shared__ uint32_t s_cnt[kSegs];
  // Every thread reads the count here, before the kernel's first barrier; *out_count is written by thread 0 in
  // small_sel_tail, behind three more barriers. That order is what makes out_count == count_dev legal (neither
  // pointer is __restrict__). With a count of 0 thread 0 stores 0 at once: over an aliased count that stores the
  // value every other thread reads anyway.
  const uint64_t stored = *count_dev;
  const uint64_t n = stored < max_rows ? stored : max_rows;
  if (n == 0) {  // uniform: nothing else is read or written
    if (threadIdx.x == 0) *out_count = 0;
    return;
  }
  fill_mask_table(s_masks);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n_segs = static_cast<uint32_t>((n + kSegRows - 1) / kSegRows);
  for (uint32_t it = wave; it < c.k * n_segs; it += kWaves) {
    const uint32_t f = it / n_segs, seg = it - f * n_segs;  // uniform
    const uint64_t base = static_cast<uint64_t>(seg) * kSegRows;
    bool pass[8];
    if (c.key_type[f] == kKeyI64) chain_probe<kKeyI64>(c.a[f], c.words[f], c.block_mask[f], s_masks, base, n, lane, pass);
    else if (c.key_type[f] == kKeyI32) chain_probe<kKeyI32>(c.a[f], c.words[f], c.block_mask[f], s_masks, base, n, lane, pass);
    else chain_probe<kKeyHash>(c.a[f], c.words[f], c.block_mask[f], s_masks, base, n, lane, pass);
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
