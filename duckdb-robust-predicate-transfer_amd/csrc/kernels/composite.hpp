// composite.hpp — composite (multi-column) join keys hashed inside the kernels (rpt_hash_keys_composite,
// rpt_bf_insert_composite, rpt_bf_probe_chain_composite, rpt_bf_transfer_composite, rpt_bf_insert_multi_composite):
// HashColumns (reference src/bloom_filter.cpp:11-24) is Hash(col_0) followed by CombineHash(h, Hash(col_j)); here every
// column of a key is read once and the combined hash goes straight into the store, the atomic OR or the probe, where
// the two-pass route (hash_kernel<K, false>, then hash_kernel<K, true> per further column) writes the hash array to
// memory and reads it back between the columns.
// A column's key type is a wave-uniform run-time branch, not a template parameter: the three kernels have two, two
// and three instantiations, not one per mix of key types.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

constexpr uint32_t kMaxKeyCols = RPT_MAX_KEY_COLUMNS;             // columns of one key
constexpr uint32_t kMaxChainKeyCols = RPT_MAX_CHAIN_KEY_COLUMNS;  // columns of all keys of one side of a one-launch call

// One column of a composite key: rpt_key_column as the kernels read it.
struct CompositeCol {
  const void* keys;
  const uint32_t* key_sel;
  const uint64_t* validity;
  int32_t key_type;  // kKeyI64 / kKeyI32, or kKeyHash as column 0 (a prefix already hashed)
};
// One key: the argument of the hash and insert kernels (n_cols >= 2: the host forwards a one-column key).
struct CompositeKeyArgs {
  CompositeCol col[kMaxKeyCols];
  uint32_t n_cols;
};
// One side of a one-launch call, the probed filters or the destinations: a flat column table, per filter the index of
// its first column (first[f] .. first[f + 1] are filter f's columns), the words and block masks, and for destinations
// the stats pointers (min/max: one-column keys only).
struct CompositeSide {
  CompositeCol col[kMaxChainKeyCols];
  uint64_t* words[kMaxChain];
  uint64_t block_mask[kMaxChain];
  int64_t* stats[kMaxChain];
  uint8_t first[kMaxChain + 1];
  uint32_t n;
};
// both sides and the five scalar arguments fit HIP's 4 KiB of kernel arguments
static_assert(2 * sizeof(CompositeSide) + 5 * 8 <= 4096, "chain_composite_small_kernel's arguments exceed 4 KiB");
static_assert(kMaxChainKeyCols <= 255 && kMaxKeyCols <= kMaxChainKeyCols, "column indices are bytes");

// A raw key as loaded (I32 zero-extended: Hash(int32) hashes the value through uint32) -> its contribution.
__device__ __forceinline__ uint64_t composite_contrib(uint64_t raw, bool values, bool valid) {
  const uint64_t hv = values ? murmur64(raw) : raw;
  return valid ? hv : kNullHash;
}

// ---- the general mapping: row(c) = base + 64 c + lane ---------------------------------------------------------
// One column's contributions for the 8 rows idx[] (all in range: positions past n were clamped by the caller), level
// by level as chain_hashes (probe_direct.hpp) does: the key_sel level if any, the keys, the validity words, the 8 loads
// of a level back to back.
__device__ __forceinline__ void composite_col_general(const CompositeCol& col, const uint64_t (&idx)[8],
                                                      uint64_t (&contrib)[8]) {
  uint64_t k[8];
#pragma unroll
  for (int c = 0; c < 8; c++) k[c] = idx[c];
  if (col.key_sel != nullptr) {
#pragma unroll
    for (int c = 0; c < 8; c++) k[c] = col.key_sel[idx[c]];
  }
  uint64_t raw[8];
  if (col.key_type == kKeyI32) {
    const uint32_t* keys = static_cast<const uint32_t*>(col.keys);
#pragma unroll
    for (int c = 0; c < 8; c++) raw[c] = keys[k[c]];
  } else {
    const uint64_t* keys = static_cast<const uint64_t*>(col.keys);
#pragma unroll
    for (int c = 0; c < 8; c++) raw[c] = keys[k[c]];
  }
  const bool values = col.key_type != kKeyHash;  // a HASH column carries no key values: its validity is not read
  uint64_t vw[8];
#pragma unroll
  for (int c = 0; c < 8; c++) vw[c] = ~0ULL;
  if (values && col.validity != nullptr) {
#pragma unroll
    for (int c = 0; c < 8; c++) vw[c] = col.validity[k[c] >> 6];
  }
#pragma unroll
  for (int c = 0; c < 8; c++) contrib[c] = composite_contrib(raw[c], values, (vw[c] >> (k[c] & 63)) & 1ULL);
}

// The combined hashes of a lane's 8 positions of the segment at `base` (base < n). The row_sel level is loaded once
// and shared by every column; then the columns one after another. Positions at or past n read position `base` (in
// range) and are discarded (ok[c] false): no row_sel entry at or past n is read.
// Column by column, not all columns' keys first: the validity bit of a key needs its physical index, so all-first
// keeps 8 raw keys and 8 indices per column live, 4 x (16 + 16) = 128 VGPRs, which is the one-launch kernel's whole
// budget under __launch_bounds__(1024) before a hash or an address exists.
__device__ __forceinline__ void composite_hashes(const CompositeCol* cols, uint32_t n_cols,
                                                 const uint32_t* __restrict__ row_sel, uint64_t base, uint64_t n,
                                                 uint32_t lane, uint64_t (&h)[8], bool (&ok)[8]) {
  const uint32_t rem = static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows);  // base < n
  uint64_t idx[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const uint32_t off = static_cast<uint32_t>(c * 64) + lane;
    ok[c] = off < rem;
    idx[c] = base + (ok[c] ? off : 0u);
  }
  if (row_sel != nullptr) {
#pragma unroll
    for (int c = 0; c < 8; c++) idx[c] = row_sel[idx[c]];
  }
  composite_col_general(cols[0], idx, h);
  for (uint32_t j = 1; j < n_cols; j++) {  // uniform
    uint64_t b[8];
    composite_col_general(cols[j], idx, b);
#pragma unroll
    for (int c = 0; c < 8; c++) h[c] = combine_hash(h[c], b[c]);
  }
}

// ---- the dense mapping: row(c, e) = base + 256 c + 4 lane + e, c < 2, e < 4 ---------------------------------------
// Every column is flat (no key_sel) and 16-byte aligned, and all columns share this one mapping whatever their key
// types (load_hashes<K, true>'s depends on KeyTraits<K>::kVec, so an I32 and an I64 column would disagree about which
// row a register holds): a lane owns two runs of four consecutive rows, one 16-byte load of an I32 column per run and
// two of an I64 / HASH column. h[4 c + e] is row(c, e): insert8<kKeyI32, true>'s order.
__device__ __forceinline__ uint32_t composite_dense_off(int c, uint32_t lane) { return static_cast<uint32_t>(c * 256) + lane * 4; }

// One column's 8 raw keys and the validity bits of its two runs (bits 0..3 of vbits[c]). FULL: a whole segment
// (uniform), every load issued back to back; else rows at or past rem are not read.
template <bool FULL>
__device__ __forceinline__ void composite_dense_load(const CompositeCol& col, uint64_t base, uint32_t rem, uint32_t lane,
                                                     uint64_t (&raw)[8], uint32_t (&vbits)[2]) {
  if (col.key_type == kKeyI32) {
    const uint32_t* kb = static_cast<const uint32_t*>(col.keys) + base;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const uint32_t off = composite_dense_off(c, lane);
      if constexpr (FULL) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(kb + off);
#pragma unroll
        for (int e = 0; e < 4; e++) raw[c * 4 + e] = x[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) raw[c * 4 + e] = off + e < rem ? kb[off + e] : 0u;
      }
    }
  } else {
    const uint64_t* kb = static_cast<const uint64_t*>(col.keys) + base;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const uint32_t off = composite_dense_off(c, lane);
      if constexpr (FULL) {
        const u64x2 x = *reinterpret_cast<const u64x2*>(kb + off), y = *reinterpret_cast<const u64x2*>(kb + off + 2);
        raw[c * 4] = x[0];
        raw[c * 4 + 1] = x[1];
        raw[c * 4 + 2] = y[0];
        raw[c * 4 + 3] = y[1];
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) raw[c * 4 + e] = off + e < rem ? kb[off + e] : 0ULL;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const uint32_t off = composite_dense_off(c, lane);
    vbits[c] = 0xFu;
    // base is a multiple of 512 and off of 4: the run's four bits lie in one word
    if (col.key_type != kKeyHash && col.validity != nullptr && (FULL || off < rem))
      vbits[c] = static_cast<uint32_t>(col.validity[(base + off) >> 6] >> (off & 63));
  }
}

// The combined hashes of a lane's 8 rows of the segment at `base` in the dense mapping: every column's loads are
// issued before the hashing starts.
template <bool FULL>
__device__ __forceinline__ void composite_dense_hashes(const CompositeKeyArgs& a, uint64_t base, uint32_t rem,
                                                       uint32_t lane, uint64_t (&h)[8]) {
  uint64_t raw[kMaxKeyCols][8];
  uint32_t vbits[kMaxKeyCols][2];
#pragma unroll
  for (uint32_t j = 0; j < kMaxKeyCols; j++)
    if (j < a.n_cols) composite_dense_load<FULL>(a.col[j], base, rem, lane, raw[j], vbits[j]);  // uniform
#pragma unroll
  for (uint32_t j = 0; j < kMaxKeyCols; j++) {
    if (j < a.n_cols) {
      const bool values = a.col[j].key_type != kKeyHash;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint64_t b = composite_contrib(raw[j][i], values, (vbits[j][i >> 2] >> (i & 3)) & 1u);
        h[i] = j == 0 ? b : combine_hash(h[i], b);
      }
    }
  }
}

// The segment's hashes in either mapping; ok[i]: the row is below n.
template <bool DENSE>
__device__ __forceinline__ void composite_segment(const CompositeKeyArgs& a, uint64_t base, uint64_t n, uint32_t lane,
                                                  uint64_t (&h)[8], bool (&ok)[8]) {
  if constexpr (DENSE) {
    const uint32_t rem = static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows);  // base < n
    if (rem == static_cast<uint32_t>(kSegRows)) composite_dense_hashes<true>(a, base, rem, lane, h);  // uniform
    else composite_dense_hashes<false>(a, base, rem, lane, h);
#pragma unroll
    for (int i = 0; i < 8; i++) ok[i] = composite_dense_off(i >> 2, lane) + static_cast<uint32_t>(i & 3) < rem;
  } else {
    composite_hashes(a.col, a.n_cols, nullptr, base, n, lane, h, ok);
  }
}

// ---- rpt_hash_keys_composite ------------------------------------------------------------------------------------
// out[i] = HashColumns of row i, i < n. A persistent grid, a wave owns whole 512-row segments, like insert_kernel.
// DENSE: every column flat and 16-byte aligned, and `out` 16-byte aligned: the hashes of a run are stored as two
// 16-byte vectors.
template <bool DENSE>
__global__ __launch_bounds__(kBlockThreads) void hash_composite_kernel(CompositeKeyArgs a, uint64_t n, uint64_t n_segs,
                                                                      uint64_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); seg < n_segs;
       seg += total_waves) {
    const uint64_t base = seg * kSegRows;
    uint64_t h[8];
    bool ok[8];
    composite_segment<DENSE>(a, base, n, lane, h, ok);
    if constexpr (DENSE) {
#pragma unroll
      for (int c = 0; c < 2; c++) {
        uint64_t* o = out + base + composite_dense_off(c, lane);
        if (ok[c * 4 + 3]) {  // the whole run is below n
          *reinterpret_cast<u64x2*>(o) = u64x2{h[c * 4], h[c * 4 + 1]};
          *reinterpret_cast<u64x2*>(o + 2) = u64x2{h[c * 4 + 2], h[c * 4 + 3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (ok[c * 4 + e]) o[e] = h[c * 4 + e];
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; c++)
        if (ok[c]) out[base + static_cast<uint32_t>(c * 64) + lane] = h[c];
    }
  }
}

// ---- rpt_bf_insert_composite ------------------------------------------------------------------------------------
// insert_kernel (misc.hpp) with the key hashed from its columns here: the mask table in LDS, a row whose hash equals
// the previous row's dropped before its atomic (insert8: the previous row is always below n where this one is), one
// relaxed agent-scope atomic OR per surviving row. No min/max: a composite key carries none, and a one-column key
// takes insert_kernel.
template <bool DENSE>
__global__ __launch_bounds__(kBlockThreads) void insert_composite_kernel(uint64_t* __restrict__ words, uint64_t block_mask,
                                                                        CompositeKeyArgs a, uint64_t n, uint64_t n_segs) {
  __shared__ uint64_t s_masks[kNumMasks];
  fill_mask_table(s_masks);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); seg < n_segs;
       seg += total_waves) {
    uint64_t h[8];
    bool ok[8];
    composite_segment<DENSE>(a, seg * kSegRows, n, lane, h, ok);
    if constexpr (DENSE) insert8<kKeyI32, true>(words, block_mask, s_masks, h, ok, lane);  // runs of four rows
    else insert8<kKeyI64, false>(words, block_mask, s_masks, h, ok, lane);
  }
}

// ---- the one-launch calls -----------------------------------------------------------------------------------------
// Column `i` of a side as the single-column helpers take it.
__device__ __forceinline__ KeyArgs composite_key_args(const CompositeCol& col, const uint32_t* row_sel) {
  return KeyArgs{col.keys, col.key_sel, col.validity, row_sel};
}

// One destination with a key of two or more columns: small_insert_dst (probe_sel_small.hpp) without the min/max.
__device__ __forceinline__ void small_insert_dst_composite(uint64_t* __restrict__ words, uint64_t block_mask,
                                                           const CompositeCol* cols, uint32_t n_cols,
                                                           const uint32_t* __restrict__ row_sel, const uint64_t* s_masks,
                                                           const uint64_t* s_words, uint32_t n_segs, uint64_t n) {
  constexpr uint32_t kWaves = kSmallThreads / 64;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t seg = wave; seg < n_segs; seg += kWaves) {
    const uint64_t mine = s_words[seg * kWordsPerSeg + (lane & 7)];  // lane w < 8 holds word w (load_alive_word)
    if (ballot64(mine != 0) == 0) continue;                          // uniform: a dead segment
    uint64_t h[8];
    bool alive[8], ins[8];
    alive_flags<kKeyI64, false>(mine, lane, alive);
    composite_hashes(cols, n_cols, row_sel, static_cast<uint64_t>(seg) * kSegRows, n, lane, h, ins);
#pragma unroll
    for (int c = 0; c < 8; c++) ins[c] = ins[c] && alive[c];
    insert8<kKeyI64, false>(words, block_mask, s_masks, h, ins, lane);
  }
}

// transfer_small_kernel's schedule (transfer_small.hpp) with a key per filter: <true,false> the chain
// (rpt_bf_probe_chain_composite), <true,true> the transfer (rpt_bf_transfer_composite), <false,true> the sink alone
// (rpt_bf_insert_multi_composite). The (filter, 512-position segment) items are spread over the 16 waves; a key of one
// column takes chain_probe<K> / small_insert_dst<K> through a uniform branch, so its result, min/max included, is the
// single-column kernels' by construction. One workgroup of kSmallThreads; 0 < n <= kSmallRows. No row_sel entry at or
// past n is read (composite_hashes, chain_hashes and chain_hashes_alive bound every read by n, the AND words hold no bit
// at or past n, the tail reads row_sel only where a bit is set). The inserts read row_sel after the tail has begun to
// store out_sel: the host refuses ranges that overlap.
template <bool PROBED, bool TRANSFER>
__global__ __launch_bounds__(kSmallThreads) void chain_composite_small_kernel(CompositeSide p, CompositeSide d,
                                                                              const uint32_t* __restrict__ row_sel,
                                                                              uint64_t n, uint32_t* __restrict__ out_sel,
                                                                              uint64_t* __restrict__ out_count) {
  static_assert(PROBED || TRANSFER, "a call probes, inserts or both");
  constexpr uint32_t kSegs = kSmallRows / kSegRows;
  constexpr uint32_t kWaves = kSmallThreads / 64;
  __shared__ uint64_t s_masks[kNumMasks];
  __shared__ uint64_t s_words[kSegs * kWordsPerSeg];
  fill_mask_table(s_masks);
  const uint32_t n_segs = static_cast<uint32_t>((n + kSegRows - 1) / kSegRows);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if constexpr (PROBED) {
    __shared__ uint64_t s_pass[kMaxChain][kSegs * kWordsPerSeg];  // each filter's position-ordered pass words
    __shared__ uint32_t s_cnt[kSegs];
    __syncthreads();
    for (uint32_t it = wave; it < p.n * n_segs; it += kWaves) {
      const uint32_t f = it / n_segs, seg = it - f * n_segs;  // uniform
      const uint64_t base = static_cast<uint64_t>(seg) * kSegRows;
      const uint32_t c0 = p.first[f], n_cols = p.first[f + 1] - c0;
      bool pass[8];
      if (n_cols == 1) {
        const KeyArgs a = composite_key_args(p.col[c0], row_sel);
        if (p.col[c0].key_type == kKeyI64) chain_probe<kKeyI64>(a, p.words[f], p.block_mask[f], s_masks, base, n, lane, pass);
        else if (p.col[c0].key_type == kKeyI32) chain_probe<kKeyI32>(a, p.words[f], p.block_mask[f], s_masks, base, n, lane, pass);
        else chain_probe<kKeyHash>(a, p.words[f], p.block_mask[f], s_masks, base, n, lane, pass);
      } else {
        uint64_t h[8];
        bool ok[8];
        composite_hashes(&p.col[c0], n_cols, row_sel, base, n, lane, h, ok);
        const uint64_t* words = p.words[f];
        const uint64_t block_mask = p.block_mask[f];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const uint64_t m = mask_of(s_masks, h[j]);
          const uint64_t w = ok[j] ? words[block_of(h[j], block_mask)] : 0ULL;
          pass[j] = ok[j] && (w & m) == m;
        }
      }
      store_segment_bits<kKeyI64, false>(pass, lane, seg, s_pass[f], nullptr);
    }
    __syncthreads();
    // the AND over the filters, word by word; then each segment's survivor count
    for (uint32_t w = threadIdx.x; w < n_segs * kWordsPerSeg; w += kSmallThreads) {
      uint64_t x = s_pass[0][w];
      for (uint32_t f = 1; f < p.n; f++) x &= s_pass[f][w];
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
  if constexpr (TRANSFER) {
    for (uint32_t j = 0; j < d.n; j++) {  // uniform
      const uint32_t c0 = d.first[j], n_cols = d.first[j + 1] - c0;
      if (n_cols == 1) {
        const KeyArgs a = composite_key_args(d.col[c0], row_sel);
        if (d.col[c0].key_type == kKeyI64)
          small_insert_dst<kKeyI64>(d.words[j], d.block_mask[j], a, d.stats[j], s_masks, s_words, n_segs, n);
        else if (d.col[c0].key_type == kKeyI32)
          small_insert_dst<kKeyI32>(d.words[j], d.block_mask[j], a, d.stats[j], s_masks, s_words, n_segs, n);
        else
          small_insert_dst<kKeyHash>(d.words[j], d.block_mask[j], a, d.stats[j], s_masks, s_words, n_segs, n);
      } else {
        small_insert_dst_composite(d.words[j], d.block_mask[j], &d.col[c0], n_cols, row_sel, s_masks, s_words, n_segs, n);
      }
    }
  }
}

}  // namespace rpt
