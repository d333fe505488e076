// probe_chain.hpp — USE_BF's filter chain for batches of any size (rpt_bf_probe_chain_ws): the stages after the
// first. The survivors of the filters so far are the accumulated result bits (row-ordered, Arrow Find layout,
// 8 words per 512-row segment) plus one count per segment; a stage ANDs its filter's result into them in place.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// A segment's 8 accumulated words, read by lanes 0..7 (the other lanes read the same 64 bytes again: no
// branch around the load). Lane l holds word l & 7.
__device__ __forceinline__ uint64_t load_alive_word(const uint64_t* acc, uint64_t seg, uint32_t lane) {
  return acc[seg * kWordsPerSeg + (lane & 7)];
}

// The alive bits of the 8 rows a lane owns in load_hashes<K, DENSE> order (seg_row), from the segment's words as
// load_alive_word left them (lane w < 8 holds word w). DENSE: a lane's V rows of one 16-byte load lie in one word,
// fetched from the lane that holds it; general mapping: row j * 64 + lane is bit `lane` of word j (uniform).
template <int K, bool DENSE>
__device__ __forceinline__ void alive_flags(uint64_t mine, uint32_t lane, bool (&alive)[8]) {
  if constexpr (DENSE) {
    constexpr int V = KeyTraits<K>::kVec;
    const uint32_t q = (lane * V) >> 6, sh = (lane * V) & 63;  // seg_row(c * V + e) = c * 64 V + lane * V + e
#pragma unroll
    for (int c = 0; c < 8 / V; c++) {
      const uint64_t w = __shfl(static_cast<unsigned long long>(mine), static_cast<int>(c * V + q), 64);
#pragma unroll
      for (int e = 0; e < V; e++) alive[c * V + e] = (w >> (sh + e)) & 1ULL;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) alive[j] = (readlane64(mine, j) >> lane) & 1ULL;
  }
}

// load_hashes' general mapping (row(c) = base + 64 c + lane: dictionaries, row_sel) for the alive rows only: a dead
// row makes none of its dependent gathers (row_sel -> key_sel -> key, validity).
template <int K>
__device__ __forceinline__ void load_hashes_alive(const KeyArgs& a, uint64_t base, uint64_t n, uint32_t lane,
                                                  const bool (&alive)[8], uint64_t (&h)[8], bool (&ok)[8]) {
  using Tr = KeyTraits<K>;
  using T = typename Tr::T;
  const uint32_t rem = n > base ? static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows) : 0u;
  const T* keys = static_cast<const T*>(a.keys);
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const uint32_t off = static_cast<uint32_t>(c * 64) + lane;
    ok[c] = off < rem && alive[c];
    uint64_t hv = 0;
    if (ok[c]) {
      const uint64_t i = base + off;
      const uint64_t r = a.row_sel ? a.row_sel[i] : i;
      const uint64_t k = a.key_sel ? a.key_sel[r] : r;
      hv = Tr::hash(keys[k]);
      if (Tr::kValues && !valid_at(a.validity, k)) hv = kNullHash;
    }
    h[c] = hv;
  }
}

// ---- stage i >= 1, GATHER / LDS (whole filter or hybrid): the masked probe ----------------------------------
// probe_bits_body (probe_direct.hpp) over the rows the previous filters kept. A wave owns whole segments; it reads
// the segment's 8 accumulated words first. All zero: no key is loaded, no filter word touched, the words stay as
// they are and the count becomes 0. Otherwise a row's alive bit is ANDed into ok[] before probe8, which makes no
// global / L2 gather for a row that is not ok, and the ANDed words and the new count are written back in place
// (a segment belongs to exactly one wave, and its stores depend on its loads).
//
// Full segments of flat NULL-free columns take a software-pipelined loop, one segment per step: the alive words are
// read two steps ahead and the keys one step ahead, so the decision to load a segment's keys waits on a load issued
// a whole step earlier. Keys are skipped per segment (not per 16-byte load). The general loop (tails, validity,
// dictionaries, row_sel) takes what is left; in the general row mapping dead rows skip their gathers one by one.
template <int K, bool DENSE, bool FILTER_IN_LDS, int THREADS, bool HYBRID>
__device__ __forceinline__ void probe_bits_masked_body(const uint64_t* __restrict__ words, uint64_t block_mask,
                                                       KeyArgs a, uint64_t n, uint64_t n_segs, uint64_t* acc,
                                                       uint32_t* seg_counts) {
  __shared__ uint64_t s_masks[kNumMasks];
  extern __shared__ uint64_t s_filter[];
  fill_mask_table(s_masks);
  if constexpr (FILTER_IN_LDS) {
    const uint64_t staged = HYBRID ? kHybridWords - 1 : block_mask;
    for (uint64_t i = threadIdx.x; i <= staged; i += blockDim.x) s_filter[i] = words[i];
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  constexpr uint32_t kWaves = THREADS / 64;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWaves +
                 static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
  if constexpr (DENSE && K != kKeySplit) {
    const uint64_t n_full = n / kSegRows;
    if (a.validity == nullptr && seg < n_full) {
      const uint64_t first = seg;
      // addresses past the last full segment are clamped (in range) and what they return is discarded
      auto word_at = [&](uint64_t sg) { return load_alive_word(acc, sg < n_full ? sg : n_full - 1, lane); };
      RawSeg<K> R[2];
      uint64_t m_cur = word_at(seg), m_nxt = word_at(seg + total_waves);
      bool live_cur = ballot64(m_cur != 0) != 0;  // uniform
      if (live_cur) R[0].load(a.keys, seg, lane);
      bool more = true;
      while (more) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
          if (more) {
            const uint64_t nseg = seg + total_waves;
            const uint64_t m_far = word_at(nseg + total_waves);
            const bool live_nxt = nseg < n_full && ballot64(m_nxt != 0) != 0;
            if (live_nxt) R[b ^ 1].load(a.keys, nseg, lane);
            asm volatile("" ::: "memory");  // issue the next segment's loads before this one's work
            if (live_cur) {
              uint64_t h[8];
              bool ok[8], pass[8];
              alive_flags<K, DENSE>(m_cur, lane, ok);
              R[b].hashes(h);
              probe8<FILTER_IN_LDS, HYBRID>(words, s_filter, s_masks, block_mask, h, ok, pass);
              store_segment_bits<K, DENSE>(pass, lane, seg, acc, seg_counts);
            } else if (lane == 0) {
              seg_counts[seg] = 0;
            }
            seg = nseg;
            m_cur = m_nxt;
            m_nxt = m_far;
            live_cur = live_nxt;
            more = seg < n_full;
          }
        }
      }
      // the general loop resumes at this wave's first segment past the full ones
      seg = first + (n_full - first + total_waves - 1) / total_waves * total_waves;
    }
  }
  for (; seg < n_segs; seg += total_waves) {
    const uint64_t mine = load_alive_word(acc, seg, lane);
    if (ballot64(mine != 0) == 0) {  // uniform
      if (lane == 0) seg_counts[seg] = 0;
      continue;
    }
    uint64_t h[8];
    bool alive[8], ok[8], pass[8];
    alive_flags<K, DENSE>(mine, lane, alive);
    if constexpr (DENSE) {
      load_hashes<K, DENSE>(a, seg * kSegRows, n, lane, h, ok);
#pragma unroll
      for (int j = 0; j < 8; j++) ok[j] = ok[j] && alive[j];
    } else {
      load_hashes_alive<K>(a, seg * kSegRows, n, lane, alive, h, ok);
    }
    probe8<FILTER_IN_LDS, HYBRID>(words, s_filter, s_masks, block_mask, h, ok, pass);
    store_segment_bits<K, DENSE>(pass, lane, seg, acc, seg_counts);
  }
}

template <int K, bool DENSE, bool FILTER_IN_LDS, int THREADS = kBlockThreads>
__global__ __launch_bounds__(THREADS) void probe_bits_masked_kernel(const uint64_t* __restrict__ words,
                                                                    uint64_t block_mask, KeyArgs a, uint64_t n,
                                                                    uint64_t n_segs, uint64_t* acc,
                                                                    uint32_t* seg_counts) {
  probe_bits_masked_body<K, DENSE, FILTER_IN_LDS, THREADS, false>(words, block_mask, a, n, n_segs, acc, seg_counts);
}
template <int K, bool DENSE>
__global__ __launch_bounds__(kLdsProbeThreads) void probe_bits_masked_hybrid_kernel(const uint64_t* __restrict__ words,
                                                                                    uint64_t block_mask, KeyArgs a,
                                                                                    uint64_t n, uint64_t n_segs,
                                                                                    uint64_t* acc, uint32_t* seg_counts) {
  probe_bits_masked_body<K, DENSE, true, kLdsProbeThreads, true>(words, block_mask, a, n, n_segs, acc, seg_counts);
}

// ---- stage i >= 1, PARTITIONED / BUCKETED: AND the stage's own result bits into the accumulated ones ----------
// acc[w] &= tmp[w] in 16-byte pieces, and every segment's count again by popcount. Four neighbouring lanes own a
// segment's four 16-byte pieces (n_units = 4 * n_segs, and the grid's stride is a multiple of 4, so the four
// leave the loop together).
__global__ __launch_bounds__(kBlockThreads) void bits_and_count_kernel(uint64_t* __restrict__ acc,
                                                                      const uint64_t* __restrict__ tmp, uint64_t n_segs,
                                                                      uint32_t* __restrict__ seg_counts) {
  const uint64_t n_units = n_segs * (kWordsPerSeg / 2);
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlockThreads;
  for (uint64_t u = static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; u < n_units; u += stride) {
    u64x2 x = reinterpret_cast<const u64x2*>(acc)[u];
    x &= reinterpret_cast<const u64x2*>(tmp)[u];
    reinterpret_cast<u64x2*>(acc)[u] = x;
    uint32_t c = static_cast<uint32_t>(__popcll(x[0]) + __popcll(x[1]));
    c += __shfl_xor(c, 1, 64);
    c += __shfl_xor(c, 2, 64);
    if ((u & 3) == 0) seg_counts[u >> 2] = c;
  }
}

}  // namespace rpt
