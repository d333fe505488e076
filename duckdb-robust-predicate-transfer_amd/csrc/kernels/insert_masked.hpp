// insert_masked.hpp — inserts whose row set lives on the device (rpt_bf_insert_bits, rpt_bf_insert_sel,
// rpt_bf_transfer_ws): the survivors of a probe go into the filter the table sends on without their count ever
// reaching the host. The rows are given as result bits (the layout of rpt_bf_probe_bits / the chain's accumulated
// bits) or as a selection vector with a device-side count. Both kernels are insert_kernel's (misc.hpp) shape:
// wave64, a persistent grid, a wave owns whole 512-row segments, one relaxed agent-scope atomic OR per inserted row,
// the key min/max folded on the way.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// The atomic ORs of the 8 rows a lane owns in a segment (load_hashes<K, DENSE> order); ins[j]: row j is inserted.
// insert_kernel's shortcut (a row whose hash equals the previous row's sets nothing new, so its atomic is dropped)
// holds only where the previous row is inserted itself: a previous row that is dead, NULL-free but out of range,
// or masked out has set nothing, and dropping the atomic would lose the key (a false negative). The previous row
// is this lane's last hash or the previous lane's (ds_bpermute), its ins flag this lane's or a ballot bit.
template <int K, bool DENSE>
__device__ __forceinline__ void insert8(uint64_t* __restrict__ words, uint64_t block_mask, const uint64_t* s_masks,
                                        const uint64_t (&h)[8], const bool (&ins)[8], uint32_t lane) {
  const int src = static_cast<int>(((lane + 63) & 63) << 2);
  const uint32_t prev_lane = (lane + 63) & 63;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    uint64_t prev;
    bool has_prev;
    if constexpr (DENSE && KeyTraits<K>::kVec > 1) {
      constexpr int V = KeyTraits<K>::kVec;
      if (j % V != 0) {
        prev = h[j - 1];
        has_prev = ins[j - 1];
      } else {
        prev = shfl_u64(h[j + V - 1], src);
        has_prev = lane != 0 && ((ballot64(ins[j + V - 1]) >> prev_lane) & 1ULL);
      }
    } else {
      prev = shfl_u64(h[j], src);
      has_prev = lane != 0 && ((ballot64(ins[j]) >> prev_lane) & 1ULL);
    }
    if (ins[j] && !(has_prev && prev == h[j])) {
      __hip_atomic_fetch_or(words + block_of(h[j], block_mask), mask_of(s_masks, h[j]), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// load_hashes<K, true> (the 16-byte loads of a flat column) for a masked insert: ins[j] = row in range and alive,
// and the min/max fold covers the alive, valid (non-NULL), in-range rows only (load_hashes<..., MM> folds every
// valid row of the segment).
template <int K>
__device__ __forceinline__ void load_dense_alive(const KeyArgs& a, uint64_t base, uint64_t n, uint32_t lane,
                                                 const bool (&alive)[8], uint64_t (&h)[8], bool (&ins)[8],
                                                 int64_t (&mm)[2]) {
  using Tr = KeyTraits<K>;
  using T = typename Tr::T;
  constexpr int V = Tr::kVec;
  const uint32_t rem = n > base ? static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows) : 0u;
  const T* kb = static_cast<const T*>(a.keys) + base;
  const uint64_t* vb = a.validity ? a.validity + (base >> 6) : nullptr;  // base is a multiple of 512
#pragma unroll
  for (int c = 0; c < 8 / V; c++) {
    const uint32_t off = static_cast<uint32_t>(c * 64 * V) + lane * V;
    T v[V];
    if (off + V <= rem) {
      if constexpr (V == 2) {
        const u64x2 x = *reinterpret_cast<const u64x2*>(kb + off);
        v[0] = static_cast<T>(x[0]);
        v[1] = static_cast<T>(x[1]);
      } else {
        const u32x4 x = *reinterpret_cast<const u32x4*>(kb + off);
#pragma unroll
        for (int e = 0; e < V; e++) v[e] = static_cast<T>(x[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < V; e++) v[e] = (off + e < rem) ? kb[off + e] : T(0);
    }
    // validity bits of this lane's V rows, shifted down to bits 0..V-1 (V | 64: one word)
    uint32_t vbits = (1u << V) - 1;
    if (Tr::kValues && vb != nullptr && off < rem) vbits = static_cast<uint32_t>(vb[off >> 6] >> (off & 63));
#pragma unroll
    for (int e = 0; e < V; e++) {
      const bool valid = (vbits >> e) & 1u;
      ins[c * V + e] = off + e < rem && alive[c * V + e];
      uint64_t hv = Tr::hash(v[e]);
      if (Tr::kValues && !valid) hv = kNullHash;
      h[c * V + e] = hv;
      if constexpr (Tr::kValues) {
        if (ins[c * V + e] && valid) {
          mm[0] = min(mm[0], static_cast<int64_t>(v[e]));
          mm[1] = max(mm[1], static_cast<int64_t>(v[e]));
        }
      }
    }
  }
}

// load_hashes_alive (probe_chain.hpp: the general mapping, a dead row makes none of its dependent gathers) with the
// min/max fold of the alive, valid rows. Columns without values (HASH) are load_hashes_alive itself.
template <int K>
__device__ __forceinline__ void load_general_alive(const KeyArgs& a, uint64_t base, uint64_t n, uint32_t lane,
                                                   const bool (&alive)[8], uint64_t (&h)[8], bool (&ins)[8],
                                                   int64_t (&mm)[2]) {
  using Tr = KeyTraits<K>;
  using T = typename Tr::T;
  if constexpr (!Tr::kValues) {
    load_hashes_alive<K>(a, base, n, lane, alive, h, ins);
  } else {
    const uint32_t rem = n > base ? static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows) : 0u;
    const T* keys = static_cast<const T*>(a.keys);
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint32_t off = static_cast<uint32_t>(c * 64) + lane;
      ins[c] = off < rem && alive[c];
      uint64_t hv = 0;
      if (ins[c]) {
        const uint64_t i = base + off;
        const uint64_t r = a.row_sel ? a.row_sel[i] : i;
        const uint64_t k = a.key_sel ? a.key_sel[r] : r;
        const T kv = keys[k];
        hv = Tr::hash(kv);
        if (valid_at(a.validity, k)) {
          mm[0] = min(mm[0], static_cast<int64_t>(kv));
          mm[1] = max(mm[1], static_cast<int64_t>(kv));
        } else {
          hv = kNullHash;
        }
      }
      h[c] = hv;
    }
  }
}

// ---- rows given as result bits ---------------------------------------------------------------------------------
// The masked twin of insert_kernel: row i < n of the column (row i, or row_sel[i]) is inserted iff bit i of `bits`
// is set (8 words per 512-row segment, LSB first; bits at positions >= n are ignored: such a row is out of range).
// A wave reads its segment's 8 words first; all zero (a ballot): no key is loaded and no atomic issued.
template <int K, bool DENSE>
__global__ __launch_bounds__(kBlockThreads) void insert_bits_kernel(uint64_t* __restrict__ words, uint64_t block_mask,
                                                                   KeyArgs a, uint64_t n, uint64_t n_segs,
                                                                   const uint64_t* __restrict__ bits,
                                                                   int64_t* __restrict__ stats) {
  __shared__ uint64_t s_masks[kNumMasks];
  fill_mask_table(s_masks);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  int64_t mm[2] = {kMinInit, kMaxInit};
  for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); seg < n_segs;
       seg += total_waves) {
    const uint64_t mine = load_alive_word(bits, seg, lane);
    if (ballot64(mine != 0) == 0) continue;  // uniform: a dead segment
    uint64_t h[8];
    bool alive[8], ins[8];
    alive_flags<K, DENSE>(mine, lane, alive);
    if constexpr (DENSE) load_dense_alive<K>(a, seg * kSegRows, n, lane, alive, h, ins, mm);
    else load_general_alive<K>(a, seg * kSegRows, n, lane, alive, h, ins, mm);
    insert8<K, DENSE>(words, block_mask, s_masks, h, ins, lane);
  }
  if constexpr (KeyTraits<K>::kValues) {
    wave_minmax(mm[0], mm[1]);
    publish_minmax(mm[0], mm[1], stats);
  }
}

// ---- rows given as a selection vector with a device-side count --------------------------------------------------
// Rows sel[0 .. min(*count_dev, max_rows)) of the column (a.row_sel = sel: the general mapping). Every wave reads
// the count once (a uniform load; the kernel that wrote it is earlier on the stream) and strides over 512-entry
// pieces of sel; load_hashes bounds every sel read by the clamped count, so no entry at or past it is touched.
// The grid is sized for max_rows on the host: waves past the count find no piece.
template <int K>
__global__ __launch_bounds__(kBlockThreads) void insert_sel_kernel(uint64_t* __restrict__ words, uint64_t block_mask,
                                                                  KeyArgs a, const uint64_t* __restrict__ count_dev,
                                                                  uint64_t max_rows, int64_t* __restrict__ stats) {
  constexpr bool MM = KeyTraits<K>::kValues;
  __shared__ uint64_t s_masks[kNumMasks];
  fill_mask_table(s_masks);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  const uint64_t stored = *count_dev;
  const uint64_t n = stored < max_rows ? stored : max_rows;
  const uint64_t n_segs = (n + kSegRows - 1) / kSegRows;
  int64_t mm[2] = {kMinInit, kMaxInit};
  for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); seg < n_segs;
       seg += total_waves) {
    uint64_t h[8];
    bool ok[8];
    load_hashes<K, false, MM>(a, seg * kSegRows, n, lane, h, ok, mm);
    insert8<K, false>(words, block_mask, s_masks, h, ok, lane);
  }
  if constexpr (MM) {
    wave_minmax(mm[0], mm[1]);
    publish_minmax(mm[0], mm[1], stats);
  }
}

}  // namespace rpt
