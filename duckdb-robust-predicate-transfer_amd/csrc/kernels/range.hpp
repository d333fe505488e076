// range.hpp — the min/max half of CREATE_BF's dynamic filter on the device: a key column tested against the range
// [stats[0], stats[1]] a filter's inserts folded (physical_create_bf.cpp:282-350 pushes ">= min" and "<= max" to the
// probe side's scan) -> result bits in the layout of probe_bits_kernel, or ANDed into a chain's accumulated bits.
// Part of librpt_gpu.so: included by rpt_gpu.hip (one translation unit: kernels and their launches
// stay together without relocatable device code).
#pragma once

namespace rpt {

// The key values of the 8 rows a lane owns in a segment, in exactly the row order of load_hashes<K, DENSE> (seg_row),
// so store_segment_bits<K, DENSE> and alive_flags<K, DENSE> apply unchanged. I32 values are sign-extended as the
// inserts' min/max fold extends them.
//  in[j]    : the row exists (row < n) and is wanted;
//  valid[j] : its key is not NULL (validity by physical index); meaningful where in[j];
//  v[j]     : its key value; meaningful where in[j].
// DENSE: 16-byte loads (a row that is not wanted is loaded with its neighbours). General mapping: a row that is not
// wanted makes none of its dependent gathers (row_sel -> key_sel -> key, validity).
template <int K, bool DENSE>
__device__ __forceinline__ void load_values(const KeyArgs& a, uint64_t base, uint64_t n, uint32_t lane,
                                            const bool (&want)[8], int64_t (&v)[8], bool (&in)[8], bool (&valid)[8]) {
  using Tr = KeyTraits<K>;
  using T = typename Tr::T;
  static_assert(Tr::kValues, "a range test needs key values: I64 or I32 columns");
  // rows left from `base` (uniform): per-row bounds checks are 32-bit
  const uint32_t rem = n > base ? static_cast<uint32_t>(n - base < kSegRows ? n - base : kSegRows) : 0u;
  if constexpr (DENSE) {
    constexpr int V = Tr::kVec;
    const T* kb = static_cast<const T*>(a.keys) + base;
    const uint64_t* vb = a.validity ? a.validity + (base >> 6) : nullptr;  // base is a multiple of 512
#pragma unroll
    for (int c = 0; c < 8 / V; c++) {
      const uint32_t off = static_cast<uint32_t>(c * 64 * V) + lane * V;
      T x[V];
      if (off + V <= rem) {
        if constexpr (V == 2) {
          const u64x2 r = stream_load<RPT_NT_PROBE_LOADS>(reinterpret_cast<const u64x2*>(kb + off));
          x[0] = static_cast<T>(r[0]);
          x[1] = static_cast<T>(r[1]);
        } else {
          const u32x4 r = stream_load<RPT_NT_PROBE_LOADS>(reinterpret_cast<const u32x4*>(kb + off));
#pragma unroll
          for (int e = 0; e < V; e++) x[e] = static_cast<T>(r[e]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < V; e++) x[e] = (off + e < rem) ? kb[off + e] : T(0);
      }
      // validity bits of this lane's V rows, shifted down to bits 0..V-1 (V | 64: one word)
      uint32_t vbits = (1u << V) - 1;
      if (vb != nullptr && off < rem) vbits = static_cast<uint32_t>(vb[off >> 6] >> (off & 63));
#pragma unroll
      for (int e = 0; e < V; e++) {
        in[c * V + e] = off + e < rem && want[c * V + e];
        valid[c * V + e] = (vbits >> e) & 1u;
        v[c * V + e] = static_cast<int64_t>(x[e]);
      }
    }
  } else {
    const T* keys = static_cast<const T*>(a.keys);
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint32_t off = static_cast<uint32_t>(c * 64) + lane;
      in[c] = off < rem && want[c];
      valid[c] = false;
      v[c] = 0;
      if (in[c]) {
        const uint64_t i = base + off;
        const uint64_t r = a.row_sel ? a.row_sel[i] : i;
        const uint64_t k = a.key_sel ? a.key_sel[r] : r;
        v[c] = static_cast<int64_t>(keys[k]);
        valid[c] = valid_at(a.validity, k);
      }
    }
  }
}

// One wave owns whole 512-row segments (persistent grid). stats = {min, max} of the filter, read from device memory
// when the kernel runs (a uniform load, once per wave): a captured launch sees the range the filter holds at replay.
//  min <= max : row i < n passes iff its key is not NULL and min <= key <= max (a NULL fails ">= min", as in the scan);
//  min >  max : no valid key was ever inserted (kMinInit / kMaxInit) and the reference pushes no min/max filter:
//               every row i < n passes, NULL rows included.
// Bits at positions >= n are 0.
// MASKED = false: every segment's 8 words and its count are written (seg_counts may be null).
// MASKED = true : `bits` / `seg_counts` are a chain's accumulated result, updated in place under the contract of
//                 probe_bits_masked_body: a segment whose words are all zero loads no key and gets count 0; otherwise
//                 the alive bits are ANDed with the range result and the words and the new count are written back
//                 (a segment belongs to exactly one wave, and its stores depend on its loads).
template <int K, bool DENSE, bool MASKED>
__global__ __launch_bounds__(kBlockThreads) void range_bits_kernel(const int64_t* __restrict__ stats, KeyArgs a,
                                                                   uint64_t n, uint64_t n_segs, uint64_t* bits,
                                                                   uint32_t* seg_counts) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  // the wave index is uniform: keep seg in scalar registers
  uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock +
                 static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
  const int64_t mn = stats[0], mx = stats[1];
  const bool no_value = mn > mx;
  for (; seg < n_segs; seg += total_waves) {
    bool want[8];
    if constexpr (MASKED) {
      const uint64_t mine = load_alive_word(bits, seg, lane);
      if (ballot64(mine != 0) == 0) {  // uniform
        if (lane == 0 && seg_counts != nullptr) seg_counts[seg] = 0;
        continue;
      }
      alive_flags<K, DENSE>(mine, lane, want);
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) want[j] = true;
    }
    int64_t v[8];
    bool in[8], valid[8], pass[8];
    load_values<K, DENSE>(a, seg * kSegRows, n, lane, want, v, in, valid);
#pragma unroll
    for (int j = 0; j < 8; j++) pass[j] = in[j] && (no_value || (valid[j] && v[j] >= mn && v[j] <= mx));
    store_segment_bits<K, DENSE>(pass, lane, seg, bits, seg_counts);
  }
}

}  // namespace rpt
