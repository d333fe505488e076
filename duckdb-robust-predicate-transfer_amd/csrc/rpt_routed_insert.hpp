// rpt_routed_insert.hpp — launchers of the routed insert's masked partition pass (kernels/partition_masked.hpp).
// Host code of librpt_gpu.so, included by rpt_gpu.hip inside its unnamed namespace, after rpt_launch.hpp
// (launch_kernel and the dispatch helpers). Every kernel recorded here has a row in tests/kernel_ledger_routed.py
// (tests/test_kernel_ledger_routed_names.py scans this file).
#pragma once

// bits != nullptr: the rows are chosen by result bits (D: the dense mapping); else by the selection vector a.row_sel
// with its device-side count. n: the row count the host knows (n / max_rows); the grid is one workgroup per tile.
template <int K, bool D, bool SEL, int TM, int SP = 0>
int launch_partition_masked_tm(unsigned grid, hipStream_t s, const rpt::KeyArgs& a, uint64_t n, uint32_t slice_mask,
                               uint32_t* recs, uint32_t* runs, int64_t* stats, const uint64_t* bits,
                               const uint64_t* count_dev) {
  if constexpr (TM == 1 && SP == 0) {
    if (slice_mask + 1 <= 4)  // few slices: wave-aggregated slice counters (as launch_partition_tm)
      return launch_partition_masked_tm<K, D, SEL, 1, 4>(grid, s, a, n, slice_mask, recs, runs, stats, bits, count_dev);
  }
  return launch_kernel<rpt::partition_masked_kernel<K, D, SEL, TM, SP>, K, D, SEL, TM, SP>(
      "partition_masked_kernel", kRecorded | kDynamicLds, grid, rpt::kTileThreads,
      rpt::partition_lds_bytes(slice_mask + 1, TM), s, a, n, slice_mask, recs, runs, stats, bits, count_dev);
}

// The pass of a column of run-time key type over tiles of tm * kTileRows rows. A selection vector (bits == nullptr) is
// always the general mapping, whatever `dense` says.
int launch_partition_masked(int key_type, bool dense, unsigned grid, hipStream_t s, const rpt::KeyArgs& a, uint64_t n,
                            uint32_t slice_mask, uint32_t* recs, uint32_t* runs, int64_t* stats, const uint64_t* bits,
                            const uint64_t* count_dev, uint32_t tm) {
  return dispatch_k(key_type, [&](auto k) {
    return dispatch_tm(tm, [&](auto t) {
      if (bits == nullptr)
        return launch_partition_masked_tm<k(), false, true, t()>(grid, s, a, n, slice_mask, recs, runs, stats, nullptr,
                                                                 count_dev);
      return dispatch_bool(dense, [&](auto d) {
        return launch_partition_masked_tm<k(), d(), false, t()>(grid, s, a, n, slice_mask, recs, runs, stats, bits, nullptr);
      });
    });
  });
}
