// rpt_routed_insert.hpp — launchers of the routed insert's masked partition pass (kernels/partition_masked.hpp).
// Host code of librpt_gpu.so, included by rpt_gpu.hip inside its unnamed namespace, after ProfScope, inst_name,
// allow_dynamic_lds and RPT_DISPATCH_KD. Every kernel recorded here has a row in tests/kernel_ledger_routed.py
// (tests/test_kernel_ledger_routed_names.py scans this file).
#pragma once

// bits != nullptr: the rows are chosen by result bits (D: the dense mapping); else by the selection vector a.row_sel
// with its device-side count. n: the row count the host knows (n / max_rows); the grid is one workgroup per tile.
template <int K, bool D, bool SEL, int TM, int SP = 0>
void launch_partition_masked_tm(unsigned grid, hipStream_t s, const rpt::KeyArgs& a, uint64_t n, uint32_t slice_mask,
                                uint32_t* recs, uint32_t* runs, int64_t* stats, const uint64_t* bits,
                                const uint64_t* count_dev) {
  if constexpr (TM == 1 && SP == 0) {
    if (slice_mask + 1 <= 4) {  // few slices: wave-aggregated slice counters (as launch_partition_tm)
      launch_partition_masked_tm<K, D, SEL, 1, 4>(grid, s, a, n, slice_mask, recs, runs, stats, bits, count_dev);
      return;
    }
  }
  const size_t lds = rpt::partition_lds_bytes(slice_mask + 1, TM);
  static std::once_flag once;  // per instantiation; > 64 KiB of dynamic LDS must be opted into
  std::call_once(once, [] { allow_dynamic_lds(reinterpret_cast<const void*>(&rpt::partition_masked_kernel<K, D, SEL, TM, SP>)); });
  ProfScope prof(inst_name<K, D, SEL, TM, SP>("partition_masked_kernel"), s);
  hipLaunchKernelGGL((rpt::partition_masked_kernel<K, D, SEL, TM, SP>), dim3(grid), dim3(rpt::kTileThreads), lds, s, a, n,
                     slice_mask, recs, runs, stats, bits, count_dev);
  prof.end();
}

template <int K, bool D>
void launch_partition_bits_t(unsigned grid, hipStream_t s, const rpt::KeyArgs& a, uint64_t n, uint32_t slice_mask,
                             uint32_t* recs, uint32_t* runs, int64_t* stats, const uint64_t* bits, uint32_t tm) {
  if (tm == 2) launch_partition_masked_tm<K, D, false, 2>(grid, s, a, n, slice_mask, recs, runs, stats, bits, nullptr);
  else launch_partition_masked_tm<K, D, false, 1>(grid, s, a, n, slice_mask, recs, runs, stats, bits, nullptr);
}

template <int K, bool D>  // D unused: a selection vector is always the general mapping
void launch_partition_sel_t(unsigned grid, hipStream_t s, const rpt::KeyArgs& a, uint64_t max_rows, uint32_t slice_mask,
                            uint32_t* recs, uint32_t* runs, int64_t* stats, const uint64_t* count_dev, uint32_t tm) {
  if (tm == 2)
    launch_partition_masked_tm<K, false, true, 2>(grid, s, a, max_rows, slice_mask, recs, runs, stats, nullptr, count_dev);
  else
    launch_partition_masked_tm<K, false, true, 1>(grid, s, a, max_rows, slice_mask, recs, runs, stats, nullptr, count_dev);
}
