// rpt_probe_sel.hpp — the device-counted probes: rpt_bf_probe_chain_sel_ws, rpt_bf_transfer_sel_ws,
// rpt_bf_transfer_insert_sel_ws, their sizing and strategy functions, and the launcher of their first stage
// (kernels/probe_sel.hpp). Host code of librpt_gpu.so, included by rpt_gpu.hip inside its extern "C" block, after
// rpt_chain_call.hpp, whose run_chain_call is the body of the entry points; the launches go through launch_kernel
// (rpt_launch.hpp). Every kernel recorded here has a row in tests/kernel_ledger_sel.py
// (tests/test_kernel_ledger_sel_names.py scans this file).
#pragma once

extern "C++" {
namespace {

// The first stage of a device-counted chain over a column of key type K: the gather, or the filter (LDS) or its first
// 128 KiB (hybrid) staged in LDS.
template <int K, int MODE>
int launch_probe_bits_sel_m(unsigned grid, hipStream_t s, const rpt_bf* bf, const rpt::KeyArgs& a,
                            const uint64_t* count_dev, uint64_t max_rows, uint64_t n_segs, uint64_t* bits,
                            uint32_t* counts) {
  constexpr bool kInLds = MODE != rpt::kSelGather;
  return launch_kernel<rpt::probe_bits_sel_kernel<K, MODE>, K, MODE>(
      "probe_bits_sel_kernel", kRecorded | (kInLds ? kDynamicLds : 0), grid, rpt::sel_probe_threads<MODE>(),
      kInLds ? 8ULL << std::min(bf->log_num_blocks, rpt::kLdsDirectMaxLog) : 0, s, bf->words,
      (1ULL << bf->log_num_blocks) - 1, a, count_dev, max_rows, n_segs, bits, counts);
}

template <int K>
int launch_probe_bits_sel_k(int strategy, unsigned grid, hipStream_t s, const rpt_bf* bf, const rpt::KeyArgs& a,
                            const uint64_t* count_dev, uint64_t max_rows, uint64_t n_segs, uint64_t* bits,
                            uint32_t* counts) {
  if (strategy == RPT_PROBE_GATHER)
    return launch_probe_bits_sel_m<K, rpt::kSelGather>(grid, s, bf, a, count_dev, max_rows, n_segs, bits, counts);
  if (bf->log_num_blocks <= rpt::kLdsDirectMaxLog)
    return launch_probe_bits_sel_m<K, rpt::kSelLds>(grid, s, bf, a, count_dev, max_rows, n_segs, bits, counts);
  return launch_probe_bits_sel_m<K, rpt::kSelHybrid>(grid, s, bf, a, count_dev, max_rows, n_segs, bits, counts);
}

}  // namespace
}  // extern "C++"

// ---- the chain over a selection vector with a device-side count -------------------------------------------------
// Workspace (all 256-aligned): accumulated result bits | their per-segment counts | the tail's group sums | group
// offsets, for max_rows rows. No stage area and no temporary bits: no stage routes (chain_workspace_layout without
// stages). run_chain_call (rpt_chain_call.hpp) is the body of the three entry points; the order of its checks:
// everything that needs no look into a handle first (lists, counts, null handles, a destination that is also probed,
// count_dev, out_count_dev, max_rows, and with max_rows > 0 sel, out_sel and their overlap); max_rows == 0 then sets
// the count and returns; then the handles are looked into.
namespace {
// Stage 0 of a device-counted chain: the only kernel that reads *count_dev; it writes every segment's words and count.
int enqueue_sel_stage0(const ChainCall& c, int strategy, int device, const ChainWorkspace& ws, hipStream_t s) {
  const rpt_bf* bf = c.filters[0];
  const rpt_key_column& col = c.cols[0];
  const uint64_t n_segs = ceil_div(c.n, rpt::kSegRows);
  const rpt::KeyArgs a{col.keys, col.key_sel, col.validity, c.sel};
  const unsigned grid = strategy == RPT_PROBE_GATHER ? persistent_grid(device, n_segs)
                                                     : lds_probe_grid(device, bf->log_num_blocks, n_segs);
  return dispatch_k(col.key_type, [&](auto k) {
    return launch_probe_bits_sel_k<k()>(strategy, grid, s, bf, a, c.count_dev, c.n, n_segs, ws.bits, ws.seg_counts);
  });
}
}  // namespace

int rpt_bf_probe_sel_strategy_for(const rpt_bf* bf, uint64_t max_rows) {
  if (!bf) return -fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  return sel_strategy(bf, max_rows);
}

size_t rpt_bf_probe_chain_sel_workspace_bytes(const rpt_bf* const* filters, uint32_t n_filters, uint64_t max_rows) {
  if (check_chain_filters(filters, n_filters) != RPT_OK) return 0;
  if (max_rows >= (1ULL << 32)) {
    fail(RPT_ERR_INVALID_ARGUMENT, "max_rows=%llu rows exceeds uint32 sel_t", (unsigned long long)max_rows);
    return 0;
  }
  return chain_workspace_layout(filters, n_filters, max_rows, 1, false, nullptr, nullptr);
}

int rpt_bf_probe_chain_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                              const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                              uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, false, nullptr, nullptr, 0, true, sel, count_dev, max_rows, 0, out_sel,
                         out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream});
}

int rpt_bf_transfer_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                           rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                           const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                           uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, true, sel, count_dev, max_rows, 0,
                         out_sel, out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream});
}

int rpt_bf_transfer_insert_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                  rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                                  const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                                  uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                  void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, true, sel, count_dev, max_rows, 0,
                         out_sel, out_count_dev, workspace, workspace_bytes, true, insert_workspace,
                         insert_workspace_bytes, stream});
}
