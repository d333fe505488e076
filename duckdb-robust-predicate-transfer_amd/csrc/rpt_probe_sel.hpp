// rpt_probe_sel.hpp — the device-counted probes: rpt_bf_probe_chain_sel_ws, rpt_bf_transfer_sel_ws,
// rpt_bf_transfer_insert_sel_ws, their sizing and strategy functions, and the launcher of their first stage
// (kernels/probe_sel.hpp). Host code of librpt_gpu.so, included by rpt_gpu.hip inside its extern "C" block, after
// enqueue_chain_later_stages, launch_sel_tail, check_routed_insert and enqueue_transfer_inserts. Every kernel recorded
// here has a row in tests/kernel_ledger_sel.py (tests/test_kernel_ledger_sel_names.py scans this file).
#pragma once

extern "C++" {
namespace {

template <int K, int MODE>
void launch_probe_bits_sel_m(unsigned grid, hipStream_t s, const rpt_bf* bf, const rpt::KeyArgs& a,
                             const uint64_t* count_dev, uint64_t max_rows, uint64_t n_segs, uint64_t* bits,
                             uint32_t* counts) {
  size_t lds = 0;
  if constexpr (MODE != rpt::kSelGather) {
    lds = 8ULL << std::min(bf->log_num_blocks, rpt::kLdsDirectMaxLog);
    static std::once_flag once;  // per instantiation; > 64 KiB of dynamic LDS must be opted into
    std::call_once(once, [] { allow_dynamic_lds(reinterpret_cast<const void*>(&rpt::probe_bits_sel_kernel<K, MODE>)); });
  }
  ProfScope prof(inst_name<K, MODE>("probe_bits_sel_kernel"), s);
  hipLaunchKernelGGL((rpt::probe_bits_sel_kernel<K, MODE>), dim3(grid), dim3(rpt::sel_probe_threads<MODE>()), lds, s,
                     bf->words, (1ULL << bf->log_num_blocks) - 1, a, count_dev, max_rows, n_segs, bits, counts);
  prof.end();
}

template <int K>
void launch_probe_bits_sel_k(int strategy, unsigned grid, hipStream_t s, const rpt_bf* bf, const rpt::KeyArgs& a,
                             const uint64_t* count_dev, uint64_t max_rows, uint64_t n_segs, uint64_t* bits,
                             uint32_t* counts) {
  if (strategy == RPT_PROBE_GATHER)
    launch_probe_bits_sel_m<K, rpt::kSelGather>(grid, s, bf, a, count_dev, max_rows, n_segs, bits, counts);
  else if (bf->log_num_blocks <= rpt::kLdsDirectMaxLog)
    launch_probe_bits_sel_m<K, rpt::kSelLds>(grid, s, bf, a, count_dev, max_rows, n_segs, bits, counts);
  else
    launch_probe_bits_sel_m<K, rpt::kSelHybrid>(grid, s, bf, a, count_dev, max_rows, n_segs, bits, counts);
}

}  // namespace
}  // extern "C++"

// ---- the chain over a selection vector with a device-side count -------------------------------------------------
// Workspace (all 256-aligned): accumulated result bits | their per-segment counts | the tail's group sums | group
// offsets, for max_rows rows. No stage area and no temporary bits: no stage routes.
namespace {
// A filter's strategy in a device-counted chain: a routed stage would partition all max_rows positions and read every
// sel entry, so PARTITIONED and BUCKETED (resolved by AUTO or forced) become GATHER, whose masked form does no work
// past the count. LDS, whole-filter or hybrid, stays.
int sel_strategy(const rpt_bf* bf, uint64_t max_rows) {
  const int st = resolve_strategy(bf->probe_strategy.load(), bf->log_num_blocks, max_rows);
  return routed(st) ? RPT_PROBE_GATHER : st;
}
size_t sel_chain_workspace_layout(uint64_t max_rows, void* base, ChainWorkspace* ws) {
  const uint64_t n_segs = ceil_div(max_rows, rpt::kSegRows);
  const uint64_t n_groups = ceil_div(n_segs, rpt::kGroupSegs);
  constexpr int kParts = 4;
  const size_t sz[kParts] = {align256(n_segs * rpt::kWordsPerSeg * 8), align256(n_groups * rpt::kGroupSegs * 4),
                             align256(n_groups * 4), align256(n_groups * 4)};
  size_t off[kParts], total = 0;
  for (int i = 0; i < kParts; i++) {
    off[i] = total;
    total += sz[i];
  }
  if (ws) {
    char* p = static_cast<char*>(base);
    ws->bits = reinterpret_cast<uint64_t*>(p + off[0]);
    ws->seg_counts = reinterpret_cast<uint32_t*>(p + off[1]);
    ws->group_sums = reinterpret_cast<uint32_t*>(p + off[2]);
    ws->group_offs = reinterpret_cast<uint32_t*>(p + off[3]);
    ws->tmp_bits = nullptr;
    ws->stage = nullptr;
    ws->stage_bytes = 0;
  }
  return total;
}

// Do the max_rows-entry ranges at sel and out_sel share a byte?
bool sel_ranges_overlap(const uint32_t* sel, const uint32_t* out_sel, uint64_t max_rows) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(sel), b = reinterpret_cast<uintptr_t>(out_sel);
  const uintptr_t bytes = static_cast<uintptr_t>(max_rows) * sizeof(uint32_t);
  return a < b + bytes && b < a + bytes;
}

// The body of the three entry points. n_dst == 0: no destinations (rpt_bf_probe_chain_sel_ws). route: as transfer_impl.
// The order of the checks: everything that needs no look into a handle first (lists, counts, null handles, a
// destination that is also probed, count_dev, out_count_dev, max_rows, and with max_rows > 0 sel, out_sel and their
// overlap); max_rows == 0 then sets the count and returns; then the handles are looked into.
int probe_chain_sel_impl(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                         rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst, bool transfer,
                         const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                         uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, bool route,
                         void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream) {
  if (!filters || !cols || !out_count_dev || (transfer && (!dst_filters || !dst_cols)))
    return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n_filters == 0 || n_filters > RPT_MAX_CHAIN)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_filters=%u outside 1..%d", n_filters, RPT_MAX_CHAIN);
  if (transfer && (n_dst == 0 || n_dst > RPT_MAX_CHAIN))
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_dst=%u outside 1..%d", n_dst, RPT_MAX_CHAIN);
  // handles are compared before any of them is looked into
  for (uint32_t f = 0; f < n_filters; f++)
    if (!filters[f]) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter %u", f);
  for (uint32_t j = 0; j < n_dst; j++) {
    if (!dst_filters[j]) return fail(RPT_ERR_INVALID_ARGUMENT, "null destination filter %u", j);
    for (uint32_t f = 0; f < n_filters; f++)
      if (dst_filters[j] == filters[f])
        return fail(RPT_ERR_INVALID_ARGUMENT, "destination filter %u is probed filter %u of the same call", j, f);
  }
  if (!count_dev) return fail(RPT_ERR_INVALID_ARGUMENT, "null count_dev");
  if (max_rows >= (1ULL << 32))
    return fail(RPT_ERR_INVALID_ARGUMENT, "max_rows=%llu rows exceeds uint32 sel_t", (unsigned long long)max_rows);
  hipStream_t s = as_stream(stream);
  if (max_rows == 0) {  // nothing can be selected: the count, stream-ordered, and nothing else
    RPT_HIP(hipMemsetAsync(out_count_dev, 0, sizeof(uint64_t), s));
    return RPT_OK;
  }
  if (!sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null sel");
  if (!out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  if (sel_ranges_overlap(sel, out_sel, max_rows))
    return fail(RPT_ERR_INVALID_ARGUMENT, "out_sel overlaps sel (%llu entries each)", (unsigned long long)max_rows);
  int st = check_chain_filters(filters, n_filters);
  if (st != RPT_OK) return st;
  int strategy[RPT_MAX_CHAIN];
  for (uint32_t f = 0; f < n_filters; f++) {
    st = check_col(&cols[f]);
    if (st != RPT_OK) return st;
    const int L = filters[f]->log_num_blocks;
    strategy[f] = sel_strategy(filters[f], max_rows);
    if (!strategy_supported(strategy[f], L))
      return fail(RPT_ERR_INVALID_ARGUMENT, "probe strategy %d unsupported for a 2^%d-block filter (filter %u)", strategy[f],
                  L, f);
  }
  const int device = filters[0]->device;
  for (uint32_t j = 0; j < n_dst; j++) {
    if (dst_filters[j]->device != device)
      return fail(RPT_ERR_INVALID_ARGUMENT, "destination filter %u is not on the chain's device", j);
    st = check_col(&dst_cols[j]);
    if (st != RPT_OK) return st;
  }
  // which destinations route, and their share of the insert workspace (they run one after another on the stream)
  bool dst_routed[RPT_MAX_CHAIN] = {};
  if (route)
    for (uint32_t j = 0; j < n_dst; j++) {
      st = check_routed_insert(dst_filters[j], max_rows, insert_workspace, insert_workspace_bytes, &dst_routed[j]);
      if (st != RPT_OK) return st;
    }
  const size_t need = sel_chain_workspace_layout(max_rows, nullptr, nullptr);
  if (!workspace || workspace_bytes < need)
    return fail(RPT_ERR_WORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, need);
  if (misaligned16(workspace)) return fail(RPT_ERR_INVALID_ARGUMENT, "workspace %p is not 16-byte aligned", workspace);
  RPT_ON_DEVICE(device);
  // every destination's capture and in-flight check, and every probed filter's pending clear, before anything is enqueued
  for (uint32_t j = 0; j < n_dst; j++) RPT_REFUSE_CAPTURE_WRITE(dst_filters[j], s, "transfer");
  for (uint32_t f = 0; f < n_filters; f++) RPT_SETTLE(filters[f], s);
  ChainWorkspace ws;
  sel_chain_workspace_layout(max_rows, workspace, &ws);
  const uint64_t n_segs = ceil_div(max_rows, rpt::kSegRows);
  // stage 0: the only kernel that reads *count_dev; it writes every segment's words and count
  {
    const rpt_bf* bf = filters[0];
    const rpt::KeyArgs a{cols[0].keys, cols[0].key_sel, cols[0].validity, sel};
    const unsigned grid = strategy[0] == RPT_PROBE_GATHER ? persistent_grid(device, n_segs)
                                                          : lds_probe_grid(device, bf->log_num_blocks, n_segs);
    switch (cols[0].key_type) {
      case RPT_KEY_I64:
        launch_probe_bits_sel_k<rpt::kKeyI64>(strategy[0], grid, s, bf, a, count_dev, max_rows, n_segs, ws.bits, ws.seg_counts);
        break;
      case RPT_KEY_I32:
        launch_probe_bits_sel_k<rpt::kKeyI32>(strategy[0], grid, s, bf, a, count_dev, max_rows, n_segs, ws.bits, ws.seg_counts);
        break;
      default:
        launch_probe_bits_sel_k<rpt::kKeyHash>(strategy[0], grid, s, bf, a, count_dev, max_rows, n_segs, ws.bits, ws.seg_counts);
        break;
    }
    RPT_LAUNCHED("probe_bits_sel_kernel");
  }
  // the later stages over all max_rows positions: the zero bits past the count keep the masked probes away from sel
  st = enqueue_chain_later_stages(filters, cols, n_filters, strategy, sel, max_rows, ws, device, stream);
  if (st != RPT_OK) return st;
  st = launch_sel_tail(s, ws.bits, ws.seg_counts, ws.group_sums, ws.group_offs, n_segs, sel, out_sel, out_count_dev);
  if (st != RPT_OK || n_dst == 0) return st;
  return enqueue_transfer_inserts(dst_filters, dst_cols, n_dst, dst_routed, ws.bits, sel, out_sel, out_count_dev, max_rows,
                                  insert_workspace, s);
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
  return sel_chain_workspace_layout(max_rows, nullptr, nullptr);
}

int rpt_bf_probe_chain_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                              const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                              uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  return probe_chain_sel_impl(filters, cols, n_filters, nullptr, nullptr, 0, false, sel, count_dev, max_rows, out_sel,
                              out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream);
}

int rpt_bf_transfer_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                           rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                           const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                           uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  return probe_chain_sel_impl(filters, cols, n_filters, dst_filters, dst_cols, n_dst, true, sel, count_dev, max_rows,
                              out_sel, out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream);
}

int rpt_bf_transfer_insert_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                  rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                                  const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                                  uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                  void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream) {
  return probe_chain_sel_impl(filters, cols, n_filters, dst_filters, dst_cols, n_dst, true, sel, count_dev, max_rows,
                              out_sel, out_count_dev, workspace, workspace_bytes, true, insert_workspace,
                              insert_workspace_bytes, stream);
}
