// rpt_probe_range.hpp — the min/max range stage (kernels/range.hpp): rpt_bf_range_bits, and the workspace chain and
// transfers that apply a filter's range on the device before its Bloom test (rpt_bf_probe_chain_range_ws,
// rpt_bf_transfer_range_ws, rpt_bf_transfer_insert_range_ws). Host code of librpt_gpu.so, included by rpt_gpu.hip
// inside its extern "C" block, directly after rpt_probe_sel_small.hpp. Every kernel recorded here has a row in
// tests/kernel_ledger_range.py (tests/test_kernel_ledger_range_names.py scans this file).
#pragma once

extern "C++" {
namespace {

template <int K, bool D, bool M>
void launch_range_bits_t(unsigned grid, hipStream_t s, const rpt_bf* bf, const rpt::KeyArgs& a, uint64_t n,
                         uint64_t n_segs, uint64_t* bits, uint32_t* counts) {
  ProfScope prof(inst_name<K, D, M>("range_bits_kernel"), s);
  hipLaunchKernelGGL((rpt::range_bits_kernel<K, D, M>), dim3(grid), dim3(rpt::kBlockThreads), 0, s, bf->stats, a, n,
                     n_segs, bits, counts);
  prof.end();
}

// The range test of one column (I64 or I32: the caller has refused HASH) over n rows. masked: AND into the accumulated
// bits / counts in place; else write every segment's words (and its count where counts != nullptr).
template <bool M>
void launch_range_bits_m(int key_type, bool dense, unsigned grid, hipStream_t s, const rpt_bf* bf,
                         const rpt::KeyArgs& a, uint64_t n, uint64_t n_segs, uint64_t* bits, uint32_t* counts) {
  if (key_type == RPT_KEY_I64) {
    if (dense) launch_range_bits_t<rpt::kKeyI64, true, M>(grid, s, bf, a, n, n_segs, bits, counts);
    else launch_range_bits_t<rpt::kKeyI64, false, M>(grid, s, bf, a, n, n_segs, bits, counts);
  } else {
    if (dense) launch_range_bits_t<rpt::kKeyI32, true, M>(grid, s, bf, a, n, n_segs, bits, counts);
    else launch_range_bits_t<rpt::kKeyI32, false, M>(grid, s, bf, a, n, n_segs, bits, counts);
  }
}

}  // namespace
}  // extern "C++"

namespace {

int enqueue_range_stage(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n, bool masked,
                        uint64_t* bits, uint32_t* counts, hipStream_t s) {
  const uint64_t n_segs = ceil_div(n, rpt::kSegRows);
  const unsigned grid = persistent_grid(bf->device, n_segs);
  const rpt::KeyArgs a{col->keys, col->key_sel, col->validity, row_sel};
  const bool dense = dense_ok(col, row_sel);
  if (masked) launch_range_bits_m<true>(col->key_type, dense, grid, s, bf, a, n, n_segs, bits, counts);
  else launch_range_bits_m<false>(col->key_type, dense, grid, s, bf, a, n, n_segs, bits, counts);
  RPT_LAUNCHED("range_bits_kernel");
  return RPT_OK;
}

// The checks of a range call that need no look into a handle, in the order of the non-range calls; then the mask and
// the flagged columns. dst_filters == nullptr: a chain without destinations.
int check_range_args(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters, uint32_t range_mask,
                     rpt_bf* const* dst_filters, uint32_t n_dst) {
  if (n_filters == 0 || n_filters > RPT_MAX_CHAIN)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_filters=%u outside 1..%d", n_filters, RPT_MAX_CHAIN);
  if (dst_filters && (n_dst == 0 || n_dst > RPT_MAX_CHAIN))
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_dst=%u outside 1..%d", n_dst, RPT_MAX_CHAIN);
  // handles are compared before any of them is looked into
  for (uint32_t f = 0; f < n_filters; f++)
    if (!filters[f]) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter %u", f);
  for (uint32_t j = 0; dst_filters && j < n_dst; j++) {
    if (!dst_filters[j]) return fail(RPT_ERR_INVALID_ARGUMENT, "null destination filter %u", j);
    for (uint32_t f = 0; f < n_filters; f++)
      if (dst_filters[j] == filters[f])
        return fail(RPT_ERR_INVALID_ARGUMENT, "destination filter %u is probed filter %u of the same call", j, f);
  }
  if ((range_mask >> n_filters) != 0)  // n_filters <= RPT_MAX_CHAIN < 32
    return fail(RPT_ERR_INVALID_ARGUMENT, "range_mask=0x%x flags a filter at or above n_filters=%u", range_mask, n_filters);
  for (uint32_t f = 0; f < n_filters; f++) {
    const int st = check_col(&cols[f]);
    if (st != RPT_OK) return st;
    if (((range_mask >> f) & 1u) && cols[f].key_type == RPT_KEY_HASH)
      return fail(RPT_ERR_INVALID_ARGUMENT, "range_mask flags filter %u, whose column holds hashes (no key values)", f);
  }
  return RPT_OK;
}

// chain_workspace_layout with the temporary bits present whenever any filter routes, filter 0 included: filter 0
// runs as a later stage here, so the layout is taken over filter 0 followed by the whole list.
size_t range_workspace_layout(const rpt_bf* const* filters, uint32_t k, uint64_t n, void* base, ChainWorkspace* ws) {
  const rpt_bf* later[RPT_MAX_CHAIN + 1];
  later[0] = filters[0];
  for (uint32_t f = 0; f < k; f++) later[f + 1] = filters[f];
  return chain_workspace_layout(later, k + 1, n, base, ws);
}

// The body of the three chain calls for range_mask != 0 (the caller has run check_range_args). *survivor_bits as in
// probe_chain_ws_impl: the accumulated bits once the call is enqueued, nullptr when nothing was probed (n == 0).
int probe_chain_range_impl(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                           uint32_t range_mask, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                           uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream,
                           const uint64_t** survivor_bits) {
  *survivor_bits = nullptr;
  int st = check_chain_filters(filters, n_filters);
  if (st != RPT_OK) return st;
  if (n >= (1ULL << 32)) return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds uint32 sel_t", (unsigned long long)n);
  int strategy[RPT_MAX_CHAIN];
  for (uint32_t f = 0; f < n_filters; f++) {
    const int L = filters[f]->log_num_blocks;
    strategy[f] = resolve_strategy(filters[f]->probe_strategy.load(), L, n);
    if (!strategy_supported(strategy[f], L))
      return fail(RPT_ERR_INVALID_ARGUMENT, "probe strategy %d unsupported for a 2^%d-block filter (filter %u)", strategy[f],
                  L, f);
  }
  const int device = filters[0]->device;
  RPT_ON_DEVICE(device);
  hipStream_t s = as_stream(stream);
  if (n == 0) {
    RPT_HIP(hipMemsetAsync(out_count_dev, 0, sizeof(uint64_t), s));
    return RPT_OK;
  }
  if (!out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  const size_t need = range_workspace_layout(filters, n_filters, n, nullptr, nullptr);
  if (!workspace || workspace_bytes < need)
    return fail(RPT_ERR_WORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, need);
  if (misaligned16(workspace)) return fail(RPT_ERR_INVALID_ARGUMENT, "workspace %p is not 16-byte aligned", workspace);
  for (uint32_t f = 0; f < n_filters; f++) RPT_SETTLE(filters[f], s);
  ChainWorkspace ws;
  range_workspace_layout(filters, n_filters, n, workspace, &ws);
  // the flagged columns' range stages, in filter order: the first writes the accumulated bits and counts, the others
  // AND into them
  bool first = true;
  for (uint32_t f = 0; f < n_filters; f++) {
    if (!((range_mask >> f) & 1u)) continue;
    st = enqueue_range_stage(filters[f], &cols[f], row_sel, n, !first, ws.bits, ws.seg_counts, s);
    if (st != RPT_OK) return st;
    first = false;
  }
  // every filter, filter 0 included, as a later stage of the chain
  st = enqueue_chain_later_stages(filters, cols, n_filters, strategy, row_sel, n, ws, device, stream, 0);
  if (st != RPT_OK) return st;
  *survivor_bits = ws.bits;
  const uint64_t n_segs = ceil_div(n, rpt::kSegRows);
  return launch_sel_tail(s, ws.bits, ws.seg_counts, ws.group_sums, ws.group_offs, n_segs, row_sel, out_sel, out_count_dev);
}

// The body of rpt_bf_transfer_range_ws and rpt_bf_transfer_insert_range_ws for range_mask != 0: transfer_impl with
// the range chain in place of the plain one.
int transfer_range_impl(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters, uint32_t range_mask,
                        rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                        const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev, void* workspace,
                        size_t workspace_bytes, bool route, void* insert_workspace, size_t insert_workspace_bytes,
                        rpt_stream_t stream) {
  if (!filters || !cols || !out_count_dev || !dst_filters || !dst_cols)
    return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  int st = check_range_args(filters, cols, n_filters, range_mask, dst_filters, n_dst);
  if (st != RPT_OK) return st;
  st = check_chain_filters(filters, n_filters);
  if (st != RPT_OK) return st;
  if (n >= (1ULL << 32)) return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds uint32 sel_t", (unsigned long long)n);
  const int device = filters[0]->device;
  for (uint32_t j = 0; j < n_dst; j++) {
    if (dst_filters[j]->device != device)
      return fail(RPT_ERR_INVALID_ARGUMENT, "destination filter %u is not on the chain's device", j);
    st = check_col(&dst_cols[j]);
    if (st != RPT_OK) return st;
  }
  // which destinations route, and their share of the insert workspace (they run one after another on the stream)
  bool routed_dst[RPT_MAX_CHAIN] = {};
  if (route && n > 0)
    for (uint32_t j = 0; j < n_dst; j++) {
      st = check_routed_insert(dst_filters[j], n, insert_workspace, insert_workspace_bytes, &routed_dst[j]);
      if (st != RPT_OK) return st;
    }
  RPT_ON_DEVICE(device);
  hipStream_t s = as_stream(stream);
  // every destination's capture and in-flight check before the chain enqueues anything (n == 0 writes none)
  if (n > 0)
    for (uint32_t j = 0; j < n_dst; j++) RPT_REFUSE_CAPTURE_WRITE(dst_filters[j], s, "transfer");
  const uint64_t* bits = nullptr;
  st = probe_chain_range_impl(filters, cols, n_filters, range_mask, row_sel, n, out_sel, out_count_dev, workspace,
                              workspace_bytes, stream, &bits);
  if (st != RPT_OK || n == 0) return st;
  return enqueue_transfer_inserts(dst_filters, dst_cols, n_dst, routed_dst, bits, row_sel, out_sel, out_count_dev, n,
                                  insert_workspace, s);
}
}  // namespace

int rpt_bf_range_bits(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n,
                      uint64_t* out_bits, rpt_stream_t stream) {
  if (!bf || !out_bits) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n >= (1ULL << 32)) return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds uint32 sel_t", (unsigned long long)n);
  if (n == 0) return RPT_OK;
  const int st = check_col(col);
  if (st != RPT_OK) return st;
  if (col->key_type == RPT_KEY_HASH)
    return fail(RPT_ERR_INVALID_ARGUMENT, "range test of a column that holds hashes (no key values)");
  RPT_ON_DEVICE(bf->device);
  hipStream_t s = as_stream(stream);
  RPT_SETTLE(bf, s);
  return enqueue_range_stage(bf, col, row_sel, n, false, out_bits, nullptr, s);
}

size_t rpt_bf_probe_chain_range_workspace_bytes(const rpt_bf* const* filters, uint32_t n_filters, uint32_t range_mask,
                                                uint64_t n_rows) {
  if (range_mask == 0) return rpt_bf_probe_chain_workspace_bytes(filters, n_filters, n_rows);
  // the mask is checked before any handle is looked into (check_chain_filters compares the filters' devices)
  if (filters && n_filters >= 1 && n_filters <= RPT_MAX_CHAIN && (range_mask >> n_filters) != 0) {
    fail(RPT_ERR_INVALID_ARGUMENT, "range_mask=0x%x flags a filter at or above n_filters=%u", range_mask, n_filters);
    return 0;
  }
  if (check_chain_filters(filters, n_filters) != RPT_OK) return 0;
  if (n_rows >= (1ULL << 32)) {
    fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds uint32 sel_t", (unsigned long long)n_rows);
    return 0;
  }
  return range_workspace_layout(filters, n_filters, n_rows, nullptr, nullptr);
}

int rpt_bf_probe_chain_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                uint32_t range_mask, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                                uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  if (range_mask == 0)
    return rpt_bf_probe_chain_ws(filters, cols, n_filters, row_sel, n, out_sel, out_count_dev, workspace,
                                 workspace_bytes, stream);
  if (!filters || !cols || !out_count_dev) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  const int st = check_range_args(filters, cols, n_filters, range_mask, nullptr, 0);
  if (st != RPT_OK) return st;
  const uint64_t* bits = nullptr;
  return probe_chain_range_impl(filters, cols, n_filters, range_mask, row_sel, n, out_sel, out_count_dev, workspace,
                                workspace_bytes, stream, &bits);
}

int rpt_bf_transfer_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                             uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                             uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                             uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  if (range_mask == 0)
    return rpt_bf_transfer_ws(filters, cols, n_filters, dst_filters, dst_cols, n_dst, row_sel, n, out_sel, out_count_dev,
                              workspace, workspace_bytes, stream);
  return transfer_range_impl(filters, cols, n_filters, range_mask, dst_filters, dst_cols, n_dst, row_sel, n, out_sel,
                             out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream);
}

int rpt_bf_transfer_insert_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                    uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                                    uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                                    uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                    void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream) {
  if (range_mask == 0)
    return rpt_bf_transfer_insert_ws(filters, cols, n_filters, dst_filters, dst_cols, n_dst, row_sel, n, out_sel,
                                     out_count_dev, workspace, workspace_bytes, insert_workspace, insert_workspace_bytes,
                                     stream);
  return transfer_range_impl(filters, cols, n_filters, range_mask, dst_filters, dst_cols, n_dst, row_sel, n, out_sel,
                             out_count_dev, workspace, workspace_bytes, true, insert_workspace, insert_workspace_bytes,
                             stream);
}
