// rpt_probe_sel_small.hpp — the device-counted probes for small batches: rpt_bf_probe_chain_sel and
// rpt_bf_transfer_sel, one launch of kernels/probe_sel_small.hpp each, no workspace. Host code of librpt_gpu.so,
// included by rpt_gpu.hip inside its extern "C" block, directly after rpt_probe_sel.hpp (whose sel_ranges_overlap
// it reuses). Every kernel recorded here has a row in tests/kernel_ledger_sel_small.py
// (tests/test_kernel_ledger_sel_small_names.py scans this file).
#pragma once

namespace {

// The write scopes of one launch that writes several filters: one WriteOrder per distinct handle, all held until the
// launch is enqueued. The caller adds the handles in ascending address, so two threads that list the same filters in
// different orders take the order_mu locks in one order.
struct WriteOrders {
  alignas(WriteOrder) unsigned char mem[RPT_MAX_CHAIN][sizeof(WriteOrder)];
  uint32_t n = 0;
  WriteOrders() = default;
  WriteOrders(const WriteOrders&) = delete;
  WriteOrders& operator=(const WriteOrders&) = delete;
  WriteOrder& operator[](uint32_t i) { return *reinterpret_cast<WriteOrder*>(mem[i]); }
  void add(rpt_bf* bf, hipStream_t s) {
    new (mem[n]) WriteOrder(bf, s);
    n++;
  }
  ~WriteOrders() {
    while (n > 0) (*this)[--n].~WriteOrder();  // released in reverse order
  }
};

// The body of both entry points. The checks run in probe_chain_sel_impl's order (rpt_probe_sel.hpp), with its
// messages: everything that needs no look into a handle first; max_rows == 0 then sets the count and returns; then
// the handles are looked into.
int probe_chain_sel_small_impl(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                               rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst, bool transfer,
                               const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                               uint64_t* out_count_dev, rpt_stream_t stream) {
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
  if (max_rows > rpt::kSmallRows)
    return fail(RPT_ERR_INVALID_ARGUMENT, "max_rows=%llu rows exceeds RPT_SMALL_PROBE_ROWS", (unsigned long long)max_rows);
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
  rpt::ChainArgs c{};
  for (uint32_t f = 0; f < n_filters; f++) {
    st = check_col(&cols[f]);
    if (st != RPT_OK) return st;
    c.words[f] = filters[f]->words;
    c.block_mask[f] = (1ULL << filters[f]->log_num_blocks) - 1;
    c.a[f] = rpt::KeyArgs{cols[f].keys, cols[f].key_sel, cols[f].validity, sel};
    c.key_type[f] = cols[f].key_type;
  }
  c.k = n_filters;
  const int device = filters[0]->device;
  rpt::DstArgs d{};
  for (uint32_t j = 0; j < n_dst; j++) {
    if (dst_filters[j]->device != device)
      return fail(RPT_ERR_INVALID_ARGUMENT, "destination filter %u is not on the chain's device", j);
    st = check_col(&dst_cols[j]);
    if (st != RPT_OK) return st;
    d.words[j] = dst_filters[j]->words;
    d.block_mask[j] = (1ULL << dst_filters[j]->log_num_blocks) - 1;
    d.a[j] = rpt::KeyArgs{dst_cols[j].keys, dst_cols[j].key_sel, dst_cols[j].validity, sel};
    d.key_type[j] = dst_cols[j].key_type;
    d.stats[j] = dst_filters[j]->stats;
  }
  d.n = n_dst;
  RPT_ON_DEVICE(device);
  // every destination's capture check and every probed filter's pending clear before anything is enqueued
  for (uint32_t j = 0; j < n_dst; j++) RPT_REFUSE_CAPTURE_WRITE(dst_filters[j], s, "transfer");
  for (uint32_t f = 0; f < n_filters; f++) RPT_SETTLE(filters[f], s);
  // has_data becomes 1 whatever the device-side selection holds: the host cannot know it was empty
  for (uint32_t j = 0; j < n_dst; j++) dst_filters[j]->has_data.store(1);
  // one write scope per distinct destination (a filter listed twice is locked, waited for and recorded once), taken
  // in ascending handle address and held across the launch
  rpt_bf* distinct[RPT_MAX_CHAIN];
  uint32_t n_distinct = 0;
  for (uint32_t j = 0; j < n_dst; j++)
    if (std::find(distinct, distinct + n_distinct, dst_filters[j]) == distinct + n_distinct)
      distinct[n_distinct++] = dst_filters[j];
  std::sort(distinct, distinct + n_distinct, [](const rpt_bf* x, const rpt_bf* y) {
    return reinterpret_cast<uintptr_t>(x) < reinterpret_cast<uintptr_t>(y);
  });
  WriteOrders orders;
  for (uint32_t i = 0; i < n_distinct; i++) orders.add(distinct[i], s);
  for (uint32_t i = 0; i < n_distinct; i++) RPT_REFUSE_IN_FLIGHT(orders[i], "write");
  for (uint32_t i = 0; i < n_distinct; i++) {
    const hipError_t ez = zero_pending_locked(distinct[i], s);
    if (ez != hipSuccess) return fail(RPT_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(ez));
  }
  if (transfer) {
    ProfScope prof(inst_name<true>("probe_chain_sel_small_kernel"), s);
    hipLaunchKernelGGL(rpt::probe_chain_sel_small_kernel<true>, dim3(1), dim3(rpt::kSmallThreads), 0, s, c, d, sel,
                       count_dev, max_rows, out_sel, out_count_dev);
    prof.end();
  } else {
    ProfScope prof(inst_name<false>("probe_chain_sel_small_kernel"), s);
    hipLaunchKernelGGL(rpt::probe_chain_sel_small_kernel<false>, dim3(1), dim3(rpt::kSmallThreads), 0, s, c, d, sel,
                       count_dev, max_rows, out_sel, out_count_dev);
    prof.end();
  }
  for (uint32_t i = 0; i < n_distinct; i++) orders[i].done(false);
  RPT_LAUNCHED("probe_chain_sel_small_kernel");
  return RPT_OK;
}
}  // namespace

int rpt_bf_probe_chain_sel(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                           const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                           uint64_t* out_count_dev, rpt_stream_t stream) {
  return probe_chain_sel_small_impl(filters, cols, n_filters, nullptr, nullptr, 0, false, sel, count_dev, max_rows,
                                    out_sel, out_count_dev, stream);
}

int rpt_bf_transfer_sel(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                        rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst, const uint32_t* sel,
                        const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel, uint64_t* out_count_dev,
                        rpt_stream_t stream) {
  return probe_chain_sel_small_impl(filters, cols, n_filters, dst_filters, dst_cols, n_dst, true, sel, count_dev,
                                    max_rows, out_sel, out_count_dev, stream);
}
