// rpt_probe_sel_small.hpp — the device-counted probes for small batches: rpt_bf_probe_chain_sel and
// rpt_bf_transfer_sel, one launch of kernels/probe_sel_small.hpp each, no workspace. Host code of librpt_gpu.so,
// included by rpt_gpu.hip inside its extern "C" block, directly after rpt_probe_sel.hpp (the checks are those of
// rpt_chain_call.hpp). Every kernel recorded here has a row in tests/kernel_ledger_sel_small.py
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

// One write scope per distinct destination of a one-launch transfer (a filter listed twice is locked, waited for and
// recorded once), taken in ascending handle address and held by `orders` across the launch; an earlier write in flight
// is refused inside a capture and every destination's pending clear is enqueued. A chain has none.
int take_write_orders(const ChainCall& c, hipStream_t s, WriteOrders& orders) {
  rpt_bf* distinct[RPT_MAX_CHAIN];
  uint32_t n_distinct = 0;
  for (uint32_t j = 0; j < c.n_dst; j++)
    if (std::find(distinct, distinct + n_distinct, c.dst_filters[j]) == distinct + n_distinct)
      distinct[n_distinct++] = c.dst_filters[j];
  std::sort(distinct, distinct + n_distinct, [](const rpt_bf* x, const rpt_bf* y) {
    return reinterpret_cast<uintptr_t>(x) < reinterpret_cast<uintptr_t>(y);
  });
  for (uint32_t i = 0; i < n_distinct; i++) orders.add(distinct[i], s);
  for (uint32_t i = 0; i < n_distinct; i++) RPT_REFUSE_IN_FLIGHT(orders[i], "write");
  for (uint32_t i = 0; i < n_distinct; i++) {
    const hipError_t ez = zero_pending_locked(distinct[i], s);
    if (ez != hipSuccess) return fail(RPT_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(ez));
  }
  return RPT_OK;
}

// The body of both entry points. The checks are run_chain_call's for a device-counted call (rpt_chain_call.hpp), in
// its order and with its messages: everything that needs no look into a handle first; max_rows == 0 then sets the
// count and returns; then the handles are looked into. No strategy and no workspace: every filter is gathered.
int probe_chain_sel_small_impl(const ChainCall& c) {
  int st = check_chain_lists(c);
  if (st != RPT_OK) return st;
  st = check_counted_rows(c, rpt::kSmallRows, "RPT_SMALL_PROBE_ROWS");
  if (st != RPT_OK || c.n == 0) return st;
  st = check_chain_filters(c.filters, c.n_filters);
  if (st != RPT_OK) return st;
  rpt::ChainArgs a{};
  for (uint32_t f = 0; f < c.n_filters; f++) {
    st = check_col(&c.cols[f]);
    if (st != RPT_OK) return st;
    a.words[f] = c.filters[f]->words;
    a.block_mask[f] = (1ULL << c.filters[f]->log_num_blocks) - 1;
    a.a[f] = rpt::KeyArgs{c.cols[f].keys, c.cols[f].key_sel, c.cols[f].validity, c.sel};
    a.key_type[f] = c.cols[f].key_type;
  }
  a.k = c.n_filters;
  const int device = c.filters[0]->device;
  st = check_chain_dsts(c, device, nullptr);  // no destination routes here
  if (st != RPT_OK) return st;
  rpt::DstArgs d{};
  for (uint32_t j = 0; j < c.n_dst; j++) {
    d.words[j] = c.dst_filters[j]->words;
    d.block_mask[j] = (1ULL << c.dst_filters[j]->log_num_blocks) - 1;
    d.a[j] = rpt::KeyArgs{c.dst_cols[j].keys, c.dst_cols[j].key_sel, c.dst_cols[j].validity, c.sel};
    d.key_type[j] = c.dst_cols[j].key_type;
    d.stats[j] = c.dst_filters[j]->stats;
  }
  d.n = c.n_dst;
  RPT_ON_DEVICE(device);
  hipStream_t s = as_stream(c.stream);
  // every destination's capture check and every probed filter's pending clear before anything is enqueued
  st = refuse_captured_dsts(c, s);
  if (st != RPT_OK) return st;
  for (uint32_t f = 0; f < c.n_filters; f++) RPT_SETTLE(c.filters[f], s);
  // has_data becomes 1 whatever the device-side selection holds: the host cannot know it was empty
  for (uint32_t j = 0; j < c.n_dst; j++) c.dst_filters[j]->has_data.store(1);
  WriteOrders orders;
  st = take_write_orders(c, s, orders);
  if (st != RPT_OK) return st;
  st = dispatch_bool(c.transfer, [&](auto transfer) {
    return launch_kernel<rpt::probe_chain_sel_small_kernel<transfer()>, transfer()>(
        "probe_chain_sel_small_kernel", kRecorded, 1, rpt::kSmallThreads, 0, s, a, d, c.sel, c.count_dev, c.n, c.out_sel,
        c.out_count_dev);
  });
  for (uint32_t i = 0; i < orders.n; i++) orders[i].done(false);
  return st;
}
}  // namespace

int rpt_bf_probe_chain_sel(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                           const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                           uint64_t* out_count_dev, rpt_stream_t stream) {
  return probe_chain_sel_small_impl({filters, cols, n_filters, false, nullptr, nullptr, 0, true, sel, count_dev, max_rows,
                                     0, out_sel, out_count_dev, nullptr, 0, false, nullptr, 0, stream});
}

int rpt_bf_transfer_sel(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                        rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst, const uint32_t* sel,
                        const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel, uint64_t* out_count_dev,
                        rpt_stream_t stream) {
  return probe_chain_sel_small_impl({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, true, sel, count_dev,
                                     max_rows, 0, out_sel, out_count_dev, nullptr, 0, false, nullptr, 0, stream});
}
