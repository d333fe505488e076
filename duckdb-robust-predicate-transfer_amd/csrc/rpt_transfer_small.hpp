// rpt_transfer_small.hpp — the one-launch forward step and sink of one DuckDB-sized vector: rpt_bf_transfer,
// rpt_bf_transfer_range and rpt_bf_insert_multi, one launch of kernels/transfer_small.hpp each, no workspace. Host code
// of librpt_gpu.so, included by rpt_gpu.hip inside its extern "C" block, directly after rpt_probe_sel_range.hpp (the
// checks are those of rpt_chain_call.hpp, the write scopes those of rpt_probe_sel_small.hpp). Every kernel recorded
// here has a row in tests/kernel_ledger_transfer_small.py (tests/test_kernel_ledger_transfer_small_names.py scans this
// file).
#pragma once

namespace {

// The write half of a call, n > 0, the device current: every destination's capture check (and, for a transfer, every
// probed filter's pending clear) before anything is enqueued, has_data, the write scopes in ascending handle address
// held across the one launch. A call without probed filters (c.n_filters == 0) is the sink alone; every destination
// column reads through the call's row list.
int launch_transfer_small(const ChainCall& c, const rpt::RangeChainArgs& r, hipStream_t s) {
  rpt::DstArgs d{};
  for (uint32_t j = 0; j < c.n_dst; j++) {
    d.words[j] = c.dst_filters[j]->words;
    d.block_mask[j] = (1ULL << c.dst_filters[j]->log_num_blocks) - 1;
    d.a[j] = rpt::KeyArgs{c.dst_cols[j].keys, c.dst_cols[j].key_sel, c.dst_cols[j].validity, c.sel};
    d.key_type[j] = c.dst_cols[j].key_type;
    d.stats[j] = c.dst_filters[j]->stats;
  }
  d.n = c.n_dst;
  int st = refuse_captured_dsts(c, s);
  if (st != RPT_OK) return st;
  for (uint32_t f = 0; f < c.n_filters; f++) RPT_SETTLE(c.filters[f], s);
  for (uint32_t j = 0; j < c.n_dst; j++) c.dst_filters[j]->has_data.store(1);
  WriteOrders orders;
  st = take_write_orders(c, s, orders);
  if (st != RPT_OK) return st;
  auto launch = [&](auto ranged, auto probed) {
    return launch_kernel<rpt::transfer_small_kernel<ranged(), probed()>, ranged(), probed()>(
        "transfer_small_kernel", kRecorded, 1, rpt::kSmallThreads, 0, s, r, d, c.sel, c.n, c.out_sel, c.out_count_dev);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  st = c.n_filters == 0 ? launch(no, no) : c.range_mask != 0 ? launch(yes, yes) : launch(no, yes);
  for (uint32_t i = 0; i < orders.n; i++) orders[i].done(false);
  return st;
}

// The body of rpt_bf_transfer (range_mask == 0) and rpt_bf_transfer_range. Before any handle is looked into: the list
// checks of a transfer, the mask checks with every probed column, n against RPT_SMALL_PROBE_ROWS, and the overlap of
// out_sel with a given row_sel (pointer arithmetic only). Then probe_chain_range_small_impl's row-list order: the
// filters' devices, the destinations, n == 0 sets the count, a null out_sel, the capture refusals and the settles. No
// strategy and no workspace: every filter is gathered, every insert is one atomic OR per row.
int transfer_small_impl(const ChainCall& c) {
  int st = check_chain_lists(c);
  if (st != RPT_OK) return st;
  st = check_range_mask(c);  // every probed column too
  if (st != RPT_OK) return st;
  if (c.n > rpt::kSmallRows)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds RPT_SMALL_PROBE_ROWS", (unsigned long long)c.n);
  // the inserts read row_sel after the tail has begun to write out_sel
  if (c.n > 0 && c.sel && c.out_sel && sel_ranges_overlap(c.sel, c.out_sel, c.n))
    return fail(RPT_ERR_INVALID_ARGUMENT, "out_sel overlaps row_sel (%llu entries each)", (unsigned long long)c.n);
  st = check_chain_filters(c.filters, c.n_filters);
  if (st != RPT_OK) return st;
  rpt::RangeChainArgs r{};
  for (uint32_t f = 0; f < c.n_filters; f++) {
    r.c.words[f] = c.filters[f]->words;
    r.c.block_mask[f] = (1ULL << c.filters[f]->log_num_blocks) - 1;
    r.c.a[f] = rpt::KeyArgs{c.cols[f].keys, c.cols[f].key_sel, c.cols[f].validity, c.sel};
    r.c.key_type[f] = c.cols[f].key_type;
    r.stats[f] = c.filters[f]->stats;
  }
  r.c.k = c.n_filters;
  r.mask = c.range_mask;
  const int device = c.filters[0]->device;
  st = check_chain_dsts(c, device, nullptr);  // no destination routes here
  if (st != RPT_OK) return st;
  RPT_ON_DEVICE(device);
  hipStream_t s = as_stream(c.stream);
  if (c.n == 0) {  // nothing can be selected: no destination is touched
    RPT_HIP(hipMemsetAsync(c.out_count_dev, 0, sizeof(uint64_t), s));
    return RPT_OK;
  }
  if (!c.out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  return launch_transfer_small(c, r, s);
}
}  // namespace

int rpt_bf_transfer(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                    rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst, const uint32_t* row_sel,
                    uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev, rpt_stream_t stream) {
  return transfer_small_impl({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, false, row_sel, nullptr, n, 0,
                              out_sel, out_count_dev, nullptr, 0, false, nullptr, 0, stream});
}

// range_mask == 0: rpt_bf_transfer, whose kernel then runs.
int rpt_bf_transfer_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                          uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                          uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                          uint64_t* out_count_dev, rpt_stream_t stream) {
  if (range_mask == 0)
    return rpt_bf_transfer(filters, cols, n_filters, dst_filters, dst_cols, n_dst, row_sel, n, out_sel, out_count_dev, stream);
  return transfer_small_impl({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, false, row_sel, nullptr, n,
                              range_mask, out_sel, out_count_dev, nullptr, 0, false, nullptr, 0, stream});
}

// The sink alone: a transfer with no probed filter, in which every listed row survives.
int rpt_bf_insert_multi(rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                        const uint32_t* row_sel, uint64_t n, rpt_stream_t stream) {
  if (!dst_filters || !dst_cols) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n_dst == 0 || n_dst > RPT_MAX_CHAIN)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_dst=%u outside 1..%d", n_dst, RPT_MAX_CHAIN);
  for (uint32_t j = 0; j < n_dst; j++)
    if (!dst_filters[j]) return fail(RPT_ERR_INVALID_ARGUMENT, "null destination filter %u", j);
  if (n > rpt::kSmallRows)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds RPT_SMALL_PROBE_ROWS", (unsigned long long)n);
  const ChainCall c{nullptr, nullptr, 0, true, dst_filters, dst_cols, n_dst, false, row_sel, nullptr, n, 0,
                    nullptr, nullptr, nullptr, 0, false, nullptr, 0, stream};
  const int device = dst_filters[0]->device;
  const int st = check_chain_dsts(c, device, nullptr);
  if (st != RPT_OK || n == 0) return st;
  RPT_ON_DEVICE(device);
  return launch_transfer_small(c, rpt::RangeChainArgs{}, as_stream(stream));
}
