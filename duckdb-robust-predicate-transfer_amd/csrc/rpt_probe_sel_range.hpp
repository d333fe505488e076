// rpt_probe_sel_range.hpp — a filter's min/max range in the device-counted probes and in the one-launch chains
// (kernels/probe_sel_range.hpp): rpt_bf_probe_chain_sel_range_ws, rpt_bf_transfer_sel_range_ws and
// rpt_bf_transfer_insert_sel_range_ws (run_chain_call of rpt_chain_call.hpp is their body; their stage 0 is launched
// here), and the one-launch rpt_bf_probe_chain_range, rpt_bf_probe_chain_sel_range and rpt_bf_transfer_sel_range. Host
// code of librpt_gpu.so, included by rpt_gpu.hip inside its extern "C" block, directly after rpt_probe_range.hpp. Every
// kernel recorded here has a row in tests/kernel_ledger_sel_range.py (tests/test_kernel_ledger_sel_range_names.py scans
// this file).
#pragma once

namespace {

// Stage 0 of a ranged device-counted call: the first flagged column's range stage over sel[0 .. min(*count_dev,
// max_rows)), the only kernel of the call that reads *count_dev; it writes every segment's words and count. The other
// flagged columns AND into them as masked range stages over all max_rows positions (the zero bits past the count keep
// them away from sel); every filter, filter 0 included, then runs as a later stage of the chain.
int enqueue_sel_range_stages(const ChainCall& c, const ChainWorkspace& ws, hipStream_t s) {
  bool first = true;
  for (uint32_t f = 0; f < c.n_filters; f++) {
    if (!((c.range_mask >> f) & 1u)) continue;
    const rpt_bf* bf = c.filters[f];
    const rpt_key_column& col = c.cols[f];
    if (!first) {
      const int st = enqueue_range_stage(bf, &col, c.sel, c.n, true, ws.bits, ws.seg_counts, s);
      if (st != RPT_OK) return st;
      continue;
    }
    first = false;
    const uint64_t n_segs = ceil_div(c.n, rpt::kSegRows);
    const unsigned grid = persistent_grid(bf->device, n_segs);
    const rpt::KeyArgs a{col.keys, col.key_sel, col.validity, c.sel};
    auto launch = [&](auto k) {
      return launch_kernel<rpt::range_bits_sel_kernel<k()>, k()>("range_bits_sel_kernel", kRecorded, grid, rpt::kBlockThreads, 0,
                                                                 s, bf->stats, a, c.count_dev, c.n, n_segs, ws.bits,
                                                                 ws.seg_counts);
    };
    // I64 or I32: check_range_mask has refused a flagged HASH column
    RPT_TRY(col.key_type == RPT_KEY_I64 ? launch(int_c<rpt::kKeyI64>{}) : launch(int_c<rpt::kKeyI32>{}));
  }
  return RPT_OK;
}

// The body of the three one-launch range calls (range_mask != 0). Device-counted: the checks of
// probe_chain_sel_small_impl, in its order and with its messages, and the mask checks with those that need no look into
// a handle, before max_rows == 0 sets the count and returns. Row list: the same lists and mask checks, n against
// RPT_SMALL_PROBE_ROWS, the filters' devices; n == 0 then sets the count, and a null out_sel is refused. No strategy and
// no workspace: every filter is gathered.
int probe_chain_range_small_impl(const ChainCall& c) {
  int st = check_chain_lists(c);
  if (st != RPT_OK) return st;
  st = check_range_mask(c);  // every probed column too
  if (st != RPT_OK) return st;
  if (c.counted) {
    st = check_counted_rows(c, rpt::kSmallRows, "RPT_SMALL_PROBE_ROWS");
    if (st != RPT_OK || c.n == 0) return st;
  } else if (c.n > rpt::kSmallRows) {
    return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds RPT_SMALL_PROBE_ROWS", (unsigned long long)c.n);
  }
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
  if (!c.counted) {
    if (c.n == 0) {
      RPT_HIP(hipMemsetAsync(c.out_count_dev, 0, sizeof(uint64_t), s));
      return RPT_OK;
    }
    if (!c.out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  }
  // every destination's capture check and every probed filter's pending clear before anything is enqueued
  st = refuse_captured_dsts(c, s);
  if (st != RPT_OK) return st;
  for (uint32_t f = 0; f < c.n_filters; f++) RPT_SETTLE(c.filters[f], s);
  // has_data becomes 1 whatever the device-side selection holds: the host cannot know it was empty
  for (uint32_t j = 0; j < c.n_dst; j++) c.dst_filters[j]->has_data.store(1);
  WriteOrders orders;
  st = take_write_orders(c, s, orders);
  if (st != RPT_OK) return st;
  auto launch = [&](auto counted, auto transfer) {
    return launch_kernel<rpt::probe_chain_range_small_kernel<counted(), transfer()>, counted(), transfer()>(
        "probe_chain_range_small_kernel", kRecorded, 1, rpt::kSmallThreads, 0, s, r, d, c.sel, c.count_dev, c.n, c.out_sel,
        c.out_count_dev);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  st = c.transfer ? launch(yes, yes) : c.counted ? launch(yes, no) : launch(no, no);
  for (uint32_t i = 0; i < orders.n; i++) orders[i].done(false);
  return st;
}
}  // namespace

// range_mask == 0: each call hands over to its twin without the argument, whose kernels then run.
int rpt_bf_probe_chain_sel_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                    uint32_t range_mask, const uint32_t* sel, const uint64_t* count_dev,
                                    uint64_t max_rows, uint32_t* out_sel, uint64_t* out_count_dev, void* workspace,
                                    size_t workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, false, nullptr, nullptr, 0, true, sel, count_dev, max_rows, range_mask,
                         out_sel, out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream});
}

int rpt_bf_transfer_sel_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                 uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                                 uint32_t n_dst, const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows,
                                 uint32_t* out_sel, uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                 rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, true, sel, count_dev, max_rows,
                         range_mask, out_sel, out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream});
}

int rpt_bf_transfer_insert_sel_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                        uint32_t range_mask, rpt_bf* const* dst_filters,
                                        const rpt_key_column* dst_cols, uint32_t n_dst, const uint32_t* sel,
                                        const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                                        uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                        void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, true, sel, count_dev, max_rows,
                         range_mask, out_sel, out_count_dev, workspace, workspace_bytes, true, insert_workspace,
                         insert_workspace_bytes, stream});
}

int rpt_bf_probe_chain_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                             uint32_t range_mask, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                             uint64_t* out_count_dev, rpt_stream_t stream) {
  if (range_mask == 0) return rpt_bf_probe_chain(filters, cols, n_filters, row_sel, n, out_sel, out_count_dev, stream);
  return probe_chain_range_small_impl({filters, cols, n_filters, false, nullptr, nullptr, 0, false, row_sel, nullptr, n,
                                       range_mask, out_sel, out_count_dev, nullptr, 0, false, nullptr, 0, stream});
}

int rpt_bf_probe_chain_sel_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                 uint32_t range_mask, const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows,
                                 uint32_t* out_sel, uint64_t* out_count_dev, rpt_stream_t stream) {
  if (range_mask == 0)
    return rpt_bf_probe_chain_sel(filters, cols, n_filters, sel, count_dev, max_rows, out_sel, out_count_dev, stream);
  return probe_chain_range_small_impl({filters, cols, n_filters, false, nullptr, nullptr, 0, true, sel, count_dev,
                                       max_rows, range_mask, out_sel, out_count_dev, nullptr, 0, false, nullptr, 0,
                                       stream});
}

int rpt_bf_transfer_sel_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                              uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                              uint32_t n_dst, const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows,
                              uint32_t* out_sel, uint64_t* out_count_dev, rpt_stream_t stream) {
  if (range_mask == 0)
    return rpt_bf_transfer_sel(filters, cols, n_filters, dst_filters, dst_cols, n_dst, sel, count_dev, max_rows, out_sel,
                               out_count_dev, stream);
  return probe_chain_range_small_impl({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, true, sel, count_dev,
                                       max_rows, range_mask, out_sel, out_count_dev, nullptr, 0, false, nullptr, 0,
                                       stream});
}
