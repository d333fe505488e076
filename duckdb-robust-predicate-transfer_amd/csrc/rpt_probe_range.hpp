// rpt_probe_range.hpp — the min/max range stage (kernels/range.hpp): rpt_bf_range_bits, and the workspace chain and
// transfers that apply a filter's range on the device before its Bloom test (rpt_bf_probe_chain_range_ws,
// rpt_bf_transfer_range_ws, rpt_bf_transfer_insert_range_ws). Host code of librpt_gpu.so, included by rpt_gpu.hip
// inside its extern "C" block, directly after rpt_probe_sel_small.hpp. Every kernel recorded here has a row in
// tests/kernel_ledger_range.py (tests/test_kernel_ledger_range_names.py scans this file).
#pragma once

namespace {

// The range test of one column (I64 or I32: the caller has refused HASH) over n rows. masked: AND into the accumulated
// bits / counts in place; else write every segment's words (and its count where counts != nullptr).
int enqueue_range_stage(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n, bool masked,
                        uint64_t* bits, uint32_t* counts, hipStream_t s) {
  const uint64_t n_segs = ceil_div(n, rpt::kSegRows);
  const unsigned grid = persistent_grid(bf->device, n_segs);
  const rpt::KeyArgs a{col->keys, col->key_sel, col->validity, row_sel};
  return dispatch_kd(col->key_type, dense_ok(col, row_sel), [&](auto k, auto d) {
    if constexpr (!rpt::KeyTraits<k()>::kValues) {
      return fail(RPT_ERR_INVALID_ARGUMENT, "range test of a column that holds hashes (no key values)");  // callers refuse it
    } else {
      return dispatch_bool(masked, [&](auto m) {
        return launch_kernel<rpt::range_bits_kernel<k(), d(), m()>, k(), d(), m()>(
            "range_bits_kernel", kRecorded, grid, rpt::kBlockThreads, 0, s, bf->stats, a, n, n_segs, bits, counts);
      });
    }
  });
}

// What a range call (range_mask != 0) checks after its lists and before any handle is looked into: the mask, every
// probed column, and that no flagged column holds hashes.
int check_range_mask(const ChainCall& c) {
  if ((c.range_mask >> c.n_filters) != 0)  // n_filters <= RPT_MAX_CHAIN < 32
    return fail(RPT_ERR_INVALID_ARGUMENT, "range_mask=0x%x flags a filter at or above n_filters=%u", c.range_mask,
                c.n_filters);
  for (uint32_t f = 0; f < c.n_filters; f++) {
    const int st = check_col(&c.cols[f]);
    if (st != RPT_OK) return st;
    if (((c.range_mask >> f) & 1u) && c.cols[f].key_type == RPT_KEY_HASH)
      return fail(RPT_ERR_INVALID_ARGUMENT, "range_mask flags filter %u, whose column holds hashes (no key values)", f);
  }
  return RPT_OK;
}

// Stage 0 of a range call: the flagged columns' range stages, in filter order. The first writes the accumulated bits and
// counts, the others AND into them; every filter, filter 0 included, then runs as a later stage of the chain.
int enqueue_range_stages(const ChainCall& c, const ChainWorkspace& ws, hipStream_t s) {
  bool first = true;
  for (uint32_t f = 0; f < c.n_filters; f++) {
    if (!((c.range_mask >> f) & 1u)) continue;
    const int st = enqueue_range_stage(c.filters[f], &c.cols[f], c.sel, c.n, !first, ws.bits, ws.seg_counts, s);
    if (st != RPT_OK) return st;
    first = false;
  }
  return RPT_OK;
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
  // the temporary bits are present whenever any filter routes, filter 0 included: it runs as a later stage here
  return chain_workspace_layout(filters, n_filters, n_rows, 0, true, nullptr, nullptr);
}

// range_mask == 0 is exactly the plain twin, hand-over for small batches included.
int rpt_bf_probe_chain_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                uint32_t range_mask, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                                uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, false, nullptr, nullptr, 0, false, row_sel, nullptr, n, range_mask,
                         out_sel, out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream});
}

int rpt_bf_transfer_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                             uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                             uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                             uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, false, row_sel, nullptr, n,
                         range_mask, out_sel, out_count_dev, workspace, workspace_bytes, false, nullptr, 0, stream});
}

int rpt_bf_transfer_insert_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                    uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                                    uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                                    uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                    void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream) {
  return run_chain_call({filters, cols, n_filters, true, dst_filters, dst_cols, n_dst, false, row_sel, nullptr, n,
                         range_mask, out_sel, out_count_dev, workspace, workspace_bytes, true, insert_workspace,
                         insert_workspace_bytes, stream});
}
