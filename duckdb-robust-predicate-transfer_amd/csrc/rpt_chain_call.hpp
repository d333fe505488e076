// rpt_chain_call.hpp — one description and one checked path for the chain and transfer entry points: the plain ones
// (rpt_bf_probe_chain_ws, rpt_bf_transfer_ws, rpt_bf_transfer_insert_ws), their device-counted twins (_sel_ws; the
// one-launch rpt_bf_probe_chain_sel / rpt_bf_transfer_sel take the checks from here and launch on their own) and their
// range twins (_range_ws, _sel_range_ws; the one-launch range calls take the checks from here too). Host code of
// librpt_gpu.so, included by rpt_gpu.hip inside its extern "C" block, after
// chain_workspace_layout, enqueue_chain_later_stages, launch_sel_tail, check_routed_insert and
// enqueue_transfer_inserts, and before the four headers that hold the device-counted and range stages. It launches no
// kernel itself: every launch stays in the file whose ledger records it.
#pragma once

namespace {

// One call of the family. The entry points fill it in this order and change nothing afterwards.
struct ChainCall {
  const rpt_bf* const* filters;  // the probed filters and their key columns
  const rpt_key_column* cols;
  uint32_t n_filters;
  bool transfer;  // the call has destination lists (n_dst == 0 is then a fault); false: a chain, n_dst == 0
  rpt_bf* const* dst_filters;
  const rpt_key_column* dst_cols;
  uint32_t n_dst;
  // the row source. counted false: rows 0..n-1, or sel[0..n) (the row_sel of the C-ABI). counted true: rows
  // sel[0 .. min(*count_dev, n)), n being the C-ABI's max_rows
  bool counted;
  const uint32_t* sel;
  const uint64_t* count_dev;
  uint64_t n;
  uint32_t range_mask;  // bit f: filters[f]'s min/max range is applied before its Bloom test; 0: the plain call
  uint32_t* out_sel;
  uint64_t* out_count_dev;
  void* workspace;
  size_t workspace_bytes;
  bool route;  // a destination whose insert strategy resolves to PARTITIONED takes the routed insert
  void* insert_workspace;
  size_t insert_workspace_bytes;
  rpt_stream_t stream;
};

// the stage-0 kinds that live beside their kernels' launchers
int enqueue_sel_stage0(const ChainCall& c, int strategy, int device, const ChainWorkspace& ws, hipStream_t s);  // rpt_probe_sel.hpp
int check_range_mask(const ChainCall& c);                                                       // rpt_probe_range.hpp
int enqueue_range_stages(const ChainCall& c, const ChainWorkspace& ws, hipStream_t s);         // rpt_probe_range.hpp
int enqueue_sel_range_stages(const ChainCall& c, const ChainWorkspace& ws, hipStream_t s);     // rpt_probe_sel_range.hpp

// The list checks, none of which looks into a handle: null lists, the counts, null handles, and a destination that is
// also probed. The plain chain has no handles to compare: it leaves them to check_chain_filters, which looks at them
// filter by filter.
int check_chain_lists(const ChainCall& c) {
  if (!c.filters || !c.cols || !c.out_count_dev || (c.transfer && (!c.dst_filters || !c.dst_cols)))
    return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (c.n_filters == 0 || c.n_filters > RPT_MAX_CHAIN)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_filters=%u outside 1..%d", c.n_filters, RPT_MAX_CHAIN);
  if (c.transfer && (c.n_dst == 0 || c.n_dst > RPT_MAX_CHAIN))
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_dst=%u outside 1..%d", c.n_dst, RPT_MAX_CHAIN);
  if (!c.transfer && !c.counted && c.range_mask == 0) return RPT_OK;
  // handles are compared before any of them is looked into
  for (uint32_t f = 0; f < c.n_filters; f++)
    if (!c.filters[f]) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter %u", f);
  for (uint32_t j = 0; j < c.n_dst; j++) {
    if (!c.dst_filters[j]) return fail(RPT_ERR_INVALID_ARGUMENT, "null destination filter %u", j);
    for (uint32_t f = 0; f < c.n_filters; f++)
      if (c.dst_filters[j] == c.filters[f])
        return fail(RPT_ERR_INVALID_ARGUMENT, "destination filter %u is probed filter %u of the same call", j, f);
  }
  return RPT_OK;
}

// Do the max_rows-entry ranges at sel and out_sel share a byte?
bool sel_ranges_overlap(const uint32_t* sel, const uint32_t* out_sel, uint64_t max_rows) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(sel), b = reinterpret_cast<uintptr_t>(out_sel);
  const uintptr_t bytes = static_cast<uintptr_t>(max_rows) * sizeof(uint32_t);
  return a < b + bytes && b < a + bytes;
}

// The row source of a device-counted call, still before any handle is looked into: count_dev, max_rows against `most`
// (named `bound` in the message), and with max_rows > 0 sel, out_sel and their overlap. max_rows == 0: nothing can be
// selected, so the count is set, stream-ordered on the current device, and the caller returns (it tests c.n == 0).
int check_counted_rows(const ChainCall& c, uint64_t most, const char* bound) {
  if (!c.count_dev) return fail(RPT_ERR_INVALID_ARGUMENT, "null count_dev");
  if (c.n > most)
    return fail(RPT_ERR_INVALID_ARGUMENT, "max_rows=%llu rows exceeds %s", (unsigned long long)c.n, bound);
  if (c.n == 0) {
    RPT_HIP(hipMemsetAsync(c.out_count_dev, 0, sizeof(uint64_t), as_stream(c.stream)));
    return RPT_OK;
  }
  if (!c.sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null sel");
  if (!c.out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  if (sel_ranges_overlap(c.sel, c.out_sel, c.n))
    return fail(RPT_ERR_INVALID_ARGUMENT, "out_sel overlaps sel (%llu entries each)", (unsigned long long)c.n);
  return RPT_OK;
}

// The destinations: on the chain's device, their columns, and under c.route which of them route (dst_routed[j]) and
// whether the insert workspace they share (they run one after another on the stream) serves them.
int check_chain_dsts(const ChainCall& c, int device, bool* dst_routed) {
  for (uint32_t j = 0; j < c.n_dst; j++) {
    if (c.dst_filters[j]->device != device)
      return fail(RPT_ERR_INVALID_ARGUMENT, "destination filter %u is not on the chain's device", j);
    const int st = check_col(&c.dst_cols[j]);
    if (st != RPT_OK) return st;
  }
  if (c.route && c.n > 0)
    for (uint32_t j = 0; j < c.n_dst; j++) {
      const int st = check_routed_insert(c.dst_filters[j], c.n, c.insert_workspace, c.insert_workspace_bytes, &dst_routed[j]);
      if (st != RPT_OK) return st;
    }
  return RPT_OK;
}

// Every destination's capture and in-flight check; the callers run it before anything is enqueued.
int refuse_captured_dsts(const ChainCall& c, hipStream_t s) {
  for (uint32_t j = 0; j < c.n_dst; j++) RPT_REFUSE_CAPTURE_WRITE(c.dst_filters[j], s, "transfer");
  return RPT_OK;
}

// A filter's strategy in a device-counted chain: a routed stage would partition all max_rows positions and read every
// sel entry, so PARTITIONED and BUCKETED (resolved by AUTO or forced) become GATHER, whose masked form does no work
// past the count. LDS, whole-filter or hybrid, stays.
int sel_strategy(const rpt_bf* bf, uint64_t max_rows) {
  const int st = resolve_strategy(bf->probe_strategy.load(), bf->log_num_blocks, max_rows);
  return routed(st) ? RPT_PROBE_GATHER : st;
}

// Every probed column, and its filter's strategy for the call's row source. *all_auto: no filter has one forced.
int resolve_chain_strategies(const ChainCall& c, int* strategy, bool* all_auto) {
  *all_auto = true;
  for (uint32_t f = 0; f < c.n_filters; f++) {
    const int st = check_col(&c.cols[f]);
    if (st != RPT_OK) return st;
    const int L = c.filters[f]->log_num_blocks, requested = c.filters[f]->probe_strategy.load();
    *all_auto = *all_auto && requested == RPT_PROBE_AUTO;
    strategy[f] = c.counted ? sel_strategy(c.filters[f], c.n) : resolve_strategy(requested, L, c.n);
    if (!strategy_supported(strategy[f], L))
      return fail(RPT_ERR_INVALID_ARGUMENT, "probe strategy %d unsupported for a 2^%d-block filter (filter %u)", strategy[f],
                  L, f);
  }
  return RPT_OK;
}

// The call's workspace: no stage area for a device-counted chain (no stage routes); after range stages filter 0 runs
// as a later stage.
size_t chain_call_layout(const ChainCall& c, void* base, ChainWorkspace* ws) {
  return chain_workspace_layout(c.filters, c.n_filters, c.n, c.range_mask != 0 ? 0 : 1, !c.counted, base, ws);
}

// The body of the twelve workspace calls: the checks in the family's documented order (the row-list calls, plain and
// range, check the destinations and refuse a captured write before they look at the probed columns, and reach the
// workspace last; the device-counted calls, plain and range, check everything that needs no handle first, the mask
// among it, then the probed columns, the destinations and the workspace, and only then make the device current), then
// stage 0, the later stages, the tail
// and the inserts. Every probed filter is settled and every destination's capture check made before anything is
// enqueued. n == 0 / max_rows == 0 sets the count and touches nothing else.
int run_chain_call(const ChainCall& c) {
  int st = check_chain_lists(c);
  if (st != RPT_OK) return st;
  if (c.range_mask != 0) {  // looks into no handle: before the device-counted calls' max_rows == 0 return
    st = check_range_mask(c);
    if (st != RPT_OK) return st;
  }
  if (c.counted) {
    st = check_counted_rows(c, 0xFFFFFFFFull, "uint32 sel_t");
    if (st != RPT_OK || c.n == 0) return st;
  }
  st = check_chain_filters(c.filters, c.n_filters);
  if (st != RPT_OK) return st;
  if (!c.counted && c.n >= (1ULL << 32))
    return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds uint32 sel_t", (unsigned long long)c.n);
  const int device = c.filters[0]->device;
  int strategy[RPT_MAX_CHAIN];
  bool all_auto = false, dst_routed[RPT_MAX_CHAIN] = {};
  if (c.counted) {
    st = resolve_chain_strategies(c, strategy, &all_auto);
    if (st != RPT_OK) return st;
  }
  st = check_chain_dsts(c, device, dst_routed);
  if (st != RPT_OK) return st;
  if (c.counted) {
    st = check_workspace(c.workspace, c.workspace_bytes, chain_call_layout(c, nullptr, nullptr));
    if (st != RPT_OK) return st;
  }
  RPT_ON_DEVICE(device);
  hipStream_t s = as_stream(c.stream);
  if (c.n > 0) {
    st = refuse_captured_dsts(c, s);
    if (st != RPT_OK) return st;
  }
  if (!c.counted) {
    st = resolve_chain_strategies(c, strategy, &all_auto);
    if (st != RPT_OK) return st;
    if (c.n == 0) {
      RPT_HIP(hipMemsetAsync(c.out_count_dev, 0, sizeof(uint64_t), s));
      return RPT_OK;
    }
    if (!c.out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
    st = check_workspace(c.workspace, c.workspace_bytes, chain_call_layout(c, nullptr, nullptr));
    if (st != RPT_OK) return st;
    // a DuckDB-sized batch with nothing forced and no range stage: the one-launch chain kernel (the workspace stays
    // untouched); the inserts then read out_sel / the count, which hold the same row ids as the bits would
    if (c.range_mask == 0 && c.n <= rpt::kSmallRows && all_auto) {
      st = rpt_bf_probe_chain(c.filters, c.cols, c.n_filters, c.sel, c.n, c.out_sel, c.out_count_dev, c.stream);
      if (st != RPT_OK || c.n_dst == 0) return st;
      return enqueue_transfer_inserts(c.dst_filters, c.dst_cols, c.n_dst, dst_routed, nullptr, c.sel, c.out_sel,
                                      c.out_count_dev, c.n, c.insert_workspace, s);
    }
  }
  for (uint32_t f = 0; f < c.n_filters; f++) RPT_SETTLE(c.filters[f], s);
  ChainWorkspace ws;
  chain_call_layout(c, c.workspace, &ws);
  // stage 0 writes every segment's words and count: the only kernel that reads *count_dev (filter 0's probe, or with a
  // mask the first flagged column's range stage, the other flagged columns' following it); or the flagged columns' range
  // stages, after which filter 0 is a later stage too; or the filter's own phase 1 (the PARTITIONED one ending in result
  // bits)
  uint32_t first_later = 1;
  if (c.counted && c.range_mask != 0) {
    st = enqueue_sel_range_stages(c, ws, s);
    first_later = 0;
  } else if (c.counted) {
    st = enqueue_sel_stage0(c, strategy[0], device, ws, s);
  } else if (c.range_mask != 0) {
    st = enqueue_range_stages(c, ws, s);
    first_later = 0;
  } else {
    bool done = false;
    st = probe_phase1_impl(c.filters[0], &c.cols[0], c.sel, c.n, ws.stage, ws.stage_bytes, c.stream, nullptr, nullptr, &done,
                           ws.bits, ws.seg_counts);
  }
  if (st != RPT_OK) return st;
  // the later stages over all n positions (device-counted: the zero bits past the count keep the masked probes away
  // from sel), then the tail, once
  st = enqueue_chain_later_stages(c.filters, c.cols, c.n_filters, strategy, c.sel, c.n, ws, device, c.stream, first_later);
  if (st != RPT_OK) return st;
  st = launch_sel_tail(s, ws.bits, ws.seg_counts, ws.group_sums, ws.group_offs, ceil_div(c.n, rpt::kSegRows), c.sel, c.out_sel,
                       c.out_count_dev);
  if (st != RPT_OK || c.n_dst == 0) return st;
  return enqueue_transfer_inserts(c.dst_filters, c.dst_cols, c.n_dst, dst_routed, ws.bits, c.sel, c.out_sel, c.out_count_dev,
                                  c.n, c.insert_workspace, s);
}

}  // namespace
