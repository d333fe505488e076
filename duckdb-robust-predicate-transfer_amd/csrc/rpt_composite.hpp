// rpt_composite.hpp — composite join keys hashed inside the kernels: rpt_hash_keys_composite,
// rpt_bf_insert_composite, and the one-launch rpt_bf_probe_chain_composite, rpt_bf_transfer_composite and
// rpt_bf_insert_multi_composite, one launch of kernels/composite.hpp each, no workspace. Host code of librpt_gpu.so,
// included by rpt_gpu.hip inside its extern "C" block, directly after rpt_transfer_small.hpp (the list, device and
// destination checks are those of rpt_chain_call.hpp, the write scopes those of rpt_probe_sel_small.hpp, both run over
// each key's first column). Nothing else dispatches to these calls. Every kernel recorded here has a row in
// tests/kernel_ledger_composite.py (tests/test_kernel_ledger_composite_names.py scans this file).
#pragma once

namespace {

// One key, looking into no handle: `what` names it in the message ("key", "key 2", "destination key 0").
int check_composite_key(const rpt_composite_key* key, const char* what) {
  if (!key) return fail(RPT_ERR_INVALID_ARGUMENT, "null %s", what);
  if (!key->cols) return fail(RPT_ERR_INVALID_ARGUMENT, "null cols in %s", what);
  if (key->n_cols == 0 || key->n_cols > RPT_MAX_KEY_COLUMNS)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_cols=%u outside 1..%d in %s", key->n_cols, RPT_MAX_KEY_COLUMNS, what);
  for (uint32_t j = 0; j < key->n_cols; j++) {
    const rpt_key_column& col = key->cols[j];
    if (col.key_type < RPT_KEY_I64 || col.key_type > RPT_KEY_HASH)
      return fail(RPT_ERR_INVALID_ARGUMENT, "bad key_type %d in column %u of %s", col.key_type, j, what);
    if (col.key_type == RPT_KEY_HASH && j > 0)
      return fail(RPT_ERR_INVALID_ARGUMENT, "HASH column at position %u of %s: a hashed prefix is column 0", j, what);
    if (!col.keys) return fail(RPT_ERR_INVALID_ARGUMENT, "null keys pointer in column %u of %s", j, what);
  }
  return RPT_OK;
}

// The keys of one side of a one-launch call (count in 1..RPT_MAX_CHAIN, checked by the caller): every key, then the
// column total. first_cols[f] becomes key f's column 0, the column the single-column helpers are run over.
int check_composite_keys(const rpt_composite_key* keys, uint32_t count, const char* side, rpt_key_column* first_cols) {
  uint32_t total = 0;
  for (uint32_t f = 0; f < count; f++) {
    char what[40];
    snprintf(what, sizeof what, "%skey %u", side, f);
    const int st = check_composite_key(&keys[f], what);
    if (st != RPT_OK) return st;
    first_cols[f] = keys[f].cols[0];
    total += keys[f].n_cols;
  }
  if (total > RPT_MAX_CHAIN_KEY_COLUMNS)
    return fail(RPT_ERR_INVALID_ARGUMENT, "%u columns over the %skeys exceed RPT_MAX_CHAIN_KEY_COLUMNS (%d)", total, side,
                RPT_MAX_CHAIN_KEY_COLUMNS);
  return RPT_OK;
}

rpt::CompositeCol composite_col(const rpt_key_column& col) {
  return rpt::CompositeCol{col.keys, col.key_sel, col.validity, col.key_type};
}

rpt::CompositeKeyArgs composite_key_args(const rpt_composite_key* key) {
  rpt::CompositeKeyArgs a{};
  for (uint32_t j = 0; j < key->n_cols; j++) a.col[j] = composite_col(key->cols[j]);
  a.n_cols = key->n_cols;
  return a;
}

// The dense mapping: every column flat and its keys 16-byte aligned.
bool composite_dense_ok(const rpt_composite_key* key) {
  for (uint32_t j = 0; j < key->n_cols; j++)
    if (!dense_ok(&key->cols[j], nullptr)) return false;
  return true;
}

// One side's kernel argument: the flat column table and each filter's first column.
void fill_composite_side(rpt::CompositeSide& side, const rpt_bf* const* filters, const rpt_composite_key* keys,
                         uint32_t count) {
  uint32_t at = 0;
  for (uint32_t f = 0; f < count; f++) {
    side.words[f] = filters[f]->words;
    side.block_mask[f] = (1ULL << filters[f]->log_num_blocks) - 1;
    side.stats[f] = filters[f]->stats;
    side.first[f] = static_cast<uint8_t>(at);
    for (uint32_t j = 0; j < keys[f].n_cols; j++) side.col[at++] = composite_col(keys[f].cols[j]);
  }
  side.first[count] = static_cast<uint8_t>(at);
  side.n = count;
}

// The launch of a checked call, n > 0, the device current: launch_transfer_small's order (rpt_transfer_small.hpp).
// Every destination's capture check and every probed filter's pending clear before anything is enqueued, has_data, the
// write scopes in ascending handle address held across the one launch. c.n_filters == 0: the sink alone; c.n_dst == 0:
// the chain, which takes no write scope.
int launch_composite_small(const ChainCall& c, const rpt_composite_key* keys, const rpt_composite_key* dst_keys,
                           hipStream_t s) {
  rpt::CompositeSide p{}, d{};
  fill_composite_side(p, c.filters, keys, c.n_filters);
  fill_composite_side(d, c.dst_filters, dst_keys, c.n_dst);
  int st = refuse_captured_dsts(c, s);
  if (st != RPT_OK) return st;
  for (uint32_t f = 0; f < c.n_filters; f++) RPT_SETTLE(c.filters[f], s);
  for (uint32_t j = 0; j < c.n_dst; j++) c.dst_filters[j]->has_data.store(1);
  WriteOrders orders;
  st = take_write_orders(c, s, orders);
  if (st != RPT_OK) return st;
  auto launch = [&](auto probed, auto transfer) {
    return launch_kernel<rpt::chain_composite_small_kernel<probed(), transfer()>, probed(), transfer()>(
        "chain_composite_small_kernel", kRecorded, 1, rpt::kSmallThreads, 0, s, p, d, c.sel, c.n, c.out_sel,
        c.out_count_dev);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  st = c.n_filters == 0 ? launch(no, yes) : c.n_dst == 0 ? launch(yes, no) : launch(yes, yes);
  for (uint32_t i = 0; i < orders.n; i++) orders[i].done(false);
  return st;
}

// The body of rpt_bf_probe_chain_composite (transfer false) and rpt_bf_transfer_composite. Before any handle is looked
// into: the lists and their counts, every key and the column totals, then transfer_small_impl's order
// (rpt_transfer_small.hpp): null handles and a destination among the probed filters, n against RPT_SMALL_PROBE_ROWS,
// the overlap of out_sel with a given row_sel; then the filters' devices, the destinations, n == 0 sets the count, a
// null out_sel, the capture refusals and the settles.
int chain_composite_impl(const rpt_bf* const* filters, const rpt_composite_key* keys, uint32_t n_filters, bool transfer,
                         rpt_bf* const* dst_filters, const rpt_composite_key* dst_keys, uint32_t n_dst,
                         const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                         rpt_stream_t stream) {
  if (!filters || !keys || !out_count_dev || (transfer && (!dst_filters || !dst_keys)))
    return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n_filters == 0 || n_filters > RPT_MAX_CHAIN)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_filters=%u outside 1..%d", n_filters, RPT_MAX_CHAIN);
  if (transfer && (n_dst == 0 || n_dst > RPT_MAX_CHAIN))
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_dst=%u outside 1..%d", n_dst, RPT_MAX_CHAIN);
  rpt_key_column first_cols[RPT_MAX_CHAIN], dst_first_cols[RPT_MAX_CHAIN];
  int st = check_composite_keys(keys, n_filters, "", first_cols);
  if (st != RPT_OK) return st;
  if (transfer) {
    st = check_composite_keys(dst_keys, n_dst, "destination ", dst_first_cols);
    if (st != RPT_OK) return st;
  }
  const ChainCall c{filters, first_cols, n_filters, transfer, dst_filters, dst_first_cols, transfer ? n_dst : 0, false,
                    row_sel, nullptr, n, 0, out_sel, out_count_dev, nullptr, 0, false, nullptr, 0, stream};
  st = check_chain_lists(c);  // the null handles, and a destination that is also probed
  if (st != RPT_OK) return st;
  if (n > rpt::kSmallRows)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds RPT_SMALL_PROBE_ROWS", (unsigned long long)n);
  // the inserts read row_sel after the tail has begun to write out_sel
  if (transfer && n > 0 && row_sel && out_sel && sel_ranges_overlap(row_sel, out_sel, n))
    return fail(RPT_ERR_INVALID_ARGUMENT, "out_sel overlaps row_sel (%llu entries each)", (unsigned long long)n);
  st = check_chain_filters(filters, n_filters);
  if (st != RPT_OK) return st;
  const int device = filters[0]->device;
  st = check_chain_dsts(c, device, nullptr);  // no destination routes here
  if (st != RPT_OK) return st;
  RPT_ON_DEVICE(device);
  hipStream_t s = as_stream(stream);
  if (n == 0) {  // nothing can be selected: no destination is touched
    RPT_HIP(hipMemsetAsync(out_count_dev, 0, sizeof(uint64_t), s));
    return RPT_OK;
  }
  if (!out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  return launch_composite_small(c, keys, dst_keys, s);
}
}  // namespace

int rpt_hash_keys_composite(const rpt_composite_key* key, uint64_t n, uint64_t* out_hashes, rpt_stream_t stream) {
  int st = check_composite_key(key, "key");
  if (st != RPT_OK) return st;
  if (key->n_cols == 1) return rpt_hash_keys(&key->cols[0], n, out_hashes, stream);
  if (!out_hashes) return fail(RPT_ERR_INVALID_ARGUMENT, "null out");
  if (n == 0) return RPT_OK;
  int device = 0;
  RPT_HIP(hipGetDevice(&device));
  const uint64_t n_segs = ceil_div(n, rpt::kSegRows);
  const unsigned grid = persistent_grid(device, n_segs);
  const rpt::CompositeKeyArgs a = composite_key_args(key);
  // the dense kernel stores the hashes of four rows as two 16-byte vectors
  const bool dense = composite_dense_ok(key) && !misaligned16(out_hashes);
  return dispatch_bool(dense, [&](auto d) {
    return launch_kernel<rpt::hash_composite_kernel<d()>, d()>("hash_composite_kernel", kRecorded, grid, rpt::kBlockThreads,
                                                             0, as_stream(stream), a, n, n_segs, out_hashes);
  });
}

// rpt_bf_insert with the key hashed from its columns in the insert kernel; no min/max (a composite key carries none).
int rpt_bf_insert_composite(rpt_bf* bf, const rpt_composite_key* key, uint64_t n, rpt_stream_t stream) {
  int st = check_composite_key(key, "key");
  if (st != RPT_OK) return st;
  if (key->n_cols == 1) return rpt_bf_insert(bf, &key->cols[0], n, stream);
  if (!bf) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  if (n == 0) return RPT_OK;
  RPT_ON_DEVICE(bf->device);
  RPT_REFUSE_CAPTURE_WRITE(bf, as_stream(stream), "insert");
  bf->has_data.store(1);
  const uint64_t n_segs = ceil_div(n, rpt::kSegRows);
  const unsigned grid = persistent_grid(bf->device, n_segs);
  const rpt::CompositeKeyArgs a = composite_key_args(key);
  WriteOrder order(bf, as_stream(stream));
  RPT_REFUSE_IN_FLIGHT(order, "write");
  const hipError_t ez = zero_pending_locked(bf, as_stream(stream));
  if (ez != hipSuccess) return fail(RPT_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(ez));
  st = dispatch_bool(composite_dense_ok(key), [&](auto d) {
    return launch_kernel<rpt::insert_composite_kernel<d()>, d()>("insert_composite_kernel", kRecorded, grid,
                                                               rpt::kBlockThreads, 0, as_stream(stream), bf->words,
                                                               (1ULL << bf->log_num_blocks) - 1, a, n, n_segs);
  });
  order.done(false);
  return st;
}

int rpt_bf_probe_chain_composite(const rpt_bf* const* filters, const rpt_composite_key* keys, uint32_t n_filters,
                                 const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                                 rpt_stream_t stream) {
  return chain_composite_impl(filters, keys, n_filters, false, nullptr, nullptr, 0, row_sel, n, out_sel, out_count_dev,
                              stream);
}

int rpt_bf_transfer_composite(const rpt_bf* const* filters, const rpt_composite_key* keys, uint32_t n_filters,
                              rpt_bf* const* dst_filters, const rpt_composite_key* dst_keys, uint32_t n_dst,
                              const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                              rpt_stream_t stream) {
  return chain_composite_impl(filters, keys, n_filters, true, dst_filters, dst_keys, n_dst, row_sel, n, out_sel,
                              out_count_dev, stream);
}

// The sink alone: a transfer with no probed filter, in which every listed row survives (rpt_bf_insert_multi's order,
// the keys checked once the count lets them be read).
int rpt_bf_insert_multi_composite(rpt_bf* const* dst_filters, const rpt_composite_key* dst_keys, uint32_t n_dst,
                                  const uint32_t* row_sel, uint64_t n, rpt_stream_t stream) {
  if (!dst_filters || !dst_keys) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n_dst == 0 || n_dst > RPT_MAX_CHAIN)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_dst=%u outside 1..%d", n_dst, RPT_MAX_CHAIN);
  rpt_key_column dst_first_cols[RPT_MAX_CHAIN];
  int st = check_composite_keys(dst_keys, n_dst, "destination ", dst_first_cols);
  if (st != RPT_OK) return st;
  for (uint32_t j = 0; j < n_dst; j++)
    if (!dst_filters[j]) return fail(RPT_ERR_INVALID_ARGUMENT, "null destination filter %u", j);
  if (n > rpt::kSmallRows)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds RPT_SMALL_PROBE_ROWS", (unsigned long long)n);
  const ChainCall c{nullptr, nullptr, 0, true, dst_filters, dst_first_cols, n_dst, false, row_sel, nullptr, n, 0,
                    nullptr, nullptr, nullptr, 0, false, nullptr, 0, stream};
  const int device = dst_filters[0]->device;
  st = check_chain_dsts(c, device, nullptr);
  if (st != RPT_OK || n == 0) return st;
  RPT_ON_DEVICE(device);
  return launch_composite_small(c, dst_keys, dst_keys, as_stream(stream));
}
