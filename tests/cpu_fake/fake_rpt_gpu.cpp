// fake_rpt_gpu.cpp — the part of include/rpt_gpu.h that csrc/rpt_host.cpp and the C++ host tests call, on the CPU.
//
// ***************************************************************************************
// TEST INFRASTRUCTURE ONLY (like oracle/). It restates the documented ABI; nothing here comes
// from the product kernels, and the product never links it.
// ***************************************************************************************
//
// Every stream-ordered entry point validates its arguments as the header documents, then enqueues ONE closure on
// the fake stream it was given (fake_hip.hpp). When the closure runs it computes the result with the functions of
// oracle/rpt_oracle.cpp (sizing, key hash, insert, find, lookup-sel, min/max, the resize predicates); what the
// oracle has no function for (row_sel / dictionary composition, widening narrow keys, the chain's AND) is written
// plainly here. Pointers are read when the closure RUNS, as a kernel would: a buffer refilled or freed too early
// is seen refilled or freed.
//
// Workspaces are strict on purpose: the sizing functions return nonzero above a row threshold and whenever a
// PARTITIONED / BUCKETED strategy is forced; an operation that needs one refuses a null or short workspace; and
// when its closure runs it overwrites the whole workspace with garbage, so a workspace freed while an operation
// is pending shows under ASan.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "fake_hip.hpp"
#include "rpt_gpu.h"

extern "C" {  // oracle/rpt_oracle.cpp, compiled into the same binary
int rpt_oracle_log_num_blocks(uint64_t n_rows);
int rpt_oracle_needs_resize(uint64_t sized_for_rows, uint64_t actual_rows);
int rpt_oracle_needs_resize_alloc(int log_num_blocks, uint64_t actual_rows);
void rpt_oracle_hash_i64(const int64_t* keys, const uint32_t* key_sel, const uint64_t* validity, uint64_t n, uint64_t* out);
void rpt_oracle_hash_i32(const int32_t* keys, const uint32_t* key_sel, const uint64_t* validity, uint64_t n, uint64_t* out);
void rpt_oracle_hash_combine_i64(const int64_t* keys, const uint32_t* key_sel, const uint64_t* validity, uint64_t n,
                                 uint64_t* inout);
void rpt_oracle_hash_combine_i32(const int32_t* keys, const uint32_t* key_sel, const uint64_t* validity, uint64_t n,
                                 uint64_t* inout);
int rpt_oracle_minmax_i64(const int64_t* keys, const uint32_t* key_sel, const uint64_t* validity, uint64_t n, int64_t* out2);
int rpt_oracle_minmax_i32(const int32_t* keys, const uint32_t* key_sel, const uint64_t* validity, uint64_t n, int64_t* out2);
void rpt_oracle_insert_hashes(uint64_t* words, int log_nb, const uint64_t* h, uint64_t n);
void rpt_oracle_find_hashes(const uint64_t* words, int log_nb, const uint64_t* h, uint64_t n, uint8_t* bv);
uint64_t rpt_oracle_lookup_sel_hashes(const uint64_t* words, int log_nb, const uint64_t* h, uint64_t n, uint32_t* sel);
}

struct rpt_bf {
  int device = 0;
  int log_num_blocks = 0;
  uint64_t sized_for_rows = 0;
  std::atomic<int> has_data{0}, finalized{0};
  std::atomic<int> probe_strategy{RPT_PROBE_AUTO}, insert_strategy{RPT_INSERT_AUTO};
  uint64_t* words = nullptr;  // fake device memory (hipMalloc)
  std::mutex mu;              // inserts, min/max
  bool has_minmax = false;
  int64_t min_value = 0, max_value = 0;
};

namespace {

thread_local std::string t_last_error;

__attribute__((format(printf, 2, 3))) int fail(int status, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  t_last_error = buf;
  return status;
}

hipStream_t as_stream(rpt_stream_t s) { return static_cast<hipStream_t>(s); }
size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

int enqueue(rpt_stream_t stream, std::function<void()> op) {
  const hipError_t e = fake_hip::enqueue(as_stream(stream), std::move(op));
  return e == hipSuccess ? RPT_OK : fail(RPT_ERR_HIP, "enqueue failed: %s", hipGetErrorString(e));
}

int check_col(const rpt_key_column* col) {
  if (!col) return fail(RPT_ERR_INVALID_ARGUMENT, "null key column");
  if (col->key_type < RPT_KEY_I64 || col->key_type > RPT_KEY_HASH)
    return fail(RPT_ERR_INVALID_ARGUMENT, "bad key_type %d", col->key_type);
  if (!col->keys) return fail(RPT_ERR_INVALID_ARGUMENT, "null keys pointer");
  return RPT_OK;
}

// ---- the fixed strategy / workspace rule of this fake ------------------------------------------------------------
// AUTO inserts take a workspace from kInsertWsRows rows; probes always do, except the fused small batch of
// rpt_bf_probe (AUTO probes are routed from kProbeRoutedRows rows); a forced strategy is echoed. The sizes only
// have to be nonzero and grow with n.
constexpr uint64_t kInsertWsRows = 40000;
constexpr uint64_t kProbeRoutedRows = 1u << 16;

int resolve_insert(const rpt_bf* bf, uint64_t n) {
  const int s = bf->insert_strategy.load();
  if (s != RPT_INSERT_AUTO) return s;
  return n >= kInsertWsRows ? RPT_INSERT_PARTITIONED : RPT_INSERT_ATOMIC;
}
size_t insert_ws_bytes(const rpt_bf* bf, uint64_t n) {
  return resolve_insert(bf, n) == RPT_INSERT_ATOMIC ? 0 : align256(256 + n * 4);
}
bool fused(const rpt_bf* bf, uint64_t n) {
  return n > 0 && n <= RPT_SMALL_PROBE_ROWS && bf->probe_strategy.load() == RPT_PROBE_AUTO;
}
int resolve_probe(const rpt_bf* bf, uint64_t n) {
  const int s = bf->probe_strategy.load();
  if (s != RPT_PROBE_AUTO) return s;
  return n >= kProbeRoutedRows ? RPT_PROBE_PARTITIONED : RPT_PROBE_GATHER;
}
size_t probe_ws_bytes(const rpt_bf* bf, uint64_t n) {
  if (n == 0) return 0;  // (a fused small probe needs none, but the sizing function does not know the entry point)
  const int s = resolve_probe(bf, n);
  if (s == RPT_PROBE_PARTITIONED || s == RPT_PROBE_BUCKETED) return align256(256 + n * 4);
  return align256(64 + (n + 511) / 512 * 72);  // result bits + one count per 512-row segment
}
int check_workspace(size_t need, const void* ws, size_t bytes) {
  if (need == 0) return RPT_OK;
  if (!ws || bytes < need) return fail(RPT_ERR_WORKSPACE, "workspace %zu bytes < required %zu", bytes, need);
  if (reinterpret_cast<uintptr_t>(ws) & 15u) return fail(RPT_ERR_INVALID_ARGUMENT, "workspace %p is not 16-byte aligned", ws);
  return RPT_OK;
}
void trash(void* ws, size_t bytes) {
  if (ws && bytes) std::memset(ws, 0x5E, bytes);
}

// ---- what the closures compute ------------------------------------------------------------------------------------
// The physical index of probed row i: key_sel[r] of the row r = row_sel[i] (or i); nullptr when it is i itself.
const uint32_t* compose(const rpt_key_column& c, const uint32_t* row_sel, uint64_t n, std::vector<uint32_t>& store) {
  if (!row_sel) return c.key_sel;
  if (!c.key_sel) return row_sel;
  store.resize(n);
  for (uint64_t i = 0; i < n; i++) store[i] = c.key_sel[row_sel[i]];
  return store.data();
}
// Hash of rows row_sel[0 .. n) (or 0 .. n) of the column, as the filter sees them.
std::vector<uint64_t> row_hashes(const rpt_key_column& c, const uint32_t* row_sel, uint64_t n) {
  std::vector<uint64_t> h(n);
  std::vector<uint32_t> store;
  const uint32_t* idx = compose(c, row_sel, n, store);
  switch (c.key_type) {
    case RPT_KEY_I64: rpt_oracle_hash_i64(static_cast<const int64_t*>(c.keys), idx, c.validity, n, h.data()); break;
    case RPT_KEY_I32: rpt_oracle_hash_i32(static_cast<const int32_t*>(c.keys), idx, c.validity, n, h.data()); break;
    default: {  // RPT_KEY_HASH: the values are the hashes; validity is not applied
      const uint64_t* k = static_cast<const uint64_t*>(c.keys);
      for (uint64_t i = 0; i < n; i++) h[i] = k[idx ? idx[i] : i];
    }
  }
  return h;
}
void do_insert(rpt_bf* bf, const rpt_key_column& c, uint64_t n) {
  const std::vector<uint64_t> h = row_hashes(c, nullptr, n);
  int64_t mm[2];
  int has = 0;
  if (c.key_type == RPT_KEY_I64) has = rpt_oracle_minmax_i64(static_cast<const int64_t*>(c.keys), c.key_sel, c.validity, n, mm);
  else if (c.key_type == RPT_KEY_I32) has = rpt_oracle_minmax_i32(static_cast<const int32_t*>(c.keys), c.key_sel, c.validity, n, mm);
  std::lock_guard<std::mutex> lk(bf->mu);
  rpt_oracle_insert_hashes(bf->words, bf->log_num_blocks, h.data(), n);
  if (has) {
    bf->min_value = bf->has_minmax ? std::min(bf->min_value, mm[0]) : mm[0];
    bf->max_value = bf->has_minmax ? std::max(bf->max_value, mm[1]) : mm[1];
    bf->has_minmax = true;
  }
}
void do_probe(const rpt_bf* bf, const rpt_key_column& c, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
              uint64_t* out_count) {
  const std::vector<uint64_t> h = row_hashes(c, row_sel, n);
  std::vector<uint32_t> pos(n);  // the oracle writes one entry past the survivors: keep that out of out_sel
  const uint64_t cnt = rpt_oracle_lookup_sel_hashes(bf->words, bf->log_num_blocks, h.data(), n, pos.data());
  for (uint64_t j = 0; j < cnt; j++) out_sel[j] = row_sel ? row_sel[pos[j]] : pos[j];
  *out_count = cnt;
}

int alloc_words(rpt_bf* bf, int log_num_blocks) {
  void* p = nullptr;
  const size_t bytes = sizeof(uint64_t) << log_num_blocks;
  if (hipMalloc(&p, bytes) != hipSuccess) return fail(RPT_ERR_OUT_OF_MEMORY, "hipMalloc of %zu bytes failed", bytes);
  std::memset(p, 0, bytes);
  bf->words = static_cast<uint64_t*>(p);
  bf->log_num_blocks = log_num_blocks;
  return RPT_OK;
}

}  // namespace

extern "C" {

const char* rpt_last_error(void) { return t_last_error.c_str(); }

int rpt_bf_needs_resize(uint64_t sized_for_rows, uint64_t actual_rows) {
  return rpt_oracle_needs_resize(sized_for_rows, actual_rows);
}
int rpt_bf_needs_resize_alloc(const rpt_bf* bf, uint64_t actual_rows) {
  if (!bf) return -fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  return rpt_oracle_needs_resize_alloc(bf->log_num_blocks, actual_rows);
}

// ---- lifetime and state ---------------------------------------------------------------------------------------------
int rpt_bf_create(int device, uint64_t est_num_rows, rpt_bf** out) {
  if (!out) return fail(RPT_ERR_INVALID_ARGUMENT, "null out");
  *out = nullptr;
  if (device != 0) return fail(RPT_ERR_HIP, "hipSetDevice(%d): invalid device ordinal", device);
  rpt_bf* bf = new rpt_bf();
  bf->device = device;
  const int st = alloc_words(bf, rpt_oracle_log_num_blocks(est_num_rows));
  if (st != RPT_OK) {
    delete bf;
    return st;
  }
  bf->sized_for_rows = est_num_rows;
  *out = bf;
  return RPT_OK;
}
int rpt_bf_destroy(rpt_bf* bf) {
  if (!bf) return RPT_OK;
  (void)hipFree(bf->words);  // waits for the device, like the real call: no pending closure still uses bf
  delete bf;
  return RPT_OK;
}
int rpt_bf_reinitialize(rpt_bf* bf, uint64_t actual_rows) {  // synchronous
  if (!bf) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  fake_hip::device_synchronize();
  (void)hipFree(bf->words);
  bf->words = nullptr;
  const int st = alloc_words(bf, rpt_oracle_log_num_blocks(actual_rows));
  if (st != RPT_OK) return st;
  bf->sized_for_rows = actual_rows;
  bf->has_data.store(0);
  std::lock_guard<std::mutex> lk(bf->mu);
  bf->has_minmax = false;
  return RPT_OK;
}
int rpt_bf_get_info(const rpt_bf* bf, rpt_bf_info* out) {
  if (!bf || !out) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  out->device = bf->device;
  out->log_num_blocks = bf->log_num_blocks;
  out->num_blocks = 1ULL << bf->log_num_blocks;
  out->sized_for_rows = bf->sized_for_rows;
  out->has_data = bf->has_data.load();
  out->finalized = bf->finalized.load();
  out->words = bf->words;
  return RPT_OK;
}
int rpt_bf_get_minmax(const rpt_bf* bf, int64_t* out_min, int64_t* out_max, int* out_has_value, rpt_stream_t stream) {
  if (!bf || !out_min || !out_max || !out_has_value) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  rpt_bf* b = const_cast<rpt_bf*>(bf);
  int64_t v[2] = {0, 0};
  int has = 0;
  const int st = enqueue(stream, [b, &v, &has] {  // stream-ordered read ...
    std::lock_guard<std::mutex> lk(b->mu);
    has = b->has_minmax ? 1 : 0;
    v[0] = has ? b->min_value : 0;
    v[1] = has ? b->max_value : 0;
  });
  if (st != RPT_OK) return st;
  if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return fail(RPT_ERR_HIP, "hipStreamSynchronize failed");  // ... then the sync
  *out_has_value = has;
  *out_min = v[0];
  *out_max = v[1];
  return RPT_OK;
}
int rpt_bf_export_words(const rpt_bf* bf, uint64_t* host_words, uint64_t n_words) {  // synchronous
  if (!bf || !host_words) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n_words != (1ULL << bf->log_num_blocks))
    return fail(RPT_ERR_SHAPE_MISMATCH, "export of %llu words from a %llu-word filter", (unsigned long long)n_words,
                (unsigned long long)(1ULL << bf->log_num_blocks));
  fake_hip::device_synchronize();
  std::memcpy(host_words, bf->words, n_words * 8);
  return RPT_OK;
}

// ---- strategy control -----------------------------------------------------------------------------------------------
int rpt_bf_set_insert_strategy(rpt_bf* bf, int strategy) {
  if (!bf) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  if (strategy < RPT_INSERT_AUTO || strategy > RPT_INSERT_BUCKETED)
    return fail(RPT_ERR_INVALID_ARGUMENT, "unknown insert strategy %d", strategy);
  bf->insert_strategy.store(strategy);
  return RPT_OK;
}
int rpt_bf_set_probe_strategy(rpt_bf* bf, int strategy) {
  if (!bf) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  if (strategy < RPT_PROBE_AUTO || strategy > RPT_PROBE_BUCKETED)
    return fail(RPT_ERR_INVALID_ARGUMENT, "unknown probe strategy %d", strategy);
  bf->probe_strategy.store(strategy);
  return RPT_OK;
}
int rpt_bf_insert_strategy_for(const rpt_bf* bf, uint64_t n_rows) {
  if (!bf) return -fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  return resolve_insert(bf, n_rows);
}
int rpt_bf_probe_strategy_for(const rpt_bf* bf, uint64_t n_rows) {
  if (!bf) return -fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  return resolve_probe(bf, n_rows);
}

// ---- inserts ----------------------------------------------------------------------------------------------------------
size_t rpt_bf_insert_workspace_bytes(const rpt_bf* bf, uint64_t n_rows) { return bf ? insert_ws_bytes(bf, n_rows) : 0; }

int rpt_bf_insert(rpt_bf* bf, const rpt_key_column* col, uint64_t n, rpt_stream_t stream) {
  if (!bf) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  if (n == 0) return RPT_OK;
  const int st = check_col(col);
  if (st != RPT_OK) return st;
  bf->has_data.store(1);
  const rpt_key_column c = *col;
  return enqueue(stream, [bf, c, n] { do_insert(bf, c, n); });
}
int rpt_bf_insert_ws(rpt_bf* bf, const rpt_key_column* col, uint64_t n, void* workspace, size_t workspace_bytes,
                     rpt_stream_t stream) {
  if (!bf) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  if (n == 0) return RPT_OK;
  if (resolve_insert(bf, n) == RPT_INSERT_ATOMIC) return rpt_bf_insert(bf, col, n, stream);
  int st = check_col(col);
  if (st != RPT_OK) return st;
  st = check_workspace(insert_ws_bytes(bf, n), workspace, workspace_bytes);
  if (st != RPT_OK) return st;
  bf->has_data.store(1);
  const rpt_key_column c = *col;
  return enqueue(stream, [bf, c, n, workspace, workspace_bytes] {
    trash(workspace, workspace_bytes);
    do_insert(bf, c, n);
  });
}

// ---- probes -----------------------------------------------------------------------------------------------------------
int rpt_bf_probe_is_fused(const rpt_bf* bf, uint64_t n_rows) {
  if (!bf) return -fail(RPT_ERR_INVALID_ARGUMENT, "null filter");
  return fused(bf, n_rows) ? 1 : 0;
}
size_t rpt_bf_probe_workspace_bytes(const rpt_bf* bf, uint64_t n_rows) { return bf ? probe_ws_bytes(bf, n_rows) : 0; }

int rpt_bf_probe(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                 uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  if (!bf || !out_count_dev) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n >= (1ULL << 32)) return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds uint32 sel_t", (unsigned long long)n);
  if (n == 0) return enqueue(stream, [out_count_dev] { *out_count_dev = 0; });
  int st = check_col(col);
  if (st != RPT_OK) return st;
  if (!out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  const bool small = fused(bf, n);  // one fused launch: the workspace is neither needed nor touched
  if (!small) {
    st = check_workspace(probe_ws_bytes(bf, n), workspace, workspace_bytes);
    if (st != RPT_OK) return st;
  }
  const rpt_key_column c = *col;
  return enqueue(stream, [=] {
    if (!small) trash(workspace, workspace_bytes);
    do_probe(bf, c, row_sel, n, out_sel, out_count_dev);
  });
}
int rpt_bf_probe_bits(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n, uint64_t* out_bits,
                      void* workspace, size_t workspace_bytes, rpt_stream_t stream) {
  if (!bf || !out_bits) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n >= (1ULL << 32)) return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds uint32 sel_t", (unsigned long long)n);
  if (n == 0) return RPT_OK;
  int st = check_col(col);
  if (st != RPT_OK) return st;
  // never fused: this entry point always runs the phased probe, so it always needs its workspace
  st = check_workspace(probe_ws_bytes(bf, n), workspace, workspace_bytes);
  if (st != RPT_OK) return st;
  const rpt_key_column c = *col;
  return enqueue(stream, [=] {
    trash(workspace, workspace_bytes);
    const std::vector<uint64_t> h = row_hashes(c, row_sel, n);
    std::memset(out_bits, 0, (n + 511) / 512 * 64);  // ceil(n / 512) * 8 words, bits past n zero
    rpt_oracle_find_hashes(bf->words, bf->log_num_blocks, h.data(), n, reinterpret_cast<uint8_t*>(out_bits));
  });
}
int rpt_bf_probe_chain(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                       const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                       rpt_stream_t stream) {
  if (!filters || !cols || !out_count_dev) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n_filters == 0 || n_filters > RPT_MAX_CHAIN)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n_filters=%u outside 1..%d", n_filters, RPT_MAX_CHAIN);
  if (n > RPT_SMALL_PROBE_ROWS)
    return fail(RPT_ERR_INVALID_ARGUMENT, "n=%llu rows exceeds RPT_SMALL_PROBE_ROWS", (unsigned long long)n);
  for (uint32_t f = 0; f < n_filters; f++) {
    if (!filters[f]) return fail(RPT_ERR_INVALID_ARGUMENT, "null filter %u", f);
    const int st = check_col(&cols[f]);
    if (st != RPT_OK) return st;
  }
  if (n == 0) return enqueue(stream, [out_count_dev] { *out_count_dev = 0; });
  if (!out_sel) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_sel");
  const std::vector<const rpt_bf*> fs(filters, filters + n_filters);
  const std::vector<rpt_key_column> cs(cols, cols + n_filters);
  return enqueue(stream, [=] {
    std::vector<uint8_t> pass((n + 7) / 8, 0xFF), one((n + 7) / 8);
    for (size_t f = 0; f < fs.size(); f++) {  // the AND of the filters, each on its own column
      const std::vector<uint64_t> h = row_hashes(cs[f], row_sel, n);
      rpt_oracle_find_hashes(fs[f]->words, fs[f]->log_num_blocks, h.data(), n, one.data());
      for (size_t b = 0; b < pass.size(); b++) pass[b] &= one[b];
    }
    uint64_t cnt = 0;
    for (uint64_t i = 0; i < n; i++)
      if ((pass[i >> 3] >> (i & 7)) & 1) out_sel[cnt++] = row_sel ? row_sel[i] : static_cast<uint32_t>(i);
    *out_count_dev = cnt;
  });
}

// ---- hashing and keys -------------------------------------------------------------------------------------------------
int rpt_hash_keys(const rpt_key_column* col, uint64_t n, uint64_t* out_hashes, rpt_stream_t stream) {
  const int st = check_col(col);
  if (st != RPT_OK) return st;
  if (n == 0) return RPT_OK;
  if (!out_hashes) return fail(RPT_ERR_INVALID_ARGUMENT, "null out_hashes");
  const rpt_key_column c = *col;
  return enqueue(stream, [c, n, out_hashes] {
    const std::vector<uint64_t> h = row_hashes(c, nullptr, n);
    std::memcpy(out_hashes, h.data(), n * 8);
  });
}
int rpt_hash_combine(const rpt_key_column* col, uint64_t n, uint64_t* inout_hashes, rpt_stream_t stream) {
  const int st = check_col(col);
  if (st != RPT_OK) return st;
  if (n == 0) return RPT_OK;
  if (!inout_hashes) return fail(RPT_ERR_INVALID_ARGUMENT, "null inout_hashes");
  if (col->key_type == RPT_KEY_HASH) return fail(RPT_ERR_INVALID_ARGUMENT, "combining a hash column is not faked");
  const rpt_key_column c = *col;
  return enqueue(stream, [c, n, inout_hashes] {
    if (c.key_type == RPT_KEY_I64)
      rpt_oracle_hash_combine_i64(static_cast<const int64_t*>(c.keys), c.key_sel, c.validity, n, inout_hashes);
    else
      rpt_oracle_hash_combine_i32(static_cast<const int32_t*>(c.keys), c.key_sel, c.validity, n, inout_hashes);
  });
}
int rpt_keys_widen(const uint32_t* lo, const uint32_t* chunk_hi, const uint32_t* chunk_row0, uint64_t n_chunks,
                   uint64_t* out, rpt_stream_t stream) {
  if (n_chunks == 0) return RPT_OK;
  if (!lo || !chunk_hi || !chunk_row0 || !out) return fail(RPT_ERR_INVALID_ARGUMENT, "null argument");
  if (n_chunks > 0x7FFFFFFFu) return fail(RPT_ERR_INVALID_ARGUMENT, "too many chunks");
  return enqueue(stream, [=] {
    for (uint64_t c = 0; c < n_chunks; c++)
      for (uint64_t r = chunk_row0[c]; r < chunk_row0[c + 1]; r++) out[r] = static_cast<uint64_t>(chunk_hi[c]) << 32 | lo[r];
  });
}

// ---- not faked ----------------------------------------------------------------------------------------------------------
int rpt_bf_allreduce_or(rpt_bf*, void*, rpt_stream_t) {
  return fail(RPT_ERR_COLLECTIVE, "the CPU fake has no RCCL");
}

}  // extern "C"
