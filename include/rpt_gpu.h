/*
 * rpt_gpu.h — C-ABI of the MI355X-native predicate-transfer Bloom filter (librpt_gpu.so).
 *
 * This is the drop-in boundary for the reference's PTBloomFilter seam
 * (/root/reference/src/include/bloom_filter.hpp:22-57, src/bloom_filter.cpp:11-78): the DuckDB
 * operators PhysicalCreateBF::Sink/Finalize (src/operators/physical_create_bf.cpp:201-242,352-419)
 * and PhysicalUseBF::ExecuteInternal (src/operators/physical_use_bf.cpp:60-198) call these entry
 * points instead of the DuckDB-native BloomFilter. Plain pointers and sizes only; no exceptions
 * cross the ABI (every entry point returns an rpt_status); device work is enqueued on the caller's
 * HIP stream and is asynchronous unless stated otherwise.
 *
 * Filter spec: the Arrow Acero BlockedBloomFilter the reference README ports (README.md:23-32):
 * 2^k 64-bit blocks, a 1024-entry table of 57-bit masks (4-5 bits set), mask rotation by hash bits
 * 10..15, block id from hash bits 16... Key hash: DuckDB VectorOperations::Hash semantics
 * (MurmurHash64 finalizer; int32 zero-extended through uint32; NULL rows hash to NULL_HASH).
 *
 * Key columns follow DuckDB's Vector model (see rpt_key_column):
 *   FLAT        keys[row]
 *   DICTIONARY  keys[key_sel[row]]        (validity indexed by the physical index key_sel[row])
 *   CONSTANT    flatten on the host first (PTBloomFilter's HashColumns flattens, bloom_filter.cpp:19-21)
 * Validity is DuckDB's ValidityMask layout: uint64 words, bit (i % 64) of word (i / 64) set = valid;
 * NULL pointer = all rows valid.
 *
 * Caller buffers (workspaces and outputs):
 *   - Contents on entry are ARBITRARY. A workspace may hold anything: the leftovers of another call, filter,
 *     strategy or batch size, or a fill pattern; an output buffer likewise. No entry point needs them cleared,
 *     and no result depends on what they held. (What a call leaves in its workspace is unspecified.)
 *   - Nothing outside the documented sizes is written: a workspace of exactly rpt_*_workspace_bytes() bytes,
 *     out_sel of exactly n entries, out_bits of exactly ceil(n/512)*8 words, out_count of one uint64, and an
 *     out_hashes / out array of exactly n entries are enough, with no slack behind them.
 *   - A workspace base must be 16-byte aligned (hipMalloc gives 256): other bases are rejected with
 *     RPT_ERR_INVALID_ARGUMENT before anything is launched. Output arrays should be 16-byte aligned as well
 *     (not checked, except by rpt_words_or and rpt_words_or_slices); out_count needs 8.
 */
#ifndef RPT_GPU_H
#define RPT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPT_GPU_ABI_VERSION 1

typedef enum rpt_status {
  RPT_OK = 0,
  RPT_ERR_INVALID_ARGUMENT = 1, /* null handle/pointer, bad key type, n too large for uint32 sel */
  RPT_ERR_HIP = 2,              /* a HIP runtime call failed; rpt_last_error() has the text */
  RPT_ERR_OUT_OF_MEMORY = 3,    /* device allocation failed */
  RPT_ERR_WORKSPACE = 4,        /* caller workspace smaller than rpt_probe_workspace_bytes() */
  RPT_ERR_SHAPE_MISMATCH = 5,   /* merge of filters with different log_num_blocks / devices */
  RPT_ERR_COLLECTIVE = 6,       /* librccl could not be loaded, or an RCCL call failed */
  RPT_ERR_COMM_ABORTED = 7      /* an OR all-reduce failed after its first collective call and ABORTED the
                                   communicator (ncclCommAbort freed it: never use or destroy it again) */
} rpt_status;

typedef enum rpt_key_type {
  RPT_KEY_I64 = 0,  /* BIGINT / int64 keys */
  RPT_KEY_I32 = 1,  /* INTEGER / int32 keys (JOB join keys) */
  RPT_KEY_HASH = 2  /* pre-computed 64-bit hashes (HashColumns output); validity/NULLs not applied */
} rpt_key_type;

/* How a probe reaches the filter blocks (rpt_bf_set_probe_strategy). All give identical results. */
typedef enum rpt_probe_strategy {
  RPT_PROBE_AUTO = 0,        /* by filter and batch size (measured crossovers): LDS (<= 128 KiB, and
                                256 / 512 KiB for n >= 4 Mi, 1 MiB for 4 Mi <= n < 32 Mi);
                                PARTITIONED (<= 128 MiB) for n >= 32 Mi (256 KiB..2 MiB) or n >= 4 Mi
                                (4 MiB and up); BUCKETED (<= 16 GiB, n >= max(blocks/8, 32 Mi));
                                otherwise GATHER */
  RPT_PROBE_GATHER = 1,      /* one random 8-byte gather per key from L2 / Infinity Cache / HBM */
  RPT_PROBE_LDS = 2,         /* filter staged in each workgroup's LDS: whole (<= 128 KiB), or its first 128 KiB
                                with the rest gathered from L2 (256 KiB .. 1 MiB) */
  RPT_PROBE_PARTITIONED = 3, /* rows bucketed per 16 Ki-row tile by 128 KiB filter slice; each slice is
                                probed from LDS, then row order is restored (filters 128 KiB..128 MiB) */
  RPT_PROBE_BUCKETED = 4     /* two levels: rows first bucketed by 32 MiB filter region into contiguous
                                hash arrays, then PARTITIONED per region (filters 32 MiB..16 GiB) */
} rpt_probe_strategy;

/* How an insert reaches the filter (rpt_bf_set_insert_strategy). All give identical filters. */
typedef enum rpt_insert_strategy {
  RPT_INSERT_AUTO = 0,        /* by filter and batch size (measured crossovers): PARTITIONED (<= 128 MiB,
                                 n >= 1 Mi), BUCKETED (larger, n >= max(blocks/16, 8 Mi)), else ATOMIC */
  RPT_INSERT_ATOMIC = 1,      /* one device-scope 64-bit atomic OR per key */
  RPT_INSERT_PARTITIONED = 2, /* rows bucketed by 128 KiB filter slice; each slice ORed in LDS, then
                                 merged with coalesced atomic ORs (filters 128 KiB..128 MiB) */
  RPT_INSERT_BUCKETED = 3     /* two levels as RPT_PROBE_BUCKETED (filters 32 MiB..16 GiB) */
} rpt_insert_strategy;

/* A hipStream_t, passed opaquely so this header needs no HIP include. NULL = the null stream. */
typedef void* rpt_stream_t;

/* Opaque filter handle: owns its device memory (PTBloomFilter + its BufferManager allocation,
 * bloom_filter.hpp:27-28,56; bloom_filter.cpp:27-32). */
typedef struct rpt_bf rpt_bf;

/* A key column on the device (DuckDB Vector shape; see header comment). */
typedef struct rpt_key_column {
  int32_t key_type;         /* rpt_key_type */
  const void* keys;         /* device pointer */
  const uint32_t* key_sel;  /* device pointer or NULL (DICTIONARY selection) */
  const uint64_t* validity; /* device pointer or NULL (all valid) */
} rpt_key_column;

typedef struct rpt_bf_info {
  int32_t device;          /* HIP device ordinal the words live on */
  int32_t log_num_blocks;  /* filter has 2^log_num_blocks uint64 blocks */
  uint64_t num_blocks;
  uint64_t sized_for_rows; /* PTBloomFilter::SizedForRows (bloom_filter.hpp:41-43) */
  int32_t has_data;        /* !PTBloomFilter::IsEmpty (bloom_filter.hpp:45-47) */
  int32_t finalized;       /* PTBloomFilter::finalized_ (bloom_filter.hpp:30) */
  uint64_t* words;         /* device pointer to the blocks (after rpt_bf_clear they read as zero only once
                              another operation on the filter has run: see rpt_bf_clear) */
} rpt_bf_info;

/* ---- library ---------------------------------------------------------------------------- */
int rpt_abi_version(void);
const char* rpt_status_string(int status);
/* Text of the last error raised on the calling thread ("" if none). */
const char* rpt_last_error(void);

/* ---- host-only sizing rules (no device work) ----------------------------------------------- */
/* log2 of the block count for a filter sized for n rows: log2ceil(max(512, 8n)) - 6 (Arrow
 * BlockedBloomFilter::CreateEmpty; the filter PTBloomFilter::Initialize allocates, bloom_filter.cpp:27-32). */
int rpt_bf_log_num_blocks_for_rows(uint64_t n_rows);
/* PhysicalCreateBF::Finalize resize rule, verbatim (physical_create_bf.cpp:394-398):
 * 1 iff actual_rows > 0 and actual_rows*8 > NextPow2(max(512, sized_for_rows*12)). */
int rpt_bf_needs_resize(uint64_t sized_for_rows, uint64_t actual_rows);
/* The resize predicate CREATE_BF's Finalize applies here: the reference's stated intent ("resize iff
 * allocated_bits / actual_rows < 8", physical_create_bf.cpp:383) evaluated on the filter actually
 * allocated (64 * 2^log_num_blocks bits, Arrow sizing at 8 bits per estimated row): 1 iff
 * actual_rows * 8 > 64 << log_num_blocks. The verbatim rule above assumes DuckDB's native 12-bit
 * allocation and would leave an Arrow-sized filter at 4 bits per key (sized_for 1000, actual 2048);
 * DESIGN.md §2. Negative rpt_status on error. */
int rpt_bf_needs_resize_alloc(const rpt_bf* bf, uint64_t actual_rows);
/* Device workspace a probe of n rows against a 2^log_num_blocks-block filter needs, for any
 * strategy (bytes, 256-aligned). rpt_bf_probe_workspace_bytes: for the strategy a probe of n rows
 * of this filter runs now (AUTO resolved), usually far less for very large filters. */
size_t rpt_probe_workspace_bytes(uint64_t n_rows, int log_num_blocks);

/* ---- lifecycle --------------------------------------------------------------------------- */
/* PTBloomFilter::Initialize(context, est_num_rows) (bloom_filter.cpp:27-32): allocate and zero a
 * filter sized for est_num_rows on `device`. Synchronous. */
int rpt_bf_create(int device, uint64_t est_num_rows, rpt_bf** out);
/* Same with an explicit size (2^log_num_blocks blocks, 0 <= log_num_blocks <= 40). */
int rpt_bf_create_log_blocks(int device, int log_num_blocks, rpt_bf** out);
int rpt_bf_destroy(rpt_bf* bf);
int rpt_bf_get_info(const rpt_bf* bf, rpt_bf_info* out);
/* First half of PTBloomFilter::ReinitializeAndRehash (bloom_filter.cpp:34-43): reallocate for
 * actual_rows, zero, sized_for_rows = actual_rows, has_data = 0. The caller then re-inserts the
 * materialized rows with rpt_bf_insert. Synchronous. */
int rpt_bf_reinitialize(rpt_bf* bf, uint64_t actual_rows);
/* PTBloomFilter::finalized_ = value (physical_create_bf.cpp:409-413). */
int rpt_bf_set_finalized(rpt_bf* bf, int value);
/* Select the probe strategy (rpt_probe_strategy); rpt_bf_probe_strategy returns the one a probe
 * will run now (AUTO resolved), or a negative status. */
int rpt_bf_set_probe_strategy(rpt_bf* bf, int strategy);
/* 1 if `strategy` can probe a 2^log_num_blocks-block filter, else 0. */
int rpt_probe_strategy_supported(int strategy, int log_num_blocks);
int rpt_bf_probe_strategy(const rpt_bf* bf);
/* The strategy a probe / insert of n rows runs now (AUTO resolved with n), or a negative status. */
int rpt_bf_probe_strategy_for(const rpt_bf* bf, uint64_t n_rows);
int rpt_bf_insert_strategy_for(const rpt_bf* bf, uint64_t n_rows);
size_t rpt_bf_probe_workspace_bytes(const rpt_bf* bf, uint64_t n_rows);
/* Zero every block and clear has_data (stream-ordered). The zeroing is deferred to the next operation on
 * the filter: a partitioned / bucketed insert that owns every slice stores the slices whole (so a rebuild
 * is one pass over the filter, not a memset and then the insert's stores); any other insert, merge,
 * probe, copy or export zeroes the words first, ordered like any other write. Only a direct read through
 * rpt_bf_info::words can see the words before that. */
int rpt_bf_clear(rpt_bf* bf, rpt_stream_t stream);
/* Settle a deferred clear now: zero the words on `stream` and wait until that zeroing has completed (a
 * no-op if no clear is pending). Needed before a stream capture (graph) reads or writes a cleared filter:
 * a read or write inside a capture that would have to settle the clear is refused with
 * RPT_ERR_INVALID_ARGUMENT (the zeroing would be replayed with the graph, wiping what was inserted between
 * replays). Synchronous.
 * Stream capture in general: probes capture freely once no clear is pending. A write (insert, merge, copy
 * into the filter) captures when no clear is pending and the filter's previous write has completed
 * (otherwise RPT_ERR_INVALID_ARGUMENT: synchronize first); a captured insert merges with atomics, so each
 * replay ORs its keys in whatever the filter holds by then, and replays are ordered by the stream the
 * graph is launched on (a captured write takes no part in the filter's cross-stream write order).
 * rpt_bf_clear and rpt_bf_allreduce_or[_ws] are refused inside a capture. Any capture mode works: the one event
 * query a captured write makes runs with the thread's capture mode relaxed around it. Under
 * hipStreamCaptureModeGlobal (torch.cuda.graph's default) no thread of the process may make an unsafe HIP call
 * while the capture is open, and rpt_bf_destroy / rpt_bf_create / rpt_bf_reinitialize are such calls (hipFree /
 * hipMalloc): create and destroy filters outside capture windows (collect garbage that may hold filters first,
 * as torch.cuda.graph does). */
int rpt_bf_settle(rpt_bf* bf, rpt_stream_t stream);

/* ---- build ------------------------------------------------------------------------------- */
/* PTBloomFilter::Insert (bloom_filter.cpp:70-78): hash each of n rows of `col` and OR its mask into
 * its block with a device-scope atomic OR. Thread-safe: any number of host threads / streams may
 * insert into one filter concurrently (parallel Sink, physical_create_bf.hpp:43-45). n == 0 is a
 * no-op; otherwise has_data becomes 1. */
int rpt_bf_insert(rpt_bf* bf, const rpt_key_column* col, uint64_t n, rpt_stream_t stream);

/* rpt_bf_insert with a caller workspace, which enables the partitioned / bucketed inserts for large
 * batches (same result, same thread-safety). workspace: rpt_insert_workspace_bytes(n,
 * log_num_blocks) bytes of device memory (the largest any insert strategy needs; 0 when the filter
 * only supports atomic inserts), or rpt_bf_insert_workspace_bytes(bf, n) for the strategy this
 * insert will run (0 = atomic, no workspace needed). The workspace is 16-byte aligned and may hold anything on
 * entry (see "Caller buffers" above). */
size_t rpt_insert_workspace_bytes(uint64_t n_rows, int log_num_blocks);
size_t rpt_bf_insert_workspace_bytes(const rpt_bf* bf, uint64_t n_rows);
int rpt_bf_insert_ws(rpt_bf* bf, const rpt_key_column* col, uint64_t n, void* workspace, size_t workspace_bytes,
                     rpt_stream_t stream);
int rpt_bf_set_insert_strategy(rpt_bf* bf, int strategy);

/* Min/max dynamic filter (PhysicalCreateBF::Sink/Combine, physical_create_bf.cpp:82-176, 229-272;
 * pushed as >= min / <= max scan filters at :335-345): every insert of an I32/I64 column also folds
 * the min and max of its valid (non-NULL) key values into the filter, fused into the insert kernels
 * (HASH columns carry no values and are skipped). I32 values are sign-extended. Reset by
 * rpt_bf_create / rpt_bf_clear / rpt_bf_reinitialize; rpt_bf_merge_or merges them. get: stream-ordered
 * read, then synchronizes `stream`; *out_has_value = 0 (and min = max = 0) when no valid key was
 * inserted. set: overwrite (the multi-GPU merge writes the all-reduced values back). */
int rpt_bf_get_minmax(const rpt_bf* bf, int64_t* out_min, int64_t* out_max, int* out_has_value, rpt_stream_t stream);
int rpt_bf_set_minmax(rpt_bf* bf, int64_t min_value, int64_t max_value, int has_value, rpt_stream_t stream);

/* ---- probe ------------------------------------------------------------------------------- */
/* PTBloomFilter::LookupSel (bloom_filter.cpp:60-68) for a batch of rows: writes the ids of rows
 * whose key may be in the filter to out_sel in ASCENDING order and the survivor count to
 * *out_count_dev (device uint64). Rows are 0..n-1, or row_sel[0..n) when row_sel != NULL (the
 * already-sliced chunk of PhysicalUseBF's multi-filter loop, physical_use_bf.cpp:137-183); the
 * written ids are then the row_sel values. n must be < 2^32 (sel_t is uint32). out_sel capacity n.
 * workspace: device memory of rpt_probe_workspace_bytes(n, log_num_blocks) bytes (or rpt_bf_probe_workspace_bytes),
 * 16-byte aligned, holding anything on entry (see "Caller buffers" above), exclusively owned by this call
 * until it completes on `stream`. Batches of at most RPT_SMALL_PROBE_ROWS rows under the AUTO strategy
 * run one fused single-workgroup kernel (probe + compaction: one launch instead of four) and leave
 * the workspace untouched. */
#define RPT_SMALL_PROBE_ROWS 16384
/* 1 if rpt_bf_probe of n_rows rows runs the fused small-batch kernel now (AUTO strategy, 1 <= n_rows <=
 * RPT_SMALL_PROBE_ROWS), else 0; negative rpt_status on error. Its key, validity, row_sel and output
 * buffers may then be device-mapped pinned host memory (hipHostGetDevicePointer): one launch and no
 * copies per call. */
int rpt_bf_probe_is_fused(const rpt_bf* bf, uint64_t n_rows);
int rpt_bf_probe(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n,
                 uint32_t* out_sel, uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                 rpt_stream_t stream);
/* PhysicalUseBF::ExecuteInternal's filter chain (physical_use_bf.cpp:127-179: each LookupSel over the rows
 * the previous filters kept, i.e. the AND of the filters) over one small batch in ONE launch: out_sel gets
 * the ascending ids of the rows that pass every filters[i], probed on its own key column cols[i] (each
 * column may have its own key type, dictionary, validity), and *out_count_dev their count. Rows are
 * 0..n-1, or row_sel[0..n) as in rpt_bf_probe. 1 <= n_filters <= RPT_MAX_CHAIN, n <= RPT_SMALL_PROBE_ROWS,
 * every filter on one device; no workspace. The skips and early exits of the reference loop (a filter not
 * yet finalized is skipped, an empty filter passes nothing) are the caller's: pass the filters that
 * apply. Buffers may be device-mapped pinned host memory, as for the fused rpt_bf_probe. */
#define RPT_MAX_CHAIN 8
int rpt_bf_probe_chain(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                       const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                       rpt_stream_t stream);
/* rpt_bf_probe_chain for batches of any size (n < 2^32): same arguments, same result (ascending ids of the
 * rows that pass every filters[i] on cols[i]; *out_count_dev their count), plus a caller workspace. What a
 * device-resident USE_BF calls for a large batch instead of one rpt_bf_probe per filter with the count read
 * back in between.
 * Filters and columns: 1..RPT_MAX_CHAIN filters, all on one device; each column has its own key type (I64 / I32 /
 *   HASH), dictionary and validity; row_sel works as in rpt_bf_probe (every filter probes rows row_sel[0..n), the
 *   ids written are the row_sel values). The result equals the reference loop's (each LookupSel over the previous
 *   survivors) and does not depend on the order of the filters.
 * Ordering and capture: fully stream-ordered: no host synchronisation, no device-to-host copy, no allocation. It
 *   captures into a stream capture under the rules of rpt_bf_probe (rpt_bf_settle above): every filter's deferred
 *   clear is settled first, as rpt_bf_probe_chain does, so a pending one is refused inside a capture with
 *   RPT_ERR_INVALID_ARGUMENT before anything is enqueued.
 * Strategies: filter i runs the strategy rpt_bf_probe_strategy_for(filters[i], n) reports (rpt_bf_set_probe_strategy
 *   is honoured per filter). The survivors stay on the device as result bits (the layout of rpt_bf_probe_bits) plus
 *   one count per 512-row segment: filter 0 runs its phase 1 into them; a later GATHER / LDS filter runs a masked
 *   probe over them in place (a 512-row segment with no survivor loads no key and touches no filter word; a dead
 *   row of a live segment makes no global gather); a later PARTITIONED / BUCKETED filter runs its phase 1 over all
 *   n rows into a temporary bits array, which is then ANDed in (dead rows are partitioned too: routing only the
 *   survivors would need their count on the host); one phase 2 at the end writes out_sel and the count.
 *   When 1 <= n <= RPT_SMALL_PROBE_ROWS and every filter is on RPT_PROBE_AUTO the call hands over to
 *   rpt_bf_probe_chain's one-launch kernel and leaves the workspace untouched; with any strategy forced it takes
 *   the path above even at n = 1.
 * Caller buffers ("Caller buffers" at the top): the workspace may hold anything on entry; exactly
 *   rpt_bf_probe_chain_workspace_bytes(filters, n_filters, n) bytes are enough, as are out_sel of exactly n entries
 *   and out_count_dev of one uint64; nothing outside these is written. A workspace that is not 16-byte aligned
 *   returns RPT_ERR_INVALID_ARGUMENT, one that is too small RPT_ERR_WORKSPACE, both before any launch.
 * Edge cases: n == 0 sets the count to 0 (stream-ordered) and does nothing else. n >= 2^32, n_filters outside
 *   1..RPT_MAX_CHAIN, a null filter or column, a null out_sel with n > 0, or filters on different devices return
 *   RPT_ERR_INVALID_ARGUMENT. An empty filter passes nothing (its words are zero).
 * rpt_bf_probe_chain_workspace_bytes: the device workspace these filters (their strategies resolved for n_rows) and
 *   n_rows rows need; 256-aligned; 0 on a null / invalid argument. Host-only. */
size_t rpt_bf_probe_chain_workspace_bytes(const rpt_bf* const* filters, uint32_t n_filters, uint64_t n_rows);
int rpt_bf_probe_chain_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                          const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                          void* workspace, size_t workspace_bytes, rpt_stream_t stream);
/* rpt_bf_probe in its two stream-ordered phases (same filter, workspace and stream), for callers that
 * time or overlap them. GATHER / LDS: phase 1 = hash + gather + result bits + per-segment counts,
 * phase 2 = scan + expansion into out_sel. PARTITIONED: phase 1 = partition rows by filter slice +
 * probe each slice from LDS + restore row order into the result bits, phase 2 = as above.
 * (rpt_bf_probe itself runs the PARTITIONED strategy without the result bits: per-tile survivor counts
 * give each tile's offset and the row-order restore writes out_sel directly. Same sel and count.) */
int rpt_bf_probe_phase1(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n,
                        void* workspace, size_t workspace_bytes, rpt_stream_t stream);
int rpt_bf_probe_phase2(const rpt_bf* bf, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                        uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
/* rpt_bf_probe's result as bits instead of a selection vector: bit i (LSB-first in uint64 words) of out_bits = the
 * i-th probed row (row i, or row_sel[i]) passes; out_bits (device memory) holds ceil(n/512)*8 words, bits past n
 * are 0. Same strategies and workspace (rpt_bf_probe_workspace_bytes) as rpt_bf_probe; stream-ordered, no sync. A
 * host-resident caller copies n/8 bytes back instead of 4 bytes per survivor (the C++ host mirror's pipelined
 * lookups do, DeviceContext::bits_back). */
int rpt_bf_probe_bits(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n,
                      uint64_t* out_bits, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
/* Arrow BlockedBloomFilter::Find(…, result_bit_vector) shape: bit i (LSB-first in uint64 words) of
 * out_bits = row i passes. out_bits must hold ceil(n/512)*8 words. */
int rpt_bf_find_bits(const rpt_bf* bf, const rpt_key_column* col, uint64_t n, uint64_t* out_bits,
                     rpt_stream_t stream);
/* Key hashes exactly as the filter sees them (DuckDB HashColumns restatement). */
int rpt_hash_keys(const rpt_key_column* col, uint64_t n, uint64_t* out_hashes, rpt_stream_t stream);
/* HashColumns' CombineHash step for composite keys (bloom_filter.cpp:15-17): inout_hashes[i] =
 * CombineHashScalar(inout_hashes[i], Hash(row i of col)) with DuckDB v1.1+'s form (a ^= a >> 32;
 * a *= 0xd6e8feb86659fd93; a ^ b; restated, parity unpinned). rpt_hash_keys(col_0) followed by
 * rpt_hash_combine(col_j) for j = 1, 2, ... is the composite-key hash; insert / probe it as an
 * RPT_KEY_HASH column. */
int rpt_hash_combine(const rpt_key_column* col, uint64_t n, uint64_t* inout_hashes, rpt_stream_t stream);
/* Narrow BIGINT keys (device memory): out[r] = (uint64_t)chunk_hi[c] << 32 | lo[r] for the rows r of chunk c,
 * [chunk_row0[c], chunk_row0[c + 1]), c < n_chunks (chunk_row0 ascending; out and lo hold chunk_row0[n_chunks]
 * entries). A host-resident batch whose chunks each share their keys' high 32 bits crosses PCIe as 4-B low words
 * plus one high word per chunk and is widened here before the insert / probe (the C++ host mirror does this by
 * itself). Stream-ordered; n_chunks == 0 is a no-op. */
int rpt_keys_widen(const uint32_t* lo, const uint32_t* chunk_hi, const uint32_t* chunk_row0, uint64_t n_chunks,
                   uint64_t* out, rpt_stream_t stream);

/* ---- transfer: a probe's survivors into the next filter, on the device --------------------------- */
/* Predicate transfer chains the two halves: a table is reduced by the filters that reach it (USE_BF,
 * physical_use_bf.cpp:127-179), and the rows that survive are inserted into the filter the table sends on
 * (CREATE_BF's Sink, physical_create_bf.cpp:201-242; PTBloomFilter::Insert, bloom_filter.cpp:70-78). The probes
 * above leave their survivors on the device (result bits, or out_sel and *out_count_dev); these inserts take their
 * row set from there, so the step needs no synchronisation and no count on the host, and captures into a graph.
 *
 * rpt_bf_insert_bits: insert the rows i < n of col (row i, or row_sel[i]) whose bit i is set in row_bits (the
 *   layout of rpt_bf_probe_bits: ceil(n/512)*8 words of device memory, LSB first; bits at positions >= n are
 *   ignored). A 512-row segment without a set bit loads no key.
 * rpt_bf_insert_sel: insert rows sel[0 .. min(*count_dev, max_rows)) of col. The count is read on the device when
 *   the kernel runs (what rpt_bf_probe / rpt_bf_probe_chain[_ws] left in *out_count_dev, earlier on the stream);
 *   max_rows is the capacity of sel (it sizes the launch and clamps the count); no sel entry at or past the clamped
 *   count is read. sel holds row ids of col (dictionary columns: key_sel[sel[i]]).
 * rpt_bf_transfer_ws: rpt_bf_probe_chain_ws(filters, cols, ..., out_sel, out_count_dev, workspace), then the
 *   survivors inserted into dst_filters[j] on its own key column dst_cols[j], j < n_dst (1..RPT_MAX_CHAIN
 *   destinations). Arguments, result and workspace (rpt_bf_probe_chain_workspace_bytes; the inserts need none) are
 *   rpt_bf_probe_chain_ws's. On the workspace path the destinations are fed from the accumulated result bits, on
 *   the small-batch hand-over (n <= RPT_SMALL_PROBE_ROWS, every probed filter on AUTO) from out_sel and the count;
 *   either way row row_sel[i] (or i) of dst_cols[j] is inserted iff it passed every probed filter. Every
 *   destination must be on the chain's device and none may be one of filters[] (RPT_ERR_INVALID_ARGUMENT); these
 *   and the destinations' capture checks run before anything is enqueued. n == 0 sets the count to 0 and touches
 *   no destination.
 *
 * All three: the filter ends up bit-identical to rpt_bf_insert of exactly the selected rows (ORed into what it
 *   holds; the min/max of the selected valid I32/I64 keys folded in; a selected NULL row inserts NULL_HASH). One
 *   atomic OR per row, whatever the filter's insert strategy (the *_ws variants below route).
 *   Stream-ordered: no synchronisation, no copy back, no allocation. Writes follow rpt_bf_insert's rules
 *   (rpt_bf_settle above): ordered after the filter's previous write; a deferred clear is settled first outside a
 *   capture and refused inside one; a captured call ORs its rows at every replay.
 * has_data becomes 1 whenever n / max_rows > 0, even if the selection turns out empty: the host cannot know. That
 *   is result-neutral (an all-zero filter passes nothing); a caller that later reads a zero count may restore
 *   IsEmpty with rpt_bf_set_has_data(bf, 0).
 * n == 0 / max_rows == 0 is a no-op. A null filter, column, keys, row_bits, sel or count_dev, n or max_rows >= 2^32,
 *   or a bad key type return RPT_ERR_INVALID_ARGUMENT before any launch. */
int rpt_bf_insert_bits(rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n,
                       const uint64_t* row_bits, rpt_stream_t stream);
int rpt_bf_insert_sel(rpt_bf* bf, const rpt_key_column* col, const uint32_t* sel, const uint64_t* count_dev,
                      uint64_t max_rows, rpt_stream_t stream);
int rpt_bf_transfer_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                       rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                       const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                       void* workspace, size_t workspace_bytes, rpt_stream_t stream);

/* The same three with the destination's insert strategy honoured (rpt_bf_insert_strategy_for(bf, n) resolved with
 * n / max_rows, the only row count the host has; rpt_bf_set_insert_strategy is honoured):
 *   PARTITIONED  a partition pass over all n rows in which a row that is not selected emits no record (a 512-row
 *                segment without a selected row loads no key; a tile without one stores no record), then
 *                rpt_bf_insert_ws's run-table transpose and LDS slice merge. No count reaches the host: the tile
 *                geometry depends on n only. Needs rpt_bf_insert_workspace_bytes(bf, n) bytes of device workspace
 *                (16-byte aligned; contents on entry do not matter; nothing past that size is written). Too small:
 *                RPT_ERR_WORKSPACE; misaligned: RPT_ERR_INVALID_ARGUMENT; both before any launch.
 *   ATOMIC, BUCKETED  the calls above, one atomic OR per row; the workspace is not looked at and may be null. A
 *                bucketed masked insert does not exist: its level 1 sizes lists from the row count and would need a
 *                second design.
 * The result, has_data, the argument checks and the write rules are those of the calls above; the slice merge picks
 * its mode as rpt_bf_insert_ws does (every slice stored whole under a deferred clear, plain stores into a pristine
 * filter, else adaptive; atomics when a slice is split over workgroups or the call is captured).
 * rpt_bf_transfer_insert_ws: rpt_bf_transfer_ws with one more workspace, shared by the destinations, which run one
 *   after another on the stream: a destination that resolves to PARTITIONED for n takes the routed insert from the
 *   accumulated result bits, the others one atomic OR per row. rpt_bf_transfer_insert_workspace_bytes returns the
 *   largest need over the destinations (0 if none routes, and 0 on null / invalid arguments). The small-batch
 *   hand-over is rpt_bf_transfer_ws's (from out_sel, one atomic OR per row; the insert workspace is checked all the
 *   same). Every destination check runs before the chain enqueues anything. insert_workspace must not overlap
 *   workspace. Callers pick the entry point: nothing switches between the two by survivor fraction. */
int rpt_bf_insert_bits_ws(rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n,
                          const uint64_t* row_bits, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
int rpt_bf_insert_sel_ws(rpt_bf* bf, const rpt_key_column* col, const uint32_t* sel, const uint64_t* count_dev,
                         uint64_t max_rows, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
size_t rpt_bf_transfer_insert_workspace_bytes(rpt_bf* const* dst_filters, uint32_t n_dst, uint64_t n_rows);
int rpt_bf_transfer_insert_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                              rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                              const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                              void* workspace, size_t workspace_bytes, void* insert_workspace,
                              size_t insert_workspace_bytes, rpt_stream_t stream);

/* The min/max range stage: the other half of CREATE_BF's dynamic filter, on the device. The reference pushes a
 * filter's Bloom test and ">= min" / "<= max" of its build keys to the probe side's scan (PushDynamicFilters,
 * physical_create_bf.cpp:282-350; rpt_filter_type all / bf_only / minmax_only). The inserts here fold that min/max
 * into the filter on the device (rpt_bf_get_minmax); these calls test keys against it there, reading the range from
 * device memory when the kernel runs: no host copy of the range, no synchronisation, and a captured call sees at
 * every replay the min/max the filter holds by then.
 * The test, per probed row i < n (row i, or row_sel[i]) of an I64 / I32 column (I32 values sign-extended, as the
 * inserts fold them):
 *   the filter has a value (min <= max): the row passes iff its key is not NULL and min <= key <= max (a NULL fails,
 *     as it fails the scan's ">= min");
 *   it has none (no valid key was ever inserted, or rpt_bf_set_minmax(.., has_value = 0)): every row passes, NULL
 *     rows included: the reference pushes no min/max filter then (physical_create_bf.cpp:335).
 *
 * rpt_bf_range_bits: the range test alone (minmax_only). out_bits has the layout of rpt_bf_probe_bits
 *   (ceil(n/512)*8 words of device memory, bits at positions >= n are 0; nothing else is written), so it composes
 *   with rpt_bf_insert_bits. No workspace; stream-ordered. The filter's deferred clear is settled as a probe settles
 *   it (refused inside a capture: rpt_bf_settle first). n == 0 is a no-op; a HASH column (no key values), a null
 *   argument or n >= 2^32 return RPT_ERR_INVALID_ARGUMENT.
 * rpt_bf_probe_chain_range_ws, rpt_bf_transfer_range_ws, rpt_bf_transfer_insert_range_ws: rpt_bf_probe_chain_ws,
 *   rpt_bf_transfer_ws and rpt_bf_transfer_insert_ws restricted to the rows that also pass the range test of every
 *   flagged filter on its own column: bit f of range_mask flags filters[f] / cols[f] (all ones up to n_filters:
 *   rpt_filter_type all). out_sel, the count, the destinations' words and min/max, has_data, and the argument,
 *   capture and write rules follow from that; the result does not depend on the order of the filters.
 *   range_mask == 0: each call is exactly its twin without the argument (small-batch hand-over included) and the
 *     workspace function returns rpt_bf_probe_chain_workspace_bytes.
 *   range_mask != 0, stage order (fixed; nothing switches on strategy or data): the flagged columns' range stages in
 *     filter order, the first writing the accumulated result bits and per-segment counts, the others ANDing into them
 *     in place; then every filter, filter 0 included, as a later stage of rpt_bf_probe_chain_ws (a masked GATHER / LDS
 *     probe that skips dead 512-row segments and dead rows' gathers; or, for a PARTITIONED / BUCKETED filter, its
 *     phase 1 over all n rows into the temporary bits, then the AND); then the selection-vector tail once; then the
 *     inserts from the bits. Each filter's strategy is rpt_bf_probe_strategy_for(filters[f], n), as in the chain.
 *     There is no small-batch hand-over: every n >= 1 takes the workspace path (the one-launch form for
 *     n <= RPT_SMALL_PROBE_ROWS is rpt_bf_probe_chain_range below, which the caller picks).
 *   Cost: the range pass reads each flagged key column once more than the plain chain does (the filter's own stage
 *     reads the keys of the live segments again), and a routed filter 0 pays what a routed later stage pays today:
 *     its phase 1 partitions all n rows, dead ones included, plus the AND pass.
 *   When to use (measured, one filter, int64 ids, range call / plain call; DESIGN §5 "Min/max range stage"): the
 *     range pass streams the whole key column at 0.95 of the box's read-stream rate, which is also about what an
 *     LDS-sized filter's own probe costs, so in front of a cheap stage it does not pay for itself: a 128 KiB filter
 *     takes 1.1-2.2x the plain chain's time (1.26x even when a sorted column's range covers 5 % of 2^27 rows and 95 %
 *     of the segments die), and a routed (PARTITIONED / BUCKETED) filter, which partitions all n rows whatever is
 *     dead, takes 1.2-1.4x. It pays in front of a stage that costs more per row than a stream: a gathered filter
 *     (16 MiB at 2^20 rows) takes 0.71-0.77x when the range covers 5 % of the column, sorted or shuffled (dead rows
 *     make no gather), 0.95x at 50 %, 1.04x at 100 %. Set the bit where the rows the range removes would otherwise
 *     be gathered (or where its exact answer matters: it removes the filter's false positives outside the range
 *     from out_sel and from the destinations); leave it clear for LDS-sized and routed filters until the range
 *     test is fused into stage 0's key read (a follow-up). Nothing is dispatched on this: the caller chooses by
 *     setting the mask.
 *   Workspace: rpt_bf_probe_chain_range_workspace_bytes(filters, n_filters, range_mask, n): the chain's layout with
 *     the temporary bits present whenever any filter routes, filter 0 included; 0 on a null / invalid argument (a
 *     mask bit at or above n_filters among them). "Caller buffers" at the top holds: contents on entry are arbitrary,
 *     exactly the reported size (and out_sel of exactly n entries) is enough, a misaligned workspace returns
 *     RPT_ERR_INVALID_ARGUMENT and a too-small one RPT_ERR_WORKSPACE, both before any launch.
 *   Arguments: a mask bit at or above n_filters, or a flagged HASH column, returns RPT_ERR_INVALID_ARGUMENT before
 *     any launch (and before any handle is looked into); n == 0 sets the count to 0 and does nothing else.
 *   Capture: under rpt_bf_probe_chain_ws's rules (transfers: rpt_bf_transfer_ws's). */
int rpt_bf_range_bits(const rpt_bf* bf, const rpt_key_column* col, const uint32_t* row_sel, uint64_t n,
                      uint64_t* out_bits, rpt_stream_t stream);
size_t rpt_bf_probe_chain_range_workspace_bytes(const rpt_bf* const* filters, uint32_t n_filters, uint32_t range_mask,
                                                uint64_t n_rows);
int rpt_bf_probe_chain_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                uint32_t range_mask, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                                uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
int rpt_bf_transfer_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                             uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                             uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                             uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
int rpt_bf_transfer_insert_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                    uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                                    uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                                    uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                    void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream);

/* Device-counted probes: the survivors of an earlier probe probed again, their count never reaching the host. The
 * backward pass of predicate transfer probes the rows a table kept in the forward pass; with these calls that second
 * probe (and the insert into the filter the table sends on) is enqueued behind the first with no synchronisation.
 *
 * rpt_bf_probe_chain_sel_ws: the rows probed are sel[0 .. min(*count_dev, max_rows)) of every cols[f] (dictionary
 *   columns: key_sel[sel[i]], as rpt_bf_insert_sel). The count is read on the device when the first kernel runs (what
 *   rpt_bf_probe / rpt_bf_probe_chain[_ws] / rpt_bf_transfer_ws left in *out_count_dev, earlier on the stream);
 *   max_rows is the capacity of sel: it sizes the launches and clamps the count. No sel entry at or past the clamped
 *   count is read by any kernel of the call (probe stages, tail, inserts). out_sel receives sel[i] for every position
 *   i that passes every filter, in position order (ascending when sel is); *out_count_dev their number. The result is
 *   rpt_bf_probe_chain_ws(row_sel = sel, n = the clamped count)'s, whatever the filter order; sel may hold ids in any
 *   order, with repeats.
 *   Strategies: filter f runs rpt_bf_probe_sel_strategy_for(filters[f], max_rows), which is
 *   rpt_bf_probe_strategy_for(bf, max_rows) with PARTITIONED and BUCKETED replaced by GATHER, whether AUTO resolved to
 *   them or rpt_bf_set_probe_strategy forced them (LDS, whole-filter or hybrid, stays LDS): a routed stage partitions
 *   all max_rows positions and reads every sel entry, and routing only the live prefix needs the count on the host,
 *   while a masked gather does no work past the count. Nothing switches on the survivor fraction. There is no
 *   small-batch hand-over either: max_rows does not say how many rows there are, so every size, max_rows = 1
 *   included, takes the workspace path. A caller whose max_rows is at most RPT_SMALL_PROBE_ROWS has the one-launch
 *   pair rpt_bf_probe_chain_sel / rpt_bf_transfer_sel below.
 *   Workspace: rpt_bf_probe_chain_sel_workspace_bytes(filters, n_filters, max_rows) bytes (result bits, per-segment
 *   counts and the tail's group sums and offsets for max_rows rows; no stage area, so usually far less than
 *   rpt_bf_probe_chain_workspace_bytes; 0 on null / invalid arguments), 16-byte aligned. "Caller buffers" at the top
 *   holds: the workspace may hold anything on entry, exactly the reported bytes are enough, out_sel of exactly
 *   max_rows entries is enough and nothing at or past the returned count is written; misaligned:
 *   RPT_ERR_INVALID_ARGUMENT, too small: RPT_ERR_WORKSPACE, both before any launch.
 *   Ordering: fully stream-ordered (no synchronisation, no copy to the host, no allocation); captures under
 *   rpt_bf_probe_chain_ws's rules (a pending clear of a probed filter is refused inside a capture before anything is
 *   enqueued).
 *   Aliasing: only the call's first kernel reads *count_dev, so out_count_dev == count_dev is allowed (the count is
 *   replaced by the survivors'). out_sel must not overlap sel (the two ranges of max_rows entries are compared:
 *   RPT_ERR_INVALID_ARGUMENT): the tail writes out_sel while other workgroups still read sel.
 *   max_rows == 0 sets *out_count_dev to 0 (stream-ordered, on the current device: no handle is looked into) and
 *   does nothing else. A null filter, column, keys or count_dev, a null sel or out_sel with max_rows > 0,
 *   max_rows >= 2^32, n_filters outside 1..RPT_MAX_CHAIN or filters on different devices return
 *   RPT_ERR_INVALID_ARGUMENT before any launch.
 * rpt_bf_transfer_sel_ws: the same, then the survivors inserted into dst_filters[j] on dst_cols[j], j < n_dst
 *   (1..RPT_MAX_CHAIN), from the accumulated result bits with sel as the row mapping: row sel[i] of dst_cols[j] is
 *   inserted iff position i passed every probed filter. One atomic OR per row. has_data, the destinations' write
 *   rules and checks (same device, not one of filters[], capture checks: all before the chain enqueues anything) are
 *   rpt_bf_transfer_ws's.
 * rpt_bf_transfer_insert_sel_ws: with the destinations' insert strategies honoured as rpt_bf_transfer_insert_ws does: a
 *   destination that resolves to PARTITIONED for max_rows takes the routed insert from the bits, through an insert
 *   workspace of rpt_bf_transfer_insert_workspace_bytes(dst_filters, n_dst, max_rows) bytes.
 *
 * When to use them (measured on an MI355X against the host loop "probe, synchronize, read the count,
 *   rpt_bf_probe_chain_ws(row_sel = out_sel, n = count)", DESIGN §5 "Device-counted probes"): the device-counted call
 *   is 1.2-2.0x faster per step up to 2^20 rows at every filter size and survivor fraction (it saves a round trip of
 *   about 30 us), 7-11 % faster at 2^24 rows when few rows survive or the filter fits LDS, and level at any size into a
 *   filter of up to 128 KiB; it is the only form that captures into a graph. A caller is better off with the host loop
 *   at 2^24 rows and more with half or more of the rows surviving into multi-MiB filters, where the host loop takes
 *   the partitioned probe over the survivors alone: 5-18 % faster at 2^24 rows, 1.5-1.7x at 2^27. */
int rpt_bf_probe_sel_strategy_for(const rpt_bf* bf, uint64_t max_rows);
size_t rpt_bf_probe_chain_sel_workspace_bytes(const rpt_bf* const* filters, uint32_t n_filters, uint64_t max_rows);
int rpt_bf_probe_chain_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                              const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                              uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
int rpt_bf_transfer_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                           rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                           const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                           uint64_t* out_count_dev, void* workspace, size_t workspace_bytes, rpt_stream_t stream);
int rpt_bf_transfer_insert_sel_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                  rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                                  const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                                  uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                  void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream);

/* The device-counted probes for small batches: rpt_bf_probe_chain_sel_ws and rpt_bf_transfer_sel_ws in ONE launch of one
 * workgroup, with no workspace, for max_rows <= RPT_SMALL_PROBE_ROWS: what a per-vector backward step calls (a DuckDB
 * vector of 2048 rows, or a few of them, whose rows an earlier probe left on the device). They are to the _ws pair what
 * rpt_bf_probe_chain is to rpt_bf_probe_chain_ws.
 *
 * Result: rpt_bf_probe_chain_sel_ws's / rpt_bf_transfer_sel_ws's for the same arguments. out_sel receives sel[i] for
 *   every position i < min(*count_dev, max_rows) that passes every filters[f] on cols[f], in position order;
 *   *out_count_dev their number; no sel entry at or past the clamped count is read, and nothing at or past the returned
 *   count is written to out_sel (max_rows entries are enough). rpt_bf_transfer_sel: each dst_filters[j] ends
 *   bit-identical to rpt_bf_insert of exactly those rows of dst_cols[j], ORed into what it holds, the min/max of the
 *   selected valid I32/I64 keys folded in, a selected NULL row inserting NULL_HASH; has_data becomes 1 whenever
 *   max_rows > 0, as for rpt_bf_transfer_sel_ws. A destination may be listed more than once (with different columns).
 * Strategy: the kernel gathers every filter from L2, as rpt_bf_probe_chain does, and inserts with one atomic OR per
 *   row: rpt_bf_set_probe_strategy of the probed filters and the destinations' insert strategies do not matter. It
 *   works for any filter size.
 * Argument checks, in rpt_bf_probe_chain_sel_ws's order and with its messages: null lists, n_filters or n_dst outside
 *   1..RPT_MAX_CHAIN, a null handle, and a destination that is also probed (all before any handle is looked into); a
 *   null count_dev; max_rows > RPT_SMALL_PROBE_ROWS (RPT_ERR_INVALID_ARGUMENT, "exceeds RPT_SMALL_PROBE_ROWS"; 2^32 and
 *   more included); max_rows == 0 sets *out_count_dev to 0 (stream-ordered, on the current device: no handle is looked
 *   into) and does nothing else; with max_rows > 0 a null sel, a null out_sel, and out_sel overlapping sel; then
 *   filters on different devices, a bad column, a destination that is not on the chain's device. All return
 *   RPT_ERR_INVALID_ARGUMENT before any launch.
 * Aliasing: every thread of the kernel reads *count_dev before its first barrier and the count is written after a
 *   later one, so out_count_dev == count_dev is allowed (the count is replaced by the survivors'). out_sel must not
 *   overlap sel (the two ranges of max_rows entries are compared).
 * Ordering and capture: fully stream-ordered: no synchronisation, no copy, no allocation, no workspace. Every probed
 *   filter's deferred clear is settled first (refused inside a capture); every destination follows rpt_bf_insert's
 *   write rules (a deferred clear or an earlier write in flight is refused inside a capture, otherwise the call is
 *   ordered after the destination's previous write and settles its clear); all refusals come before anything is
 *   launched. The destinations' write scopes are all held across the one launch, taken in ascending handle address
 *   (a filter listed twice once), so threads that list the same destinations in different orders do not deadlock.
 * When to use them (measured on an MI355X against the _ws call with the same arguments, and against the host loop
 *   "synchronize, read the count, rpt_bf_probe_chain, one rpt_bf_insert_sel per destination"; a full vector whose sel
 *   is ascending, 1 / 3 / 8 filters of 128 KiB or 16 MiB, 0-2 destinations, 0.1-0.9 of the rows surviving; DESIGN §5
 *   "One launch for DuckDB-sized vectors"): at max_rows = 2048 the one-launch call is 1.2-3.9x faster per step than the
 *   _ws call in every shape, enqueued eagerly or replayed from a graph, and 1.6-4.7x faster than the host loop. At 8192
 *   rows it is ahead into 128 KiB filters (up to 1.57x; 4-23 % behind with one filter when 0.9 of the rows survive or two
 *   destinations are fed) and behind into 16 MiB filters (the _ws call is up to 1.8x faster; only one filter with 0.1
 *   surviving is ahead). At 16384 rows the _ws call is faster in every shape measured, 1.2-3.4x: one workgroup gathers
 *   every filter word through one CU and expands the selection with 8 lanes per wave. So: one DuckDB vector per call
 *   takes this pair; from 8192 rows on, multi-MiB filters or several destinations take the _ws pair. */
int rpt_bf_probe_chain_sel(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                           const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                           uint64_t* out_count_dev, rpt_stream_t stream);
int rpt_bf_transfer_sel(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                        rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst, const uint32_t* sel,
                        const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel, uint64_t* out_count_dev,
                        rpt_stream_t stream);

/* The min/max range in the device-counted probes and in the one-launch chains: every way of calling a chain applies
 * both halves of the dynamic filter. Each call is its twin's argument list with range_mask after n_filters (bit f flags
 * filters[f] / cols[f], as in rpt_bf_probe_chain_range_ws), and the range test is the one described at "The min/max
 * range stage" above, the range read from device memory when the kernel runs (a captured call sees at every replay the
 * min/max the filter holds by then).
 *
 * Result. The device-counted calls return exactly rpt_bf_probe_chain_range_ws(row_sel = sel, n = min(*count_dev,
 *   max_rows), range_mask)'s result: out_sel receives sel[i], in position order, for every position i that passes the
 *   range test of every flagged filter on its own column and the Bloom test of every filter; *out_count_dev their
 *   number; the transfers insert exactly those rows. rpt_bf_probe_chain_range returns rpt_bf_probe_chain_range_ws's
 *   result for the same arguments (row_sel may be null). No result depends on the order of the filters.
 * range_mask == 0: each call hands over to its twin without the argument (rpt_bf_probe_chain_sel_ws,
 *   rpt_bf_transfer_sel_ws, rpt_bf_transfer_insert_sel_ws, rpt_bf_probe_chain_sel, rpt_bf_transfer_sel,
 *   rpt_bf_probe_chain): the twin's kernels are what run and what the profiler records.
 * Everything else is the twin's, unchanged: no sel entry at or past the clamped count is read by any kernel of the call,
 *   nothing at or past the returned count is written to out_sel, out_count_dev == count_dev is allowed, out_sel
 *   overlapping sel is refused, has_data, the destinations' write rules and the capture rules; in the one-launch
 *   transfer the destinations' scopes are taken in ascending handle address and a destination may be listed twice.
 * Arguments: the twin's checks, in its order and with its messages, plus the mask's: a bit at or above n_filters and a
 *   flagged HASH column return RPT_ERR_INVALID_ARGUMENT. The mask is checked with the checks that look into no handle:
 *   for the device-counted calls before max_rows == 0 sets the count and returns, so a bad mask is refused at
 *   max_rows == 0 too, as the row-list range calls refuse it at n == 0.
 *
 * rpt_bf_probe_chain_sel_range_ws, rpt_bf_transfer_sel_range_ws, rpt_bf_transfer_insert_sel_range_ws (any
 *   max_rows < 2^32). Stage order (fixed, mirroring the _range_ws calls): the first flagged filter's range stage over
 *   sel[0 .. min(*count_dev, max_rows)), which is the only kernel of the call that reads *count_dev and writes every
 *   512-position segment's words and count (zeros past the count); the other flagged filters' range stages, masked, over
 *   all max_rows positions (the zero bits keep them away from sel); every filter, filter 0 included, as a masked later
 *   stage under rpt_bf_probe_sel_strategy_for(filters[f], max_rows) (GATHER, LDS or hybrid; PARTITIONED and BUCKETED
 *   become GATHER); the selection-vector tail once; the inserts from the bits.
 *   Workspace: rpt_bf_probe_chain_sel_workspace_bytes(filters, n_filters, max_rows) serves the ranged calls too: no
 *   stage routes, so the layout does not depend on the mask. Its contents on entry are arbitrary and exactly the
 *   reported size is enough. The insert workspace is rpt_bf_transfer_insert_workspace_bytes(dst_filters, n_dst,
 *   max_rows), as for rpt_bf_transfer_insert_sel_ws.
 * rpt_bf_probe_chain_sel_range, rpt_bf_transfer_sel_range (max_rows <= RPT_SMALL_PROBE_ROWS) and
 *   rpt_bf_probe_chain_range (the row-list form: row_sel / n as in rpt_bf_probe_chain, n <= RPT_SMALL_PROBE_ROWS): one
 *   launch of one workgroup, no workspace. A (filter, 512-position segment) item of a flagged filter loads its keys
 *   once and computes range pass and hash from that load; a row outside the range makes no filter gather. Items of
 *   unflagged filters are the twin's. The one-launch row-list transfer is rpt_bf_transfer_range, below.
 *
 * When to use them (measured on an MI355X, int64 keys, filter 0 flagged, its range covering 100 / 50 / 5 % of the probed
 *   keys, about 0.9 of the rows passing each Bloom test; DESIGN §5 "Ranges in the device-counted probes"):
 *   One launch (2048 / 8192 / 16384 positions, 1 / 3 filters of 128 KiB or 16 MiB, 0 / 1 destinations): the range test
 *     shares the key load, so where it removes nothing (100 % cover) the ranged call takes 1.00-1.03x the plain
 *     one-launch call's time, the only shapes in which it is slower; at 50 % cover 0.56-0.80x, at 5 % 0.32-0.65x (rows
 *     outside the range gather no filter word and are neither written to out_sel nor inserted). Against the ranged _ws
 *     call with the same arguments it is 1.5-4.2x faster at 2048 positions; at 8192 ahead into 128 KiB filters and, into
 *     16 MiB filters, with one filter or a 5 % range (1.2-1.4x behind with three filters otherwise); at 16384 behind (up
 *     to 2.7x) unless the range covers 5 % and the filters are 128 KiB or there is one of them. Against the host loop
 *     (synchronize, read the count, rpt_bf_probe_chain_range_ws, one rpt_bf_insert_sel per destination) 2.9-7.6x faster
 *     at 2048 positions and 1.3-4.7x at 8192. So: one DuckDB vector per call takes the one-launch calls with whatever
 *     mask the plan asks for; the size rule is the plain pair's.
 *   Workspace (2^20 / 2^24 rows, one filter): the range stage over a selection is a gather pass of its own, not a
 *     stream. Where the range removes nothing it is pure cost, 1.02x (16 MiB filter, 2^20 rows) to 1.20-1.28x (128 KiB
 *     filter) of rpt_bf_probe_chain_sel_ws; it pays once it removes rows: 0.62-0.94x at 50 % cover, 0.18-0.52x at 5 %
 *     (part of that is the rows that are not written out). Against the host loop with rpt_bf_probe_chain_range_ws over
 *     the survivors it takes 0.58-0.95x, except into the 16 MiB filter at 2^24 rows with half or more of the rows in
 *     range (1.03x, 1.23x), where the host loop gets the partitioned probe. Set the bit where the range is expected to
 *     remove rows (or where its exact answer matters); a wide range in front of an LDS-sized filter is better left clear.
 *   Nothing is dispatched on any of this: the caller sets the mask. */
int rpt_bf_probe_chain_sel_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                    uint32_t range_mask, const uint32_t* sel, const uint64_t* count_dev,
                                    uint64_t max_rows, uint32_t* out_sel, uint64_t* out_count_dev, void* workspace,
                                    size_t workspace_bytes, rpt_stream_t stream);
int rpt_bf_transfer_sel_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                 uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                                 uint32_t n_dst, const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows,
                                 uint32_t* out_sel, uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                 rpt_stream_t stream);
int rpt_bf_transfer_insert_sel_range_ws(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                        uint32_t range_mask, rpt_bf* const* dst_filters,
                                        const rpt_key_column* dst_cols, uint32_t n_dst, const uint32_t* sel,
                                        const uint64_t* count_dev, uint64_t max_rows, uint32_t* out_sel,
                                        uint64_t* out_count_dev, void* workspace, size_t workspace_bytes,
                                        void* insert_workspace, size_t insert_workspace_bytes, rpt_stream_t stream);
int rpt_bf_probe_chain_sel_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                                 uint32_t range_mask, const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows,
                                 uint32_t* out_sel, uint64_t* out_count_dev, rpt_stream_t stream);
int rpt_bf_transfer_sel_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                              uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                              uint32_t n_dst, const uint32_t* sel, const uint64_t* count_dev, uint64_t max_rows,
                              uint32_t* out_sel, uint64_t* out_count_dev, rpt_stream_t stream);
int rpt_bf_probe_chain_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                             uint32_t range_mask, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                             uint64_t* out_count_dev, rpt_stream_t stream);

/* The forward step and the sink of one vector in one launch. rpt_bf_transfer and rpt_bf_transfer_range are
 * rpt_bf_transfer_ws / rpt_bf_transfer_range_ws without `workspace, workspace_bytes`: scan -> USE_BF chain -> CREATE_BF
 * sink over a host-counted row list, one launch of one workgroup with no workspace, for n <= RPT_SMALL_PROBE_ROWS.
 * rpt_bf_insert_multi is the sink alone: one vector into one filter per build column, in one launch. With
 * rpt_bf_transfer_sel / rpt_bf_transfer_sel_range for the backward steps, every per-vector step of a forward-and-backward
 * schedule is one kernel (and one node of a captured graph).
 *
 * Result (the transfers): exactly the _ws twin's for the same arguments. out_sel receives row_sel[i] (or i), in position
 *   order, for every position i < n that passes the range test of every flagged filter on its own column and the Bloom
 *   test of every filters[f] on cols[f]; *out_count_dev their number. Each dst_filters[j] ends bit-identical to
 *   rpt_bf_insert of exactly those rows of dst_cols[j], ORed into what it holds, the min/max of the selected valid
 *   I32/I64 keys folded in, a selected NULL row inserting NULL_HASH. row_sel may be null, ascending, or in any order with
 *   repeats: a repeated row is probed, written and inserted as often as it is listed. Nothing at or past the returned
 *   count is written to out_sel (exactly n entries are enough) and no row_sel entry at or past n is read. has_data
 *   becomes 1 whenever n > 0. A destination may be listed twice, with different columns. range_mask == 0 in
 *   rpt_bf_transfer_range hands over to rpt_bf_transfer, whose kernel is what runs and what the profiler records. The
 *   range is read from device memory when the kernel runs: a captured call sees at every replay the min/max the filter
 *   holds by then.
 * Memory: key, validity, key_sel, row_sel and the output buffers (out_sel, the count) may be device-mapped pinned host
 *   memory (hipHostGetDevicePointer), as for rpt_bf_probe_chain; the filters' words stay in device memory.
 * Strategy: every probed filter is gathered and every insert is one atomic OR per row: forced probe and insert
 *   strategies do not matter, and any filter size works.
 * Argument checks, all before any launch and all RPT_ERR_INVALID_ARGUMENT. Before any handle is looked into: null lists
 *   ("null argument"), n_filters / n_dst outside 1..RPT_MAX_CHAIN, a null handle, a destination that is also probed; the
 *   mask (a bit at or above n_filters, a flagged HASH column) and the probed columns; n > RPT_SMALL_PROBE_ROWS ("n=...
 *   rows exceeds RPT_SMALL_PROBE_ROWS", 2^32 and more included, before row_sel and out_sel are looked at); with a
 *   row_sel, an out_sel range of n entries that overlaps row_sel's ("out_sel overlaps row_sel": the inserts read
 *   row_sel after the tail has begun to write out_sel). Then, in rpt_bf_probe_chain_range's order: filters on different
 *   devices; a destination off the chain's device or with a bad column; n == 0 sets *out_count_dev to 0, stream-ordered,
 *   and touches no destination; a null out_sel; the destinations' capture and in-flight refusals; the probed filters'
 *   pending clears settled (refused inside a capture).
 * Ordering and capture: rpt_bf_transfer_sel's rules. Fully stream-ordered: no synchronisation, no copy, no allocation.
 *   Every destination follows rpt_bf_insert's write rules (a deferred clear or an earlier write in flight is refused
 *   inside a capture, otherwise the call is ordered after the destination's previous write and settles its clear); the
 *   write scopes are taken in ascending handle address, a filter listed twice once, and held across the one launch, so
 *   threads that list the same destinations in different orders do not deadlock.
 *
 * rpt_bf_insert_multi: the sink of one vector into 1..RPT_MAX_CHAIN filters in one launch. Each dst_filters[j] ends
 *   bit-identical to rpt_bf_insert(dst_filters[j], &dst_cols[j], n) over rows 0..n-1, or over row_sel[0..n), min/max
 *   included. n == 0 is a no-op and leaves has_data alone; otherwise has_data becomes 1. Refused before any handle is
 *   looked into: null lists, n_dst outside 1..RPT_MAX_CHAIN ("n_dst=... outside 1..8"), a null destination handle,
 *   n > RPT_SMALL_PROBE_ROWS. Then every destination must be on dst_filters[0]'s device and have a good column; then the
 *   write rules and scopes of the transfer. The buffers may be device-mapped pinned host memory too.
 *
 * When to use them (measured on an MI355X, int64 keys, row_sel null, against rpt_bf_transfer_ws with the same arguments,
 *   whose small-batch hand-over is already 1 + n_dst launches, and against the host loop "rpt_bf_probe_chain,
 *   synchronize, read the count, one rpt_bf_insert_sel per destination"; 1 / 3 / 8 filters of 128 KiB or 16 MiB, 1-2
 *   destinations, 0.1-0.9 of the rows surviving; spread within a line at most 4 %; DESIGN §5 "One launch for a forward
 *   step"): at n = 2048 rpt_bf_transfer is level with or ahead of the _ws call in every shape, 1.00-1.16x faster per step
 *   enqueued eagerly and 1.04-1.29x replayed from a graph, and 1.7-3.4x faster than the host loop. At 8192 rows it is
 *   level or ahead (1.00-1.10x) while at most half of the rows survive and BEHIND when 0.9 survive (the _ws call is
 *   1.04-1.25x faster). At 16384 rows it LOSES in 33 of 36 shapes: the _ws call is up to 1.6x faster (level only with
 *   0.1 surviving), and with 0.9 surviving into two destinations even the host loop is 1-8 % faster. The filter size
 *   hardly moves these ratios: one workgroup inserts the destinations one after another on one CU.
 *   rpt_bf_insert_multi against one rpt_bf_insert per filter (1 / 2 / 4 filters): level at 2048 rows (0.90-1.05x eager;
 *   replayed 0.85-0.97x for one filter, 1.04-1.10x for two and four), and it LOSES beyond: the m multi-workgroup inserts
 *   are 2.1-2.2x faster at 8192 rows and 3.1-3.6x at 16384. So: one DuckDB vector (2048 rows) per call takes these
 *   calls, for a modest gain and one graph node per step; row lists of 8192 and more take rpt_bf_transfer_ws /
 *   rpt_bf_insert.
 *   Nothing is dispatched on any of this: rpt_bf_transfer_ws keeps its hand-over and the caller picks the call. */
int rpt_bf_transfer(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                    rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                    const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                    rpt_stream_t stream);
int rpt_bf_transfer_range(const rpt_bf* const* filters, const rpt_key_column* cols, uint32_t n_filters,
                          uint32_t range_mask, rpt_bf* const* dst_filters, const rpt_key_column* dst_cols,
                          uint32_t n_dst, const uint32_t* row_sel, uint64_t n, uint32_t* out_sel,
                          uint64_t* out_count_dev, rpt_stream_t stream);
int rpt_bf_insert_multi(rpt_bf* const* dst_filters, const rpt_key_column* dst_cols, uint32_t n_dst,
                        const uint32_t* row_sel, uint64_t n, rpt_stream_t stream);

/* ---- composite join keys, hashed inside the kernels ------------------------------------------ */
/* A join key of several columns (the optimizer's multi-column transfer edges; HashColumns, reference
 * src/bloom_filter.cpp:11-24) without the hash passes: the calls below read every column of a key once and hash and
 * combine in the kernel that uses the hash, where rpt_hash_keys + rpt_hash_combine per further column write an 8-byte
 * hash column to memory and read it back between the columns.
 *
 * A key, for every call below. Position i is row r = row_sel ? row_sel[i] : i. Column j contributes
 *   Hash(keys_j[key_sel_j ? key_sel_j[r] : r]), or NULL_HASH where that physical index is NULL in validity_j, exactly as
 *   rpt_hash_combine treats it; h = contrib_0, then h = CombineHashScalar(h, contrib_j) for j = 1 .. n_cols - 1. The
 *   result is bit-identical to rpt_hash_keys(col_0) followed by rpt_hash_combine(col_j).
 * Key types: RPT_KEY_I64 and RPT_KEY_I32, mixed freely. RPT_KEY_HASH only as column 0: a prefix already hashed, so a key
 *   of more than RPT_MAX_KEY_COLUMNS columns is hashed in rounds; with n_cols == 1 it is the pre-hashed column of the
 *   single-column calls. A HASH column at position >= 1 is RPT_ERR_INVALID_ARGUMENT.
 * Min/max: a key of two or more columns folds no min/max into a destination filter (composite keys carry none); a key
 *   of one column behaves exactly as in the single-column call, min/max included.
 * Argument checks, before any handle is looked into and all RPT_ERR_INVALID_ARGUMENT: a null key or key list, null
 *   cols ("null cols"), n_cols outside 1..RPT_MAX_KEY_COLUMNS ("n_cols=... outside 1..4"), a bad key type, a HASH column
 *   past column 0 ("HASH column at position ..."), a null keys pointer, and for the one-launch calls more than
 *   RPT_MAX_CHAIN_KEY_COLUMNS columns over the probed keys, or over the destination keys ("... columns over the ...
 *   keys exceed RPT_MAX_CHAIN_KEY_COLUMNS"). The list checks a key check depends on (a null list, n_filters / n_dst
 *   outside 1..RPT_MAX_CHAIN) come before it, the twin's other checks after it, in the twin's order.
 *
 * rpt_hash_keys_composite: out_hashes[i] for rows 0..n-1, any n, one launch; out_hashes holds exactly n entries.
 *   n_cols == 1 forwards to rpt_hash_keys. Runs on the current device, like rpt_hash_keys.
 * rpt_bf_insert_composite: rows 0..n-1 into bf, any n, one launch, one atomic OR per row. Every rule of rpt_bf_insert:
 *   the write order, the deferred clear, capture, has_data; n == 0 is a no-op. n_cols == 1 forwards to rpt_bf_insert.
 *   There is no routed (PARTITIONED / BUCKETED) composite insert: hash with rpt_hash_keys_composite and call
 *   rpt_bf_insert_ws on the HASH column.
 * rpt_bf_probe_chain_composite, rpt_bf_transfer_composite, rpt_bf_insert_multi_composite: rpt_bf_probe_chain,
 *   rpt_bf_transfer and rpt_bf_insert_multi with a key per filter instead of a column: n <= RPT_SMALL_PROBE_ROWS, one
 *   workgroup, one launch, no workspace, 1..RPT_MAX_CHAIN filters and destinations, and the twins' refusals before any
 *   launch (filters on different devices, a destination among the probed filters, out_sel overlapping a given row_sel,
 *   null arguments, n too large, captured destinations, pending clears). n == 0 sets the count to 0 and touches no
 *   destination. The row_sel of the call is read once per (filter, 512-position segment), not once per column. With
 *   every key of one column the result equals the single-column twin's: words, min/max, selection and count.
 * When to use them (measured on an MI355X against the hash passes followed by the single-column call, int64 and int32
 *   columns, row_sel null; DESIGN §5 "Composite keys hashed in the kernel"): one vector of 2048-8192 rows through 1 or 3
 *   filters with keys of 2 or 3 columns is 1.1-3.5x faster per step enqueued eagerly and 1.1-2.1x replayed from a graph,
 *   in every shape; at 16384 rows the calls are level with the passes (0.96-1.25x: behind by up to 4 % on 16 MiB filters
 *   with three-column keys). rpt_hash_keys_composite is 1.25-2.7x faster (at 2^27 rows the ratio of the bytes moved),
 *   rpt_bf_insert_composite 1.14-1.33x (the atomics bound both routes).
 * Not provided: a composite form of the workspace chains (*_ws), of the device-counted *_sel calls, and of the range
 *   mask (a range belongs to one column's values). Nothing dispatches to these calls. */
#define RPT_MAX_KEY_COLUMNS 4        /* columns of one composite key */
#define RPT_MAX_CHAIN_KEY_COLUMNS 16 /* columns over all probed keys of one call; likewise over all destination keys */
typedef struct rpt_composite_key {
  const rpt_key_column* cols; /* host array of n_cols column descriptors (device pointers inside, as everywhere) */
  uint32_t n_cols;            /* 1..RPT_MAX_KEY_COLUMNS */
} rpt_composite_key;
int rpt_hash_keys_composite(const rpt_composite_key* key, uint64_t n, uint64_t* out_hashes, rpt_stream_t stream);
int rpt_bf_insert_composite(rpt_bf* bf, const rpt_composite_key* key, uint64_t n, rpt_stream_t stream);
int rpt_bf_probe_chain_composite(const rpt_bf* const* filters, const rpt_composite_key* keys, uint32_t n_filters,
                                 const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                                 rpt_stream_t stream);
int rpt_bf_transfer_composite(const rpt_bf* const* filters, const rpt_composite_key* keys, uint32_t n_filters,
                              rpt_bf* const* dst_filters, const rpt_composite_key* dst_keys, uint32_t n_dst,
                              const uint32_t* row_sel, uint64_t n, uint32_t* out_sel, uint64_t* out_count_dev,
                              rpt_stream_t stream);
int rpt_bf_insert_multi_composite(rpt_bf* const* dst_filters, const rpt_composite_key* dst_keys, uint32_t n_dst,
                                  const uint32_t* row_sel, uint64_t n, rpt_stream_t stream);

/* ---- merge / fold / export ----------------------------------------------------------------- */
/* dst |= src (same log_num_blocks, same device): merging per-thread or per-GPU partial filters
 * built over disjoint row ranges gives the filter of the union, bit-identical to one build. */
int rpt_bf_merge_or(rpt_bf* dst, const rpt_bf* src, rpt_stream_t stream);
/* Multi-GPU CREATE_BF Combine: OR all-reduce of every rank's partial filter over an RCCL
 * communicator (`comm` is an ncclComm_t, one rank per GPU; every rank's filter has the same
 * log_num_blocks). It is composed as a reduce-scatter by OR (grouped ncclSend/ncclRecv of 1/W of the
 * words, then an OR kernel) and an all-gather (grouped ncclSend/ncclRecv). RCCL has no bitwise-OR
 * ncclRedOp_t. The key min/max and has_data are reduced too, in one ncclAllReduce(MIN). Collective:
 * every rank of the communicator must call it. Stream-ordered on `stream`; returns after has_data is
 * known (one stream sync). librccl is loaded on first use (dlopen), so the library itself does not
 * depend on it.
 * Rank j owns words [lo(j), lo(j+1)), lo(j) = (num_blocks * j / world) rounded down to 32 words (W need not
 * divide the block count). The reduce-scatter runs in rounds of at most RPT_ALLREDUCE_ROUND_WORDS words
 * per peer through two staging buffers: the OR kernel of round r runs on a library helper stream while
 * round r + 1 transfers on `stream`. rpt_bf_allreduce_or_ws takes that staging from the caller
 * (rpt_allreduce_workspace_bytes(world, log_num_blocks) bytes of device memory, exclusively owned until
 * the call returns; <= 2 (W-1) * 32 MiB + 256 B whatever the filter size); rpt_bf_allreduce_or allocates
 * and frees it itself.
 * Failure (the cross-GPU analogue of a Combine that cannot finish, physical_create_bf.cpp:244-275): the
 * call never blocks on the stream blindly. It polls the stream and ncclCommGetAsyncError until every
 * transfer completed or the collective timeout (rpt_collective_set_timeout_ms) passed; a non-blocking
 * communicator's ncclInProgress results are polled against the same deadline. A peer that dies mid-merge
 * never posts its side, so its peers' streams would wait forever: on a timeout, an asynchronous RCCL error
 * or any error after the first collective call, the call ABORTS the communicator (ncclCommAbort, which
 * frees it), drains the streams (bounded again) and returns RPT_ERR_COMM_ABORTED: never use the
 * communicator again, and do not ncclCommDestroy it (rpt_rccl_comm_destroy accepts one this library made
 * and does nothing). An error before any collective call returns RPT_ERR_COLLECTIVE (or another status)
 * with the communicator intact. The filter then holds its own partial plus possibly some peers' bits
 * (never fewer bits than before the call): rebuild it, or merge again on a new communicator.
 * If even the aborted streams do not drain by the second deadline, the message says "streams did not
 * drain": the workspace, `stream` and the filter stay in use by work that may never finish (later work
 * ordered after them may never run; rpt_bf_allreduce_or then leaks its workspace rather than free it).
 * A caller that owns its communicator and wants to abort it itself sets rpt_collective_set_abort_on_error(0):
 * the merge then never aborts; after a failure past the first collective call it returns
 * RPT_ERR_COLLECTIVE with the communicator untouched, and, when RCCL's kernels still hold the streams (the
 * message says "streams are still blocked"), `stream`, the workspace and the filter stay in use until the
 * owner calls ncclCommAbort. Not inside a stream capture (RPT_ERR_INVALID_ARGUMENT): it waits on the host. */
#define RPT_ALLREDUCE_ROUND_WORDS (4ULL << 20)
size_t rpt_allreduce_workspace_bytes(int world, int log_num_blocks);
int rpt_bf_allreduce_or_ws(rpt_bf* bf, void* nccl_comm, void* workspace, size_t workspace_bytes,
                           rpt_stream_t stream);
int rpt_bf_allreduce_or(rpt_bf* bf, void* nccl_comm, rpt_stream_t stream);
/* Bound of one OR all-reduce's waits (process-wide; default RPT_COLLECTIVE_TIMEOUT_MS_DEFAULT). An 8 GiB
 * filter merges in well under a second over xGMI; the bound only has to outlast RCCL's first connection
 * setup between the ranks. 0 is rejected. */
#define RPT_COLLECTIVE_TIMEOUT_MS_DEFAULT 120000ULL
int rpt_collective_set_timeout_ms(uint64_t ms);
uint64_t rpt_collective_timeout_ms(void);
/* Process-wide: 1 (default) = a failed merge aborts its communicator (RPT_ERR_COMM_ABORTED above); 0 = it
 * leaves the communicator to its owner (RPT_ERR_COLLECTIVE). */
int rpt_collective_set_abort_on_error(int abort_on_error);
int rpt_collective_abort_on_error(void);
/* RCCL communicator for callers that bring none (bench.py, tests; a DuckDB shim that owns an
 * ncclComm_t passes it to rpt_bf_allreduce_or directly). Rank 0 calls rpt_rccl_get_unique_id, the
 * caller broadcasts the RPT_RCCL_UNIQUE_ID_BYTES bytes out of band (torch.distributed, MPI, a file),
 * then every rank calls rpt_rccl_comm_init_rank for its own GPU (collective; blocks until all ranks
 * joined) — ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy of the dlopened librccl. */
#define RPT_RCCL_UNIQUE_ID_BYTES 128
/* RPT_OK if librccl loads with every entry point the merge uses and `device` can be made current (no
 * collective call): every rank checks it, and the ranks agree, before the collective init, so a rank
 * that cannot join never leaves the others blocked in ncclCommInitRank. */
int rpt_rccl_available(int device);
int rpt_rccl_get_unique_id(uint8_t* out_id);
int rpt_rccl_comm_init_rank(int device, int world, const uint8_t* id, int rank, void** out_comm);
/* The same as a NON-BLOCKING communicator (ncclCommInitRankConfig, blocking = 0): every RCCL call on it returns
 * at once (ncclInProgress) and rpt_bf_allreduce_or[_ws] polls ncclCommGetAsyncError against the collective
 * timeout, so even RCCL's host-side connection setup with a peer that died cannot block the caller past the
 * bound (a blocking communicator's ncclGroupEnd can). Init itself completes within the timeout or fails. */
int rpt_rccl_comm_init_rank_nonblocking(int device, int world, const uint8_t* id, int rank, void** out_comm);
/* Destroy a communicator made by rpt_rccl_comm_init_rank[_nonblocking] (one a failed merge aborted: nothing to
 * do). A non-blocking one is finalized first (ncclCommFinalize, polled to completion against the collective
 * timeout; aborted if it does not complete), so its teardown has finished when this returns. */
int rpt_rccl_comm_destroy(void* comm);
/* dst[i] |= src[i] for n_words words (device pointers): the local step of the multi-GPU
 * OR all-reduce (reduce-scatter slices). dst and src must be 16-byte aligned (RPT_ERR_INVALID_ARGUMENT
 * otherwise); n_words may be odd. */
int rpt_words_or(uint64_t* dst, const uint64_t* src, uint64_t n_words, rpt_stream_t stream);
/* dst[i] = src_0[i] | src_1[i] | ... | src_{k-1}[i], srcs given as k contiguous slices of
 * n_words words starting at `srcs` (a receive buffer of k peer slices). dst and every slice are read and
 * written in 16-byte pieces: dst and srcs must be 16-byte aligned, and with k >= 2 n_words must be even (slice
 * s starts at srcs + s * n_words). Anything else is rejected with RPT_ERR_INVALID_ARGUMENT before any launch. */
int rpt_words_or_slices(uint64_t* dst, const uint64_t* srcs, uint32_t k, uint64_t n_words, rpt_stream_t stream);
/* BlockedBloomFilter::IsSameAs (pyarrow 25 arrow/acero/bloom_filter.h:131): *out_same = 1 iff both filters
 * have the same log_num_blocks and every word is equal, compared on the device (no host copy of either
 * filter; bench.py's multi-GPU merge check of C5's 8 GiB filters). *out_diff_words (nullable) = the number of
 * differing words (~0 for different geometry). Filters on one device. Synchronous (waits for the device). */
int rpt_bf_is_same_as(const rpt_bf* a, const rpt_bf* b, int* out_same, uint64_t* out_diff_words);
/* Number of set bits (BlockedBloomFilter::NumBitsSet). Synchronous. */
int rpt_bf_count_bits(const rpt_bf* bf, uint64_t* out);
/* BlockedBloomFilter::Fold (bloom_filter.h:135-158): while fewer than 1/4 of the bits are set and
 * the filter has more than 2^4 blocks, OR its upper slices into the lowest one. Synchronous. */
int rpt_bf_fold(rpt_bf* bf, int* out_new_log_num_blocks);
/* Copy the blocks to/from host memory (parity, checkpoint of a finished filter). Synchronous.
 * import sets has_data = (any bit set). */
int rpt_bf_export_words(const rpt_bf* bf, uint64_t* host_words, uint64_t n_words);
int rpt_bf_import_words(rpt_bf* bf, const uint64_t* host_words, uint64_t n_words);
/* Stream-ordered device-to-device copies of all 2^log_num_blocks blocks to / from a caller buffer
 * (the staging buffer of the multi-GPU OR all-reduce). n_words must equal the block count. */
int rpt_bf_copy_words_to(const rpt_bf* bf, uint64_t* dst_dev, uint64_t n_words, rpt_stream_t stream);
int rpt_bf_copy_words_from(rpt_bf* bf, const uint64_t* src_dev, uint64_t n_words, rpt_stream_t stream);
/* Mark has_data after words were filled by a device-side exchange (multi-GPU merge). */
int rpt_bf_set_has_data(rpt_bf* bf, int value);

/* ---- kernel timing ----------------------------------------------------------------------- */
/* The reference's per-operator profiling counters (src/include/rpt_profiling.hpp:16-217), at kernel
 * granularity: while enabled, every kernel the library launches is bracketed by HIP events on its
 * own stream. rpt_profiling_read resolves pending events (waits for them), fills up to `capacity`
 * entries and returns the number of distinct kernels (negative status on error); out == NULL or
 * capacity == 0 only counts. Names are the kernels' instantiation names ("partition_kernel<0,true,false,1,0>"),
 * cut to 47 characters. Process-wide, thread-safe.
 * Stream capture: a launch on a capturing stream is not recorded (events recorded into a graph cannot be
 * timed), and neither are the graph's replays: the record holds the launches made outside captures only.
 * A launch whose events cannot be resolved at read time is dropped from the record, the others are counted. */
typedef struct rpt_kernel_stat {
  char name[48];
  uint64_t launches;
  double total_ms;
} rpt_kernel_stat;
int rpt_profiling_enable(int enable);
int rpt_profiling_reset(void);
int rpt_profiling_read(rpt_kernel_stat* out, int capacity);

#ifdef __cplusplus
}
#endif

#endif /* RPT_GPU_H */
