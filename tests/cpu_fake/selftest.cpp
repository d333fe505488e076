// selftest.cpp — drives the CPU fakes (fake_hip.cpp, fake_rpt_gpu.cpp) directly and proves that the lazy schedule
// detects what it claims to: each case shows that the misuse yields poisoned or stale bytes and that the correct
// sequence yields the right ones. Without this a green run of the host mirror on the fake would prove nothing.
// Under RPT_FAKE_EAGER=1 (run-at-enqueue) the misuses of (a)-(e) cannot show; only the correct sequences are checked
// then. Case (g) sets its two streams' schedules itself, so it shows in every mode.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fake_hip.hpp"
#include "rpt_gpu.h"

extern "C" {
void rpt_oracle_insert_i64(uint64_t* words, int log_nb, const int64_t* keys, const uint32_t* key_sel,
                           const uint64_t* validity, uint64_t n);
uint64_t rpt_oracle_probe_i64(const uint64_t* words, int log_nb, const int64_t* keys, const uint32_t* key_sel,
                              const uint64_t* validity, uint64_t n, uint32_t* sel);
}

static int g_fail = 0;
#define EXPECT(cond, ...)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      g_fail++;                                            \
    }                                                      \
  } while (0)
#define HIP_OK(call) EXPECT((call) == hipSuccess, "%s failed", #call)

constexpr size_t kN = 1024;
static const uint32_t kPoisonWord = 0x01010101u * fake_hip::kPoison;

static std::vector<uint32_t> pattern(uint32_t seed) {
  std::vector<uint32_t> v(kN);
  for (size_t i = 0; i < kN; i++) v[i] = seed * 1000003u + static_cast<uint32_t>(i);
  return v;
}
static bool equals(const uint32_t* p, const std::vector<uint32_t>& v) { return std::memcmp(p, v.data(), kN * 4) == 0; }
static bool all_poison(const uint32_t* p) {
  for (size_t i = 0; i < kN; i++)
    if (p[i] != kPoisonWord) return false;
  return true;
}

struct Buffers {
  uint32_t *dev = nullptr, *pin_in = nullptr, *pin_out = nullptr;
  hipStream_t p = nullptr, c = nullptr;
  hipEvent_t ev = nullptr;
  Buffers() {
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&dev), kN * 4));
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&pin_in), kN * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&pin_out), kN * 4, hipHostMallocDefault));
    HIP_OK(hipStreamCreateWithFlags(&p, hipStreamNonBlocking));
    HIP_OK(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  ~Buffers() {
    HIP_OK(hipStreamDestroy(p));
    HIP_OK(hipStreamDestroy(c));
    HIP_OK(hipEventDestroy(ev));
    HIP_OK(hipFree(dev));
    HIP_OK(hipHostFree(pin_in));
    HIP_OK(hipHostFree(pin_out));
  }
};

// (a) a device-to-host copy into pinned memory, read before hipStreamSynchronize
static void case_read_before_sync(bool lazy) {
  Buffers b;
  const std::vector<uint32_t> a = pattern(1);
  EXPECT(all_poison(b.dev) && all_poison(b.pin_out), "(a) fresh allocations are poisoned");
  HIP_OK(hipMemcpyAsync(b.dev, a.data(), kN * 4, hipMemcpyHostToDevice, b.p));  // pageable source: read at the call
  HIP_OK(hipMemcpyAsync(b.pin_out, b.dev, kN * 4, hipMemcpyDeviceToHost, b.p));
  if (lazy) EXPECT(all_poison(b.pin_out), "(a) pinned memory read before the synchronisation must still be poison");
  HIP_OK(hipStreamSynchronize(b.p));
  EXPECT(equals(b.pin_out, a), "(a) after hipStreamSynchronize the copy has arrived");
}

// (b) a pinned source overwritten after hipMemcpyAsync and before its event
static void case_refill_before_event(bool lazy) {
  const std::vector<uint32_t> a = pattern(2), z = pattern(3);
  for (int misuse = lazy ? 1 : 0; misuse >= 0; misuse--) {
    Buffers b;
    std::memcpy(b.pin_in, a.data(), kN * 4);
    HIP_OK(hipMemcpyAsync(b.dev, b.pin_in, kN * 4, hipMemcpyHostToDevice, b.p));
    HIP_OK(hipEventRecord(b.ev, b.p));
    if (!misuse) HIP_OK(hipEventSynchronize(b.ev));
    std::memcpy(b.pin_in, z.data(), kN * 4);  // the next stage's keys
    HIP_OK(hipStreamSynchronize(b.p));
    if (misuse) EXPECT(equals(b.dev, z), "(b) a pinned buffer refilled before its copied event must reach the device refilled");
    else EXPECT(equals(b.dev, a), "(b) waiting for the event first keeps the copy intact");
  }
}

// (c) a consumer stream without hipStreamWaitEvent on the producer's event
static void case_missing_stream_wait(bool lazy) {
  const std::vector<uint32_t> a = pattern(4);
  for (int misuse = lazy ? 1 : 0; misuse >= 0; misuse--) {
    Buffers b;
    std::memcpy(b.pin_in, a.data(), kN * 4);
    HIP_OK(hipMemcpyAsync(b.dev, b.pin_in, kN * 4, hipMemcpyHostToDevice, b.p));
    HIP_OK(hipEventRecord(b.ev, b.p));
    if (!misuse) HIP_OK(hipStreamWaitEvent(b.c, b.ev, 0));
    HIP_OK(hipMemcpyAsync(b.pin_out, b.dev, kN * 4, hipMemcpyDeviceToHost, b.c));
    HIP_OK(hipStreamSynchronize(b.c));
    if (misuse) {
      EXPECT(all_poison(b.pin_out), "(c) a consumer that does not wait for the producer must read poison");
      EXPECT(all_poison(b.dev), "(c) a stream nothing waited for stays un-run");
    } else {
      EXPECT(equals(b.pin_out, a), "(c) with hipStreamWaitEvent the consumer sees the producer's bytes");
    }
    HIP_OK(hipStreamSynchronize(b.p));
  }
}

// (d) a wait captured before the event is re-recorded still waits for the old position (and only for it)
static void case_rerecord(bool lazy) {
  Buffers b;
  const std::vector<uint32_t> a = pattern(5), z = pattern(6);
  HIP_OK(hipMemcpyAsync(b.dev, a.data(), kN * 4, hipMemcpyHostToDevice, b.p));
  HIP_OK(hipEventRecord(b.ev, b.p));
  HIP_OK(hipStreamWaitEvent(b.c, b.ev, 0));
  HIP_OK(hipMemcpyAsync(b.dev, z.data(), kN * 4, hipMemcpyHostToDevice, b.p));
  HIP_OK(hipEventRecord(b.ev, b.p));  // the same event, a later position
  HIP_OK(hipMemcpyAsync(b.pin_out, b.dev, kN * 4, hipMemcpyDeviceToHost, b.c));
  HIP_OK(hipStreamSynchronize(b.c));
  if (lazy) EXPECT(equals(b.pin_out, a), "(d) the wait belongs to the first record: the second copy has not run");
  HIP_OK(hipEventSynchronize(b.ev));  // the latest record
  EXPECT(equals(b.dev, z), "(d) hipEventSynchronize waits for the latest record");
  hipEvent_t never;
  HIP_OK(hipEventCreate(&never));
  EXPECT(hipEventQuery(never) == hipSuccess && hipEventSynchronize(never) == hipSuccess, "(d) a never-recorded event is complete");
  HIP_OK(hipStreamWaitEvent(b.c, never, 0));
  HIP_OK(hipStreamSynchronize(b.c));
  HIP_OK(hipEventDestroy(never));
}

// (e) a polling loop on hipEventQuery (and on hipStreamQuery) terminates, one pending closure per poll
static void case_polling(bool lazy) {
  Buffers b;
  const std::vector<uint32_t> a = pattern(7);
  for (int i = 0; i < 5; i++) HIP_OK(hipMemcpyAsync(b.dev, a.data(), kN * 4, hipMemcpyHostToDevice, b.p));
  HIP_OK(hipEventRecord(b.ev, b.p));
  int polls = 0;
  hipError_t q;
  while ((q = hipEventQuery(b.ev)) == hipErrorNotReady && polls < 100) polls++;
  EXPECT(q == hipSuccess && (lazy ? polls == 5 : fake_hip::eager() ? polls == 0 : polls <= 5), "(e) hipEventQuery loop: %d polls", polls);
  EXPECT(equals(b.dev, a), "(e) the polled work has run");
  for (int i = 0; i < 3; i++) HIP_OK(hipMemcpyAsync(b.dev, a.data(), kN * 4, hipMemcpyHostToDevice, b.c));
  polls = 0;
  while ((q = hipStreamQuery(b.c)) == hipErrorNotReady && polls < 100) polls++;
  EXPECT(q == hipSuccess && (lazy ? polls == 3 : fake_hip::eager() ? polls == 0 : polls <= 3), "(e) hipStreamQuery loop: %d polls", polls);
}

// (g) write after read across streams: a stream that overwrites a buffer another stream has yet to read, without
// waiting for that read. Neither the all-lazy nor the all-eager schedule can show it; an early writer and a late
// reader (what RPT_FAKE_EAGER=mix:<seed> deals out) do.
static void case_write_after_read() {
  const std::vector<uint32_t> a = pattern(9), z = pattern(10);
  for (int misuse = 1; misuse >= 0; misuse--) {
    Buffers b;
    HIP_OK(fake_hip::set_stream_eager(b.p, true));   // the writer runs ahead
    HIP_OK(fake_hip::set_stream_eager(b.c, false));  // the reader lags
    HIP_OK(hipMemcpyAsync(b.dev, a.data(), kN * 4, hipMemcpyHostToDevice, b.p));
    HIP_OK(hipMemcpyAsync(b.pin_out, b.dev, kN * 4, hipMemcpyDeviceToHost, b.c));  // the read
    HIP_OK(hipEventRecord(b.ev, b.c));
    if (!misuse) HIP_OK(hipStreamWaitEvent(b.p, b.ev, 0));
    HIP_OK(hipMemcpyAsync(b.dev, z.data(), kN * 4, hipMemcpyHostToDevice, b.p));  // the next stage's bytes
    HIP_OK(hipStreamSynchronize(b.c));
    if (misuse) EXPECT(equals(b.pin_out, z), "(g) a buffer overwritten before its reader ran must be read overwritten");
    else EXPECT(equals(b.pin_out, a), "(g) with the writer waiting for the read, the reader sees the first bytes");
  }
}

// pageable host memory: the source of a copy to the device is read at the call; a copy to it is done at return
static void case_pageable() {
  Buffers b;
  std::vector<uint32_t> a = pattern(8), out(kN, 0);
  const std::vector<uint32_t> a0 = a;
  HIP_OK(hipMemcpyAsync(b.dev, a.data(), kN * 4, hipMemcpyHostToDevice, b.p));
  std::fill(a.begin(), a.end(), 0u);  // legal for pageable memory
  HIP_OK(hipMemcpyAsync(out.data(), b.dev, kN * 4, hipMemcpyDeviceToHost, b.p));
  EXPECT(out == a0, "pageable copies: read at the call, back at return");
  void* dp = nullptr;
  EXPECT(hipHostGetDevicePointer(&dp, b.pin_in, 0) == hipSuccess && dp == b.pin_in, "pinned memory maps to its own address");
  EXPECT(hipHostGetDevicePointer(&dp, out.data(), 0) != hipSuccess, "pageable memory has no device pointer");
}

// (f) a _ws insert refuses a null or short workspace; with the right one it trashes it and inserts; the probes
// answer as the oracle does
static void case_workspace() {
  const uint64_t n = 3000;
  std::vector<int64_t> keys(n), probe(n);
  for (uint64_t i = 0; i < n; i++) {
    keys[i] = static_cast<int64_t>(i * 7919 + 13);
    probe[i] = static_cast<int64_t>(i % 2 ? i * 7919 + 13 : i * 104729 + 5);
  }
  rpt_bf* bf = nullptr;
  EXPECT(rpt_bf_create(0, n, &bf) == RPT_OK && bf, "create");
  rpt_bf_info info;
  EXPECT(rpt_bf_get_info(bf, &info) == RPT_OK && info.has_data == 0, "info");
  EXPECT(rpt_bf_insert_workspace_bytes(bf, n) == 0 && rpt_bf_insert_strategy_for(bf, n) == RPT_INSERT_ATOMIC, "a small AUTO insert is atomic");
  EXPECT(rpt_bf_set_insert_strategy(bf, RPT_INSERT_PARTITIONED) == RPT_OK, "force the partitioned insert");
  const size_t need = rpt_bf_insert_workspace_bytes(bf, n);
  EXPECT(need > 0 && rpt_bf_insert_strategy_for(bf, n) == RPT_INSERT_PARTITIONED, "a forced strategy needs a workspace and is echoed");
  Buffers b;
  int64_t* dkeys = nullptr;
  unsigned char* ws = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&dkeys), n * 8));
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&ws), need));
  HIP_OK(hipMemcpyAsync(dkeys, keys.data(), n * 8, hipMemcpyHostToDevice, b.p));
  const rpt_key_column col{RPT_KEY_I64, dkeys, nullptr, nullptr};
  EXPECT(rpt_bf_insert_ws(bf, &col, n, nullptr, need, b.p) == RPT_ERR_WORKSPACE, "(f) a null workspace is refused");
  EXPECT(rpt_bf_insert_ws(bf, &col, n, ws, need - 1, b.p) == RPT_ERR_WORKSPACE, "(f) a short workspace is refused");
  EXPECT(rpt_bf_insert_ws(bf, &col, n, ws + 8, need, b.p) == RPT_ERR_INVALID_ARGUMENT, "(f) a misaligned workspace is refused");
  EXPECT(rpt_bf_get_info(bf, &info) == RPT_OK && info.has_data == 0, "(f) a refused insert leaves the filter empty");
  EXPECT(rpt_bf_insert_ws(bf, &col, n, ws, need, b.p) == RPT_OK, "(f) the right workspace is accepted");
  std::vector<uint64_t> w(info.num_blocks), want(info.num_blocks, 0);
  EXPECT(rpt_bf_export_words(bf, w.data(), w.size()) == RPT_OK, "export");
  rpt_oracle_insert_i64(want.data(), info.log_num_blocks, keys.data(), nullptr, nullptr, n);
  EXPECT(w == want, "(f) the inserted words are the oracle's");
  EXPECT(ws[0] == 0x5E && ws[need - 1] == 0x5E, "(f) a _ws operation overwrites its whole workspace");
  int64_t mn = 0, mx = 0;
  int has = 0;
  EXPECT(rpt_bf_get_minmax(bf, &mn, &mx, &has, nullptr) == RPT_OK && has && mn == keys[0] && mx == keys[n - 1], "min/max");
  // probe: selection vector and result bits against the oracle
  std::vector<uint32_t> exp(n);
  exp.resize(rpt_oracle_probe_i64(want.data(), info.log_num_blocks, probe.data(), nullptr, nullptr, n, exp.data()));
  uint32_t* dsel = nullptr;
  uint64_t *dcnt = nullptr, *dbits = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&dsel), n * 4));
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&dcnt), 8));
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&dbits), (n + 511) / 512 * 64));
  HIP_OK(hipMemcpyAsync(dkeys, probe.data(), n * 8, hipMemcpyHostToDevice, b.p));
  EXPECT(rpt_bf_probe_is_fused(bf, n) == 1, "a small AUTO probe is fused");
  EXPECT(rpt_bf_probe(bf, &col, nullptr, n, dsel, dcnt, nullptr, 0, b.p) == RPT_OK, "the fused probe needs no workspace");
  const size_t pneed = rpt_bf_probe_workspace_bytes(bf, n);
  unsigned char* pws = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&pws), pneed));
  EXPECT(pneed > 0 && rpt_bf_probe_bits(bf, &col, nullptr, n, dbits, pws, pneed - 1, b.p) == RPT_ERR_WORKSPACE,
         "(f) probe_bits refuses a short workspace");
  EXPECT(rpt_bf_probe_bits(bf, &col, nullptr, n, dbits, pws, pneed, b.p) == RPT_OK, "probe_bits");
  HIP_OK(hipStreamSynchronize(b.p));
  EXPECT(*dcnt == exp.size() && std::memcmp(dsel, exp.data(), exp.size() * 4) == 0, "the probe's sel is the oracle's");
  bool bits_ok = true;
  for (uint64_t i = 0, k = 0; i < (n + 511) / 512 * 512; i++) {
    const bool hit = k < exp.size() && exp[k] == i;
    k += hit;
    bits_ok &= ((dbits[i >> 6] >> (i & 63)) & 1) == (hit ? 1u : 0u);
  }
  EXPECT(bits_ok, "the probe's result bits are the oracle's, zero past n");
  for (void* p : {static_cast<void*>(dkeys), static_cast<void*>(ws), static_cast<void*>(dsel), static_cast<void*>(dcnt),
                  static_cast<void*>(dbits), static_cast<void*>(pws)})
    HIP_OK(hipFree(p));
  EXPECT(rpt_bf_destroy(bf) == RPT_OK, "destroy");
}

int main() {
  const bool lazy = fake_hip::lazy();
  case_read_before_sync(lazy);
  case_refill_before_event(lazy);
  case_missing_stream_wait(lazy);
  case_rerecord(lazy);
  case_polling(lazy);
  case_write_after_read();
  case_pageable();
  case_workspace();
  if (g_fail) {
    fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("ALL OK (%s)\n", lazy ? "lazy" : fake_hip::eager() ? "eager" : "mixed");
  return 0;
}
