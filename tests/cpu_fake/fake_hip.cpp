// fake_hip.cpp — the subset of the HIP runtime that csrc/rpt_host.cpp uses, on the CPU, with LAZY streams.
//
// ***************************************************************************************
// TEST INFRASTRUCTURE ONLY (like oracle/). Linked into tests/cpu_fake/build/* in place of
// libamdhip64; the product never sees it. It restates documented HIP runtime behaviour.
// ***************************************************************************************
//
// Why: on a real GPU, work enqueued a few microseconds ago has almost always finished by the time the host
// looks at its buffers again, so a missing hipStreamWaitEvent, a pinned buffer refilled before its copy was
// waited for, or a result read before its event all pass. Here the schedule is the LATEST one HIP allows:
//
//   * device and pinned memory are host allocations (posix_memalign, so ASan knows their bounds), filled
//     with kPoison when fresh;
//   * a stream is a FIFO of closures; enqueueing runs nothing;
//   * work runs only when the host demands it: hipStreamSynchronize, hipEventSynchronize, hipFree,
//     hipHostFree, hipStreamDestroy, hipDeviceSynchronize, and a copy the real runtime makes synchronous
//     (pageable memory, below). Demanding a stream up to a position runs its closures in order; a
//     hipStreamWaitEvent closure first demands the event's captured position on the event's stream. Nothing
//     else runs: a stream nothing waited for stays un-run;
//   * hipEventRecord snapshots (stream, position) as a token; hipStreamWaitEvent captures the token current
//     at the call (a later re-record of the event does not move that wait, as in HIP); hipEventSynchronize
//     waits for the latest token; a never-recorded event is complete;
//   * hipEventQuery / hipStreamQuery return hipErrorNotReady while work is pending, and each such call runs
//     ONE pending closure of what it asks about, so polling loops end;
//   * the null stream: everything pending runs first, then the operation runs at once.
//
// So a missing cross-stream wait or a host access before its synchronisation sees stale or poisoned bytes,
// every time. RPT_FAKE_EAGER=1 switches to run-at-enqueue (the earliest legal schedule), to bisect a failure.
//
// What neither extreme shows is a write-after-read hazard between two streams (a buffer overwritten by stream A
// before stream B has read it): it needs A early and B late. RPT_FAKE_EAGER=mix:<seed> makes each stream eager or
// lazy by a hash of the seed and the stream's creation ordinal; an eager stream runs each operation at enqueue, and
// its hipStreamWaitEvent demands the awaited (lazy) stream then and there. Every mix is a legal schedule too.
//
// One mutex guards everything and is held while closures run: the closures of the whole fake never run
// concurrently, and whichever host thread demands work runs it.
#include "fake_hip.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace {

struct Stream {
  std::deque<std::function<void()>> q;
  uint64_t enqueued = 0, executed = 0;  // positions: closure k (1-based) is done when executed >= k
  bool running = false;
  bool eager = false;  // operations run at enqueue
};
struct Token {
  std::shared_ptr<Stream> stream;  // null: complete
  uint64_t pos = 0;
};
struct Event {
  Token tok;
};

struct State {
  std::mutex mu;
  std::map<Stream*, std::shared_ptr<Stream>> streams;
  std::map<Event*, std::unique_ptr<Event>> events;
  std::map<uintptr_t, size_t> device, pinned;  // live allocations: base -> bytes
  enum Mode { kLazy, kEager, kMix } mode = kLazy;
  uint64_t seed = 0, created = 0;  // kMix: stream number `created` is eager by a hash of both
};
uint64_t mix64(uint64_t z) {  // splitmix64's finalizer
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
State& state() {
  static State* s = [] {  // never destroyed: static destructors of the code under test may still call in
    State* p = new State;
    const char* e = std::getenv("RPT_FAKE_EAGER");
    if (e && std::strncmp(e, "mix:", 4) == 0) {
      p->mode = State::kMix;
      p->seed = std::strtoull(e + 4, nullptr, 10);
    } else if (e && e[0] && std::strcmp(e, "0") != 0) {
      p->mode = State::kEager;
    }
    return p;
  }();
  return *s;
}
thread_local int t_device = 0;

using Lock = std::unique_lock<std::mutex>;

void run_to(Stream& s, uint64_t pos);

void run_one(Stream& s) {
  if (s.running) {
    // a closure of this stream is waiting (through events) for a later closure of the same stream: on a GPU
    // the two streams would wait for each other for ever
    std::fprintf(stderr, "fake_hip: circular wait between streams\n");
    std::abort();
  }
  std::function<void()> fn = std::move(s.q.front());
  s.q.pop_front();
  s.running = true;
  fn();
  s.running = false;
  s.executed++;
}
void run_to(Stream& s, uint64_t pos) {
  while (s.executed < pos) run_one(s);
}
bool complete(const Token& t) { return !t.stream || t.stream->executed >= t.pos; }
void drain_all(State& st) {
  // a closure may demand other streams; none creates or destroys one
  for (auto& kv : st.streams) run_to(*kv.second, kv.second->enqueued);
}

std::shared_ptr<Stream> find_stream(State& st, hipStream_t h) {
  auto it = st.streams.find(reinterpret_cast<Stream*>(h));
  return it == st.streams.end() ? nullptr : it->second;
}
Event* find_event(State& st, hipEvent_t h) {
  auto it = st.events.find(reinterpret_cast<Event*>(h));
  return it == st.events.end() ? nullptr : it->second.get();
}

// lock held
hipError_t enqueue_locked(State& st, hipStream_t h, std::function<void()> op) {
  if (h == nullptr) {  // the null stream
    drain_all(st);
    op();
    return hipSuccess;
  }
  std::shared_ptr<Stream> s = find_stream(st, h);
  if (!s) return hipErrorInvalidHandle;
  if (s->eager) {
    op();
    return hipSuccess;
  }
  s->q.push_back(std::move(op));
  s->enqueued++;
  return hipSuccess;
}

bool inside(const std::map<uintptr_t, size_t>& ranges, const void* p, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = ranges.upper_bound(a);
  if (it == ranges.begin()) return false;
  --it;
  return a >= it->first && a + bytes <= it->first + it->second;
}

hipError_t alloc(std::map<uintptr_t, size_t> State::*which, void** out, size_t bytes) {
  if (!out) return hipErrorInvalidValue;
  *out = nullptr;
  if (bytes == 0) return hipSuccess;
  void* p = nullptr;
  // hipMalloc returns 256-byte aligned memory and hipHostMalloc whole pages; the mirror picks its aligned
  // streaming-store paths by the address, so keep that alignment. posix_memalign is intercepted by ASan.
  if (posix_memalign(&p, 256, bytes) != 0) return hipErrorOutOfMemory;
  std::memset(p, fake_hip::kPoison, bytes);
  State& st = state();
  Lock lk(st.mu);
  (st.*which)[reinterpret_cast<uintptr_t>(p)] = bytes;
  *out = p;
  return hipSuccess;
}
hipError_t release(std::map<uintptr_t, size_t> State::*which, void* p) {
  if (!p) return hipSuccess;
  State& st = state();
  {
    Lock lk(st.mu);
    drain_all(st);  // hipFree / hipHostFree wait for the device before they release the memory
    auto it = (st.*which).find(reinterpret_cast<uintptr_t>(p));
    if (it == (st.*which).end()) return hipErrorInvalidValue;
    (st.*which).erase(it);
  }
  std::free(p);
  return hipSuccess;
}

}  // namespace

namespace fake_hip {
hipError_t enqueue(hipStream_t stream, std::function<void()> op) {
  State& st = state();
  Lock lk(st.mu);
  return enqueue_locked(st, stream, std::move(op));
}
void device_synchronize() {
  State& st = state();
  Lock lk(st.mu);
  drain_all(st);
}
bool eager() { return state().mode == State::kEager; }
bool lazy() { return state().mode == State::kLazy; }
hipError_t set_stream_eager(hipStream_t stream, bool eager) {
  State& st = state();
  Lock lk(st.mu);
  std::shared_ptr<Stream> s = find_stream(st, stream);
  if (!s) return hipErrorInvalidHandle;
  run_to(*s, s->enqueued);
  s->eager = eager;
  return hipSuccess;
}
}  // namespace fake_hip

// ---- the hip* entry points (signatures from hip/hip_runtime_api.h, which also gives them C linkage) ----------

hipError_t hipGetDevice(int* device) {
  if (!device) return hipErrorInvalidValue;
  *device = t_device;
  return hipSuccess;
}
hipError_t hipSetDevice(int device) {
  if (device != 0) return hipErrorInvalidDevice;  // one fake device
  t_device = device;
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
  fake_hip::device_synchronize();
  return hipSuccess;
}

hipError_t hipMalloc(void** ptr, size_t size) { return alloc(&State::device, ptr, size); }
hipError_t hipFree(void* ptr) { return release(&State::device, ptr); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) { return alloc(&State::pinned, ptr, size); }
hipError_t hipHostFree(void* ptr) { return release(&State::pinned, ptr); }
hipError_t hipHostGetDevicePointer(void** dev_ptr, void* host_ptr, unsigned int) {
  State& st = state();
  Lock lk(st.mu);
  if (!dev_ptr || !inside(st.pinned, host_ptr, 1)) return hipErrorInvalidValue;
  *dev_ptr = host_ptr;  // one address space
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int) {
  if (!stream) return hipErrorInvalidValue;
  auto s = std::make_shared<Stream>();
  State& st = state();
  Lock lk(st.mu);
  s->eager = st.mode == State::kEager || (st.mode == State::kMix && (mix64(st.seed * 0x9e3779b97f4a7c15ULL + st.created) & 1));
  st.created++;
  st.streams[s.get()] = s;
  *stream = reinterpret_cast<hipStream_t>(s.get());
  return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* stream) { return hipStreamCreateWithFlags(stream, hipStreamDefault); }
hipError_t hipStreamDestroy(hipStream_t stream) {
  State& st = state();
  Lock lk(st.mu);
  std::shared_ptr<Stream> s = find_stream(st, stream);
  if (!s) return hipErrorInvalidHandle;
  run_to(*s, s->enqueued);  // the real call lets the stream's work finish
  st.streams.erase(s.get());
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
  State& st = state();
  Lock lk(st.mu);
  if (stream == nullptr) {
    drain_all(st);
    return hipSuccess;
  }
  std::shared_ptr<Stream> s = find_stream(st, stream);
  if (!s) return hipErrorInvalidHandle;
  run_to(*s, s->enqueued);
  return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t stream) {
  State& st = state();
  Lock lk(st.mu);
  if (stream == nullptr) {
    drain_all(st);
    return hipSuccess;
  }
  std::shared_ptr<Stream> s = find_stream(st, stream);
  if (!s) return hipErrorInvalidHandle;
  if (s->executed >= s->enqueued) return hipSuccess;
  run_one(*s);  // a poll makes progress, so a polling loop ends
  return hipErrorNotReady;
}
hipError_t hipStreamIsCapturing(hipStream_t stream, hipStreamCaptureStatus* status) {
  State& st = state();
  Lock lk(st.mu);
  if (!status || (stream != nullptr && !find_stream(st, stream))) return hipErrorInvalidValue;
  *status = hipStreamCaptureStatusNone;  // no graphs here
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int) {
  State& st = state();
  Lock lk(st.mu);
  Event* e = find_event(st, event);
  if (!e) return hipErrorInvalidHandle;
  if (stream != nullptr && !find_stream(st, stream)) return hipErrorInvalidHandle;
  const Token tok = e->tok;  // the record current NOW: a later hipEventRecord does not move this wait
  if (complete(tok)) return hipSuccess;
  return enqueue_locked(st, stream, [tok] { run_to(*tok.stream, tok.pos); });
}

hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned int) {
  if (!event) return hipErrorInvalidValue;
  auto e = std::make_unique<Event>();
  State& st = state();
  Lock lk(st.mu);
  *event = reinterpret_cast<hipEvent_t>(e.get());
  st.events[e.get()] = std::move(e);
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* event) { return hipEventCreateWithFlags(event, hipEventDefault); }
hipError_t hipEventDestroy(hipEvent_t event) {
  State& st = state();
  Lock lk(st.mu);
  return st.events.erase(reinterpret_cast<Event*>(event)) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
  State& st = state();
  Lock lk(st.mu);
  Event* e = find_event(st, event);
  if (!e) return hipErrorInvalidHandle;
  if (stream == nullptr) {
    drain_all(st);
    e->tok = Token{};
    return hipSuccess;
  }
  std::shared_ptr<Stream> s = find_stream(st, stream);
  if (!s) return hipErrorInvalidHandle;
  e->tok = Token{s, s->enqueued};
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
  State& st = state();
  Lock lk(st.mu);
  Event* e = find_event(st, event);
  if (!e) return hipErrorInvalidHandle;
  const Token tok = e->tok;
  if (tok.stream) run_to(*tok.stream, tok.pos);
  return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t event) {
  State& st = state();
  Lock lk(st.mu);
  Event* e = find_event(st, event);
  if (!e) return hipErrorInvalidHandle;
  if (complete(e->tok)) return hipSuccess;
  run_one(*e->tok.stream);
  return hipErrorNotReady;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  if (bytes == 0) return hipSuccess;
  if (!dst || !src) return hipErrorInvalidValue;
  State& st = state();
  Lock lk(st.mu);
  std::shared_ptr<Stream> s;
  if (stream != nullptr && !(s = find_stream(st, stream))) return hipErrorInvalidHandle;
  // which side is host memory (hipMemcpyDefault: whatever is not a device allocation)
  const bool src_host = kind == hipMemcpyHostToDevice || kind == hipMemcpyHostToHost ||
                        (kind == hipMemcpyDefault && !inside(st.device, src, bytes));
  const bool dst_host = kind == hipMemcpyDeviceToHost || kind == hipMemcpyHostToHost ||
                        (kind == hipMemcpyDefault && !inside(st.device, dst, bytes));
  // Pageable host memory (not from hipHostMalloc), as the HIP runtime treats it: the source of a copy to the
  // device is read (into the runtime's staging) before hipMemcpyAsync returns, the destination still written in
  // stream order; a copy to pageable host memory has completed when the call returns.
  if (src_host && !inside(st.pinned, src, bytes)) {
    auto snap = std::make_shared<std::vector<unsigned char>>(static_cast<const unsigned char*>(src),
                                                             static_cast<const unsigned char*>(src) + bytes);
    const hipError_t e = enqueue_locked(st, stream, [dst, snap] { std::memcpy(dst, snap->data(), snap->size()); });
    if (e != hipSuccess) return e;
  } else {
    const hipError_t e = enqueue_locked(st, stream, [dst, src, bytes] { std::memcpy(dst, src, bytes); });
    if (e != hipSuccess) return e;
  }
  if (dst_host && !inside(st.pinned, dst, bytes) && s) run_to(*s, s->enqueued);
  return hipSuccess;
}

const char* hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    case hipErrorInvalidHandle: return "invalid resource handle";
    case hipErrorNotReady: return "device not ready";
    default: return "unknown error";
  }
}
