// rpt_launch.hpp — the one way librpt_gpu.so launches a kernel: launch_kernel, which opts the kernel into the CU's
// whole LDS, records the launch for rpt_profiling_*, launches and checks, and the dispatch_* helpers that turn a
// run-time key type, flag or tile multiple into the template arguments of the call. Host code, included by rpt_gpu.hip
// inside its unnamed namespace, after fail(), the profiling record (g_prof_*) and stream_capturing().
#pragma once

// Brackets one kernel launch with events on its stream when profiling is enabled. Not on a capturing stream: an
// event recorded there becomes a node of the graph and can never be timed (hipEventElapsedTime fails on it), so a
// captured launch, and every replay of it, stays out of the record.
struct ProfScope {
  hipStream_t stream;
  hipEvent_t start = nullptr;
  ProfScope(bool recorded, hipStream_t s) : stream(s) {
    if (!recorded || !g_prof_enabled.load(std::memory_order_relaxed) || stream_capturing(s)) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    start = prof_event();
    if (start && hipEventRecord(start, stream) != hipSuccess) start = nullptr;
  }
  void end(const char* name) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t e = prof_event();
    if (e && hipEventRecord(e, stream) == hipSuccess) {
      g_prof_pending.push_back({name, start, e});
    } else {
      g_prof_free.push_back(start);
      if (e) g_prof_free.push_back(e);
    }
  }
};

// The name a launch is recorded and reported under: `base` itself, or with NameArgs that of a kernel template
// instantiation, spelled as tools/pmc_summary.py short() spells rocprofv3's kernel names
// ("partition_kernel<0,true,false,1,0>"), so bench.py can match the PMC counters of exactly the instantiation that
// ran. The arguments are the caller's, not the kernel's own: a defaulted one is spelled out, and suffixed names
// ("or_slices_kernel(fold)") have none. Built once per instantiation; asked for only by a launch that is recorded or
// has failed.
template <typename T>
std::string targ_str(T v) {
  if constexpr (std::is_same_v<T, bool>) return v ? "true" : "false";
  else return std::to_string(v);
}
template <auto Kernel, auto... NameArgs>
const char* recorded_name(const char* base) {
  if constexpr (sizeof...(NameArgs) == 0) {
    return base;
  } else {
    static const std::string name = [base] {
      std::string s = base;
      s += '<';
      ((s += targ_str(NameArgs), s += ','), ...);
      s.back() = '>';
      return s;
    }();
    return name.c_str();
  }
}

// Let `Kernel` use all of the CU's 160 KiB of LDS (more than 64 KiB of dynamic LDS must be opted into): dynamic
// allowance = 160 KiB - its static LDS. Once per process and instantiation, on its first launch, whatever LDS that
// launch asks for.
template <auto Kernel>
void allow_dynamic_lds() {
  static const bool done = [] {
    const void* fn = reinterpret_cast<const void*>(Kernel);
    hipFuncAttributes at{};
    size_t stat = 0;
    if (hipFuncGetAttributes(&at, fn) == hipSuccess) stat = at.sharedSizeBytes;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>((160u << 10) - stat));
    (void)hipGetLastError();
    return true;
  }();
  (void)done;
}

// kUnrecorded: the launch stays out of rpt_profiling_read (the ledgers compare exact sets of names).
enum LaunchFlags : unsigned { kUnrecorded = 0, kRecorded = 1, kDynamicLds = 2 };

// Launches Kernel<<<grid, block, lds, s>>>(args...) and returns its status. In this order: the LDS opt-in
// (kDynamicLds), the profiling start event (kRecorded, profiling enabled, s not capturing), the launch, the profiling
// end event, the launch-error check. `base` and NameArgs: recorded_name above, written once per launch site.
template <auto Kernel, auto... NameArgs, typename... Args>
int launch_kernel(const char* base, unsigned flags, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args&&... args) {
  if (flags & kDynamicLds) allow_dynamic_lds<Kernel>();
  ProfScope prof((flags & kRecorded) != 0, s);
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, std::forward<Args>(args)...);
  if (prof.start) prof.end(recorded_name<Kernel, NameArgs...>(base));
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return RPT_OK;
  return fail(RPT_ERR_HIP, "launch of %s failed: %s", recorded_name<Kernel, NameArgs...>(base), hipGetErrorString(e));
}

// Run-time values as template arguments: f is a generic lambda called with std::integral_constants, whose status
// is returned. K: the column's key type; D: the dense row mapping; TM: the partition's tile multiple (1 or 2).
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename F>
int dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
int dispatch_k(int key_type, F&& f) {
  switch (key_type) {
    case RPT_KEY_I64: return f(int_c<rpt::kKeyI64>{});
    case RPT_KEY_I32: return f(int_c<rpt::kKeyI32>{});
    default: return f(int_c<rpt::kKeyHash>{});
  }
}
template <typename F>
int dispatch_kd(int key_type, bool dense, F&& f) {
  return dispatch_k(key_type, [&](auto k) { return dispatch_bool(dense, [&](auto d) { return f(k, d); }); });
}
template <typename F>
int dispatch_tm(uint32_t tm, F&& f) {
  return tm == 2 ? f(int_c<2>{}) : f(int_c<1>{});
}
