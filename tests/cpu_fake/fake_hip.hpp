// fake_hip.hpp — what the CPU fake of the C-ABI (fake_rpt_gpu.cpp) needs from the CPU fake of the HIP runtime
// (fake_hip.cpp) beyond the hip* entry points themselves. TEST INFRASTRUCTURE ONLY.
#pragma once

#include <hip/hip_runtime_api.h>

#include <functional>

namespace fake_hip {

// One stream-ordered operation ("kernel") on `stream` (nullptr = the null stream). Lazy mode: it runs when the host
// demands the stream up to it, on whichever thread demands it, never concurrently with anything else the fake runs.
// Eager mode (RPT_FAKE_EAGER=1): it runs before enqueue returns.
hipError_t enqueue(hipStream_t stream, std::function<void()> op);

// hipDeviceSynchronize: run everything pending on every stream.
void device_synchronize();

// The schedule: every stream eager (RPT_FAKE_EAGER=1) / every stream lazy (the default). Neither under
// RPT_FAKE_EAGER=mix:<seed>, where each stream is one or the other.
bool eager();
bool lazy();
// Make one stream eager or lazy, whatever the mode (its pending work runs first): for the self-test.
hipError_t set_stream_eager(hipStream_t stream, bool eager);

// The byte fresh device / pinned allocations are filled with.
constexpr unsigned char kPoison = 0xA7;

}  // namespace fake_hip
