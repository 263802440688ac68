// What every handle of the library shares: the error string behind cc_last_error, the profiler's launch note, the per-device stream
// pool, the hardware-queue probe that finds the slots of a handle (batches in flight) streams that really run side by side.
#include <deque>
#include "kernels.h"
#include "../../include/clearcam_hip.h"

static thread_local std::string g_err;

namespace cc {

void set_error(const std::string& m) { g_err = m; }

thread_local LaunchNote g_launch_note = {"", 0, 1};
thread_local bool g_note_launches = false;

// what is enqueued on `waiter` from here on runs after what `signaller` holds now (a throw-away event: the runtime keeps it while in use)
void order_after(hipStream_t waiter, hipStream_t signaller) {
  hipEvent_t e; CC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  CC_HIP(hipEventRecord(e, signaller)); CC_HIP(hipStreamWaitEvent(waiter, e, 0)); CC_HIP(hipEventDestroy(e));
}

// ~0.2 ms of one wave doing nothing (s_memrealtime ticks at 100 MHz): the probe of streams_overlap
__global__ void spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
}

// Do kernels on streams a and b run side by side?  Both streams idle on entry.  One spin kernel alone, then one on each stream
// (b's first: if the two share a queue, a's is queued behind it): on different hardware queues the pair takes about one kernel's time.
bool streams_overlap(hipStream_t a, hipStream_t b) {
  const long long ticks = 20000;
  hipEvent_t e0 = nullptr, e1 = nullptr, eb = nullptr;
  CC_HIP(hipEventCreate(&e0)); CC_HIP(hipEventCreate(&e1));
  CC_HIP(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
  float alone = 0.f, pair = 0.f;
  for (int rep = 0; rep < 2; ++rep) {                   // the first round also pays for code loading and queue creation
    CC_HIP(hipEventRecord(e0, a));
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, ticks);
    CC_HIP(hipEventRecord(e1, a));
    CC_HIP(hipEventSynchronize(e1)); CC_HIP(hipEventElapsedTime(&alone, e0, e1));
    CC_HIP(hipEventRecord(e0, a));
    CC_HIP(hipStreamWaitEvent(b, e0, 0));               // b starts no earlier than a's clock
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, ticks);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, ticks);
    CC_HIP(hipEventRecord(eb, b));
    CC_HIP(hipStreamWaitEvent(a, eb, 0));
    CC_HIP(hipEventRecord(e1, a));
    CC_HIP(hipEventSynchronize(e1)); CC_HIP(hipEventElapsedTime(&pair, e0, e1));
  }
  hipEventDestroy(e0); hipEventDestroy(e1); hipEventDestroy(eb);
  CC_HIP(hipGetLastError());
  if (getenv("CLEARCAM_VERBOSE")) fprintf(stderr, "[clearcam] stream probe: one kernel %.3f ms, one per stream %.3f ms\n", alone, pair);
  return pair < 1.5f * alone;
}

// The stream pool (kernels.h): per device, streams parked by dead handles for the next one
static std::mutex g_pool_mu;
static std::map<int, std::deque<hipStream_t>> g_pool;
hipStream_t pool_stream_get(int device) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto& q = g_pool[device];
    if (!q.empty()) { hipStream_t s = q.front(); q.pop_front(); return s; }
  }
  hipStream_t s = nullptr;
  CC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return s;
}
void pool_stream_put(int device, hipStream_t s) {
  if (!s) return;
  // a stream left in capture state by a failed capture, or one whose work faulted, must not be handed to the next handle
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
  const bool healthy = !capturing && hipStreamSynchronize(s) == hipSuccess;
  static const bool pooled = [] { const char* e = getenv("CLEARCAM_STREAM_POOL"); return !(e && atoi(e) == 0); }();
  if (!pooled || !healthy) { hipStreamDestroy(s); return; }   // CLEARCAM_STREAM_POOL=0: the round-3 behaviour, for A/B (tests/test_gpu_streams.py)
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_pool[device].push_back(s);
}

// Slots of a handle (batches in flight) must not share a hardware queue: the runtime maps streams onto a small pool of queues
// (GPU_MAX_HW_QUEUES, 4 unless the environment says otherwise, handed out least-used first), packets of one queue run in order, and
// two slots on one queue do not overlap at all.  So a new slot's stream is PROBED against the streams it has to run beside and
// replaced until it overlaps with all of them; rejected streams stay alive until the end so that the runtime moves on to another
// queue.  (Stream priority classes have queue pools of their own and would separate three slots by construction, but strict
// priority only fills gaps: 10.7 ms per B = 64 detect step against 10.1 with three equal slots.)
void grow_slot_streams(int device, hipStream_t base, std::vector<hipStream_t>& slots, int n_extra) {
  std::vector<hipStream_t> rejected;
  // Rejected streams are held out of the pool until the end, so a call never draws the same stream twice: it works through what the pool
  // holds (possibly the very streams an earlier call rejected for this base - they share its hardware queue) and then through fresh
  // ones.  The attempt budget therefore covers the pooled streams PLUS twelve fresh ones; the pool only grows when everything it held
  // was rejected (an unconditional "fresh after the first rejection" grew it by a stream per depth change: tools/dev/soak.py flight).
  size_t pooled = 0;
  { std::lock_guard<std::mutex> lk(g_pool_mu); pooled = g_pool[device].size(); }
  while ((int)slots.size() < n_extra) {
    hipStream_t t = nullptr;
    const int budget = (int)pooled + 12;
    for (int attempt = 0; attempt < budget; ++attempt) {
      t = pool_stream_get(device);
      bool ok = streams_overlap(base, t);
      for (size_t j = 0; ok && j < slots.size(); ++j) ok = streams_overlap(slots[j], t);
      if (ok) break;
      if (attempt == budget - 1) {
        fprintf(stderr, "[clearcam] warning: no stream found that overlaps with the handle's other slots after %d attempts: batches in flight on this slot will serialise\n", budget);
        break;
      }
      rejected.push_back(t); t = nullptr;               // held until the end, so that the pool / the runtime moves on to another queue
    }
    slots.push_back(t);
  }
  for (hipStream_t t : rejected) pool_stream_put(device, t);
}

// A handle's slots for n batches in flight: slot 0 runs on `base`, slots 1 .. n-1 on slot_stream (surplus streams go back to the pool,
// new ones are probed: kernels on any two of them really run side by side), one completion event per slot.  The caller has idled the streams.
void resize_slots(int device, hipStream_t base, std::vector<hipStream_t>& slot_stream, std::vector<hipEvent_t>& slot_done, int n) {
  while ((int)slot_stream.size() > n - 1) { pool_stream_put(device, slot_stream.back()); slot_stream.pop_back(); }
  grow_slot_streams(device, base, slot_stream, n - 1);
  while ((int)slot_done.size() > n) { hipEventDestroy(slot_done.back()); slot_done.pop_back(); }
  while ((int)slot_done.size() < n) { hipEvent_t e; CC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); slot_done.push_back(e); }
}

}  // namespace cc

extern "C" {

const char* cc_last_error(void) { return g_err.c_str(); }
int cc_version(void) { return 100; }
int cc_device_count(int* n) { CC_API_BEGIN CC_HIP(hipGetDeviceCount(n)); CC_API_END }

}  // extern "C"
