// Text-described alerts at ingest: the fourth step of the crop path (clearcam.py:1289-1307), for a whole batch in one call.
//
// The reference walks the camera's alerts for every crop: skip the ones that fired less than 60 s ago, are inactive or have no
// description, take `desc_emb @ emb.T`, and the first one strictly above its threshold notifies and ends the walk.  So a crop fires at
// most one alert, and an alert that fired is spent for the crops behind it.  Here the standing table of descriptions lives on the
// device (cc_watch_set, index in the table = priority) and cc_watch_match answers a batch of embeddings with two launches on one stream:
//
//   watch_hits_kernel     every (crop, alert) score into a (B, A) scratch, and the bit `score > threshold[a] && group[a] == crop_group[b]`
//                         into hits[b][a / 32].  It is scan_kernel (index.hip) with the roles turned round: the crops are the rows
//                         (16 lanes a crop, four crops a wave), the descriptions are the queries in LDS, and the additions run in
//                         scan_kernel's order exactly (lane `sub` takes elements 64 t + 4 sub + {0,1,2,3}, t ascending, fma from 0; then the
//                         16-lane xor butterfly 8, 4, 2, 1).  A score is therefore the score an f32 EmbeddingIndex holding the crop gives a
//                         single query with the description, bit for bit, and depends on nothing but its pair.
//   watch_resolve_kernel  the sequential rule on one wave: lane l keeps word l of the armed mask in a register; per crop, in order,
//                         hits & armed, a ballot, the lowest lane's lowest bit fires, and that lane clears the bit.  No barrier, no LDS.
//
// Every word of `hits`, every score and every output is written by exactly one lane with a plain store; the two launches are ordered by the
// stream alone.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>
#include "kernels.h"
#include "../../include/clearcam_hip.h"

using namespace cc;

namespace {
constexpr int kMaxAlerts = CC_WATCH_MAX_ALERTS;   // one lane of one wave owns one 32-bit word of the armed mask: 64 x 32
constexpr int kMaskWords = kMaxAlerts / 32;
static_assert(kMaskWords == 64, "the resolve kernel keeps the armed mask in one wave");
constexpr int kMaxBatch = 1 << 20;                // crops per call: keeps B * A and every grid dimension far inside 32 bits
}

struct cc_watch {
  int dim = 0, device = 0, A = 0;
  hipStream_t stream = nullptr;
  float* desc = nullptr; size_t desc_cap = 0;     // (A, dim) descriptions, priority order
  float* thr = nullptr; int* grp = nullptr; size_t meta_cap = 0;   // (A) thresholds and camera numbers
  float* emb = nullptr; size_t emb_cap = 0;       // (B, dim) device copy of a host batch
  unsigned* in_dev = nullptr; size_t in_cap = 0;  // the small inputs of a call, one upload: kMaskWords words of the armed mask, then B crop cameras
  float* scores = nullptr; size_t scores_cap = 0; // (B, A) scratch
  unsigned* hits = nullptr; size_t hits_cap = 0;  // (B, ceil(A / 32)) hit words
  char* pin = nullptr; size_t pin_cap = 0;        // pinned, device-visible host staging: small host inputs in; host results are written into it by the kernel
  hipEvent_t staged = nullptr;                    // behind the last copy that read `pin`: the next call waits for it before refilling
};

namespace {

// One block: 16 crops (four waves of four) against the 32 alerts of one word of `hits`, P descriptions per pass through LDS.
// Alerts at or past A are zero rows in LDS and no bits.  crop_grp null (cc_watch_scores): scores only.
template <int P>
__global__ __launch_bounds__(256) void watch_hits_kernel(const float* __restrict__ emb, const float* __restrict__ desc, const float* __restrict__ thr,
                                                          const int* __restrict__ grp, const int* __restrict__ crop_grp,
                                                          float* __restrict__ scores, unsigned* __restrict__ hits, int B, int A, int dim) {
  extern __shared__ float4 qs[];                                  // P x dim/4
  const int nchunk = dim >> 2;
  const int lane = threadIdx.x & 63, sub = lane & 15;
  const int b = blockIdx.x * 16 + (threadIdx.x >> 6) * 4 + (lane >> 4);
  const bool live = b < B;
  const int word = blockIdx.y, W = (A + 31) >> 5;
  const float4* e = reinterpret_cast<const float4*>(emb + (size_t)(live ? b : B - 1) * dim) + sub;
  const int steps = dim >> 6;                                     // 16 lanes x 4 floats per step; a multiple of 4
  const int cg = (crop_grp && live) ? crop_grp[b] : -1;
  unsigned bits = 0;
  for (int a0 = word * 32; a0 < word * 32 + 32 && a0 < A; a0 += P) {
    __syncthreads();                                              // the previous pass has read its descriptions
    for (int i = threadIdx.x; i < P * nchunk; i += 256) {
      const int a = a0 + i / nchunk;
      qs[i] = a < A ? reinterpret_cast<const float4*>(desc)[(size_t)a0 * nchunk + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    float acc[P];
#pragma unroll
    for (int c = 0; c < P; ++c) acc[c] = 0.f;
    for (int t0 = 0; t0 < steps; t0 += 4) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = e[(t0 + u) * 16];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < P; ++c) {
          const float4 w = qs[c * nchunk + (t0 + u) * 16 + sub];
          acc[c] = fmaf(v[u].x, w.x, acc[c]); acc[c] = fmaf(v[u].y, w.y, acc[c]); acc[c] = fmaf(v[u].z, w.z, acc[c]); acc[c] = fmaf(v[u].w, w.w, acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < P; ++c) {
      float sum = acc[c];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      const int a = a0 + c;
      if (sub == 0 && live && a < A) {
        scores[(size_t)b * A + a] = sum;
        if (crop_grp && sum > thr[a] && grp[a] == cg) bits |= 1u << (a & 31);   // a NaN score compares false
      }
    }
  }
  if (crop_grp && sub == 0 && live) hits[(size_t)b * W + word] = bits;
}

// The reference's walk for the crops in order, on one wave.  Lane l owns word l of the armed mask (zero at and past ceil(A / 32), tail bits
// of the last word zero: the host builds it so).  Per crop: hits & armed, a ballot, the lowest lane's lowest set bit fires and that lane
// clears it.  Nothing in that chain touches memory: the hit words of kResolveStep crops are loaded together before they are walked (data of
// the launch before, so when they are loaded changes nothing), the firing alert of crop b is a scalar (two find-first-bits and one lane
// read) kept by lane b & 63, and after every 64 crops each lane writes its crop's pair, the score read from the scratch.  A load or a store
// inside the walk costs one memory latency per crop: 66 - 100 us for 255 crops against 19 - 27 us this way (docs/measurement.md).
constexpr int kResolveStep = 16;

__global__ __launch_bounds__(64) void watch_resolve_kernel(const unsigned* __restrict__ hits, const float* __restrict__ scores,
                                                            const unsigned* __restrict__ armed_in, int* __restrict__ alert, float* __restrict__ score,
                                                            int B, int A) {
  const int l = threadIdx.x, W = (A + 31) >> 5;
  unsigned armed = armed_in[l];
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int nb = min(64, B - b0);
    int mine = -1;                                                // the alert crop b0 + l fires
    for (int c0 = 0; c0 < nb; c0 += kResolveStep) {
      unsigned hw[kResolveStep];
#pragma unroll
      for (int i = 0; i < kResolveStep; ++i) hw[i] = (l < W && c0 + i < nb) ? hits[(size_t)(b0 + c0 + i) * W + l] : 0u;
#pragma unroll
      for (int i = 0; i < kResolveStep; ++i) {
        const unsigned w = hw[i] & armed;
        const unsigned long long any = __ballot(w != 0u);
        int a = -1;
        if (any != 0ull) {                                        // uniform
          const int first = __ffsll(any) - 1;                     // scalar: the lowest lane with a live hit
          const int bit = __ffs(__builtin_amdgcn_readlane(w, first)) - 1;   // its lowest set bit, read across as a scalar too
          a = first * 32 + bit;
          if (l == first) armed &= ~(1u << bit);
        }
        if (l == c0 + i) mine = a;
      }
    }
    if (l < nb) {
      const int b = b0 + l;
      alert[b] = mine;
      score[b] = mine >= 0 ? scores[(size_t)b * A + mine] : 0.f;
    }
  }
}

void ensure(void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return;
  if (*p) hipFree(*p);
  *p = nullptr; *cap = 0;
  CC_HIP(hipMalloc(p, bytes + 256));
  *cap = bytes;
}

// The pinned buffer may be refilled once the last copy out of it has run (normally long ago: nothing waits here in practice).
void pin_begin(cc_watch* h, size_t bytes) {
  CC_HIP(hipEventSynchronize(h->staged));
  if (h->pin_cap >= bytes) return;
  if (h->pin) hipHostFree(h->pin);
  h->pin = nullptr; h->pin_cap = 0;
  CC_HIP(hipHostMalloc((void**)&h->pin, bytes, hipHostMallocDefault));
  h->pin_cap = bytes;
}

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// The batch on the device: the caller's pointer, or the handle's copy of a host batch (staged at pin + off).
const float* stage_emb(cc_watch* h, const float* emb, int B, int emb_on_device, size_t off, hipStream_t s) {
  if (emb_on_device) return emb;
  const size_t bytes = (size_t)B * h->dim * 4;
  ensure((void**)&h->emb, &h->emb_cap, bytes);
  memcpy(h->pin + off, emb, bytes);
  CC_HIP(hipMemcpyAsync(h->emb, h->pin + off, bytes, hipMemcpyHostToDevice, s));
  return h->emb;
}

void launch_hits(cc_watch* h, const float* emb, const int* crop_grp, int B, hipStream_t s) {
  ensure((void**)&h->scores, &h->scores_cap, (size_t)B * h->A * 4);
  const int W = (h->A + 31) / 32;
  if (crop_grp) ensure((void**)&h->hits, &h->hits_cap, (size_t)B * W * 4);
  const dim3 grid((unsigned)((B + 15) / 16), (unsigned)W);
  // P descriptions per pass, as many of 8 as 64 KB of LDS hold: 8 up to dim 2048, 4 beyond (dim <= 4096); both divide a word's 32 alerts
  if (h->dim <= 2048)
    hipLaunchKernelGGL(watch_hits_kernel<8>, grid, dim3(256), (size_t)8 * h->dim * 4, s, emb, h->desc, h->thr, h->grp, crop_grp, h->scores, h->hits, B, h->A, h->dim);
  else
    hipLaunchKernelGGL(watch_hits_kernel<4>, grid, dim3(256), (size_t)4 * h->dim * 4, s, emb, h->desc, h->thr, h->grp, crop_grp, h->scores, h->hits, B, h->A, h->dim);
  CC_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

int cc_watch_create(cc_watch** h, int dim, int device) {
  CC_API_BEGIN
  CC_CHECK(h, "null argument");
  CC_CHECK(dim > 0 && dim % 256 == 0 && dim <= 4096, "a watch list needs dim % 256 == 0 and dim <= 4096");
  int n = 0; CC_HIP(hipGetDeviceCount(&n));
  CC_CHECK(n > 0 && device >= 0 && device < n, "no such HIP device");
  CC_HIP(hipSetDevice(device));
  std::unique_ptr<cc_watch> x(new cc_watch());
  x->dim = dim; x->device = device;
  CC_HIP(hipEventCreateWithFlags(&x->staged, hipEventDisableTiming));
  x->stream = pool_stream_get(device);
  *h = x.release();
  CC_API_END
}

int cc_watch_set(cc_watch* h, const float* desc, const float* threshold, const int32_t* group, int A) {
  CC_API_BEGIN
  CC_CHECK(h && A >= 0, "bad argument");
  CC_CHECK(A <= kMaxAlerts, "a watch list holds at most 2048 alerts (one lane of one wave owns one 32-bit word of the armed mask)");
  CC_CHECK(A == 0 || (desc && threshold && group), "null argument");
  for (int a = 0; a < A; ++a) CC_CHECK(group[a] >= 0 && group[a] < (1 << 24), "alert groups must be in [0, 2^24)");
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));              // a match on our stream may still be reading the table
  if (A) {
    ensure((void**)&h->desc, &h->desc_cap, (size_t)A * h->dim * 4);
    if (h->meta_cap < (size_t)A) {
      if (h->thr) hipFree(h->thr);
      if (h->grp) hipFree(h->grp);
      h->thr = nullptr; h->grp = nullptr; h->meta_cap = 0;
      CC_HIP(hipMalloc((void**)&h->thr, (size_t)A * 4 + 256)); CC_HIP(hipMalloc((void**)&h->grp, (size_t)A * 4 + 256));
      h->meta_cap = (size_t)A;
    }
    h->A = 0;                                            // a failed copy leaves an empty table, not a half-written one
    CC_HIP(hipMemcpy(h->desc, desc, (size_t)A * h->dim * 4, hipMemcpyHostToDevice));
    CC_HIP(hipMemcpy(h->thr, threshold, (size_t)A * 4, hipMemcpyHostToDevice));
    CC_HIP(hipMemcpy(h->grp, group, (size_t)A * 4, hipMemcpyHostToDevice));
  }
  h->A = A;
  CC_API_END
}

int cc_watch_size(cc_watch* h, int* A) {
  CC_API_BEGIN
  CC_CHECK(h && A, "null argument");
  *A = h->A;
  CC_API_END
}

int cc_watch_scores(cc_watch* h, const float* emb, int B, int emb_on_device, float* scores, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && B >= 0 && B <= kMaxBatch, "bad argument (B must be in [0, 2^20])");
  if (B == 0 || h->A == 0) return 0;
  CC_CHECK(emb && scores, "null argument");
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (!emb_on_device) pin_begin(h, (size_t)B * h->dim * 4);
  const float* e = stage_emb(h, emb, B, emb_on_device, 0, s);
  if (!emb_on_device) CC_HIP(hipEventRecord(h->staged, s));
  launch_hits(h, e, nullptr, B, s);
  CC_HIP(hipMemcpyAsync(scores, h->scores, (size_t)B * h->A * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  if (!on_device) CC_HIP(hipStreamSynchronize(s));
  CC_API_END
}

int cc_watch_match(cc_watch* h, const float* emb, int B, int emb_on_device, const int32_t* crop_group, const uint8_t* armed,
                   int32_t* alert, float* score, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && B >= 0 && B <= kMaxBatch, "bad argument (B must be in [0, 2^20])");
  if (B == 0) return 0;
  CC_CHECK(emb && crop_group && alert && score, "null argument");
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const int A = h->A;
  if (A == 0) {                                          // nothing to score: every crop fires nothing
    if (on_device) {
      CC_HIP(hipMemsetAsync(alert, 0xff, (size_t)B * 4, s));
      CC_HIP(hipMemsetAsync(score, 0, (size_t)B * 4, s));
    } else {
      for (int b = 0; b < B; ++b) { alert[b] = -1; score[b] = 0.f; }
    }
    return 0;
  }
  // pinned layout: [armed words, crop groups | results: alerts, scores (host outputs) | embeddings (host batch)]
  const size_t in_bytes = (size_t)(kMaskWords + B) * 4, off_res = up256(in_bytes), off_emb = off_res + (on_device ? 0 : up256((size_t)B * 8));
  pin_begin(h, off_emb + (emb_on_device ? 0 : (size_t)B * h->dim * 4));
  unsigned* words = reinterpret_cast<unsigned*>(h->pin);
  for (int w = 0; w < kMaskWords; ++w) {
    unsigned m = 0;
    for (int a = w * 32; a < std::min(A, w * 32 + 32); ++a) if (!armed || armed[a]) m |= 1u << (a & 31);
    words[w] = m;
  }
  memcpy(words + kMaskWords, crop_group, (size_t)B * 4);
  ensure((void**)&h->in_dev, &h->in_cap, in_bytes);
  CC_HIP(hipMemcpyAsync(h->in_dev, words, in_bytes, hipMemcpyHostToDevice, s));
  const int* crop_dev = reinterpret_cast<const int*>(h->in_dev + kMaskWords);
  const float* e = stage_emb(h, emb, B, emb_on_device, off_emb, s);
  int* alert_out = alert; float* score_out = score;
  if (!on_device) {                                      // the B pairs go straight into pinned host memory, as the index's small results do
    alert_out = reinterpret_cast<int*>(h->pin + off_res); score_out = reinterpret_cast<float*>(h->pin + off_res) + B;
  }
  launch_hits(h, e, crop_dev, B, s);
  hipLaunchKernelGGL(watch_resolve_kernel, dim3(1), dim3(64), 0, s, h->hits, h->scores, h->in_dev, alert_out, score_out, B, A);
  CC_HIP(hipGetLastError());
  if (!on_device) {
    CC_HIP(hipStreamSynchronize(s));
    memcpy(alert, alert_out, (size_t)B * 4); memcpy(score, score_out, (size_t)B * 4);
  } else {
    CC_HIP(hipEventRecord(h->staged, s));                // the uploads above read `pin`; the next call waits for them only
  }
  CC_API_END
}

void cc_watch_destroy(cc_watch* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->staged) { hipEventSynchronize(h->staged); hipEventDestroy(h->staged); }
  for (void* p : {(void*)h->desc, (void*)h->thr, (void*)h->grp, (void*)h->emb, (void*)h->in_dev, (void*)h->scores, (void*)h->hits}) if (p) hipFree(p);
  if (h->pin) hipHostFree(h->pin);
  pool_stream_put(h->device, h->stream);                 // parked, never destroyed (kernels.h)
  delete h;
}

}  // extern "C"
