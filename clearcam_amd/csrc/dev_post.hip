// Development entries that run ONE launch of a detector post-processing kernel outside any plan, on inputs the caller crafts:
// cc_dev_decode (decode_kernel), cc_dev_head_tail (head_tail_kernel, weights packed by the detector's own pack_convs as Builder::head_level
// packs them) and cc_dev_topk_nms (topk_nms_kernel, uniform or ragged).  Each validates its arguments and launches nothing on bad input,
// goes through the production launcher, synchronises the stream and frees what it allocated.  cc_dev_blaze_post is in blaze.hip, beside
// the kernel it launches.
#include <cmath>
#include "yolo_plan.h"

using namespace cc;

namespace {

struct Owner {                                           // device allocations of one call
  std::vector<void*> p;
  ~Owner() { for (void* q : p) hipFree(q); }
  template <class T> T* alloc(size_t n) { void* d = nullptr; CC_HIP(hipMalloc(&d, n * sizeof(T) + 256)); p.push_back(d); return (T*)d; }
  template <class T> T* upload(const T* host, size_t n) {
    T* d = alloc<T>(n);
    CC_HIP(hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// B > 0, every level non-empty, A = sum H*W and B*A inside int; returns A
int check_levels(int B, const int* H, const int* W) {
  CC_CHECK(H && W && B > 0, "bad shape");
  long A = 0;
  for (int l = 0; l < 3; ++l) { CC_CHECK(H[l] > 0 && W[l] > 0 && (long)H[l] * W[l] < (1L << 24), "bad level size"); A += (long)H[l] * W[l]; }
  CC_CHECK(A > 0 && (long)B * A < (1L << 28), "too many anchors");
  return (int)A;
}

// the device counter of DecodeP / HeadTailP::nonfinite: zeroed before the launch, read back after it
struct Counter {
  int* dev;
  explicit Counter(Owner& o) : dev(o.alloc<int>(1)) { CC_HIP(hipMemset(dev, 0, sizeof(int))); }
  int read() const { int v = 0; CC_HIP(hipMemcpy(&v, dev, sizeof(int), hipMemcpyDeviceToHost)); return v; }
};

}  // namespace

extern "C" {

int cc_dev_decode(const float* const* raw_dev, const int* H, const int* W, int B, const float* dfl_w16, float conf, float* det_dev,
                  int* nonfinite, void* stream) {
  CC_API_BEGIN
  CC_CHECK(raw_dev && dfl_w16 && det_dev && nonfinite, "null argument");
  const int A = check_levels(B, H, W);
  for (int l = 0; l < 3; ++l) CC_CHECK(raw_dev[l] && aligned16(raw_dev[l]), "raw maps must be non-null and 16-byte aligned (float4 loads)");
  Owner own;
  DecodeP p{};
  for (int l = 0; l < 3; ++l) { p.raw[l] = raw_dev[l]; p.H[l] = H[l]; p.W[l] = W[l]; }
  p.B = B; p.A = A; p.dfl_w = own.upload(dfl_w16, 16); p.conf = conf; p.det = det_dev;
  Counter cnt(own);
  p.nonfinite = cnt.dev;
  launch_decode(p, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  *nonfinite = cnt.read();
  CC_API_END
}

int cc_dev_head_tail(int dtype, int ch, const void* const* bx_dev, const void* const* cl_dev, const float* const* w2, const float* const* b2,
                     const float* const* w3, const float* const* b3, const int* H, const int* W, int B, const float* dfl_w16, float conf,
                     float* det_dev, int* nonfinite, void* stream) {
  std::vector<PackedConv> packed;                        // pack_convs hands its device memory to the caller
  auto release = [&]() { for (PackedConv& pc : packed) { hipFree(pc.w); hipFree(pc.bias); } packed.clear(); };
  try {
    CC_CHECK(bx_dev && cl_dev && w2 && b2 && w3 && b3 && dfl_w16 && det_dev && nonfinite, "null argument");
    CC_CHECK(dtype == F16 || dtype == BF16 || dtype == F16S, "dtype must be 1 (f16), 2 (bf16) or 3 (f16s)");
    const int split = dtype == F16S, dt = storage_dtype(dtype);
    CC_CHECK(head_tail_supported(dt, ch, split), "fused DDetect tail: unsupported dtype / class-branch width");
    const int A = check_levels(B, H, W);
    for (int l = 0; l < 3; ++l)
      CC_CHECK(bx_dev[l] && cl_dev[l] && aligned16(bx_dev[l]) && aligned16(cl_dev[l]) && w2[l] && b2[l] && w3[l] && b3[l],
               "activations must be non-null and 16-byte aligned (uint4 loads), weights and biases non-null");
    Owner own;
    HeadTailP q{};
    for (int l = 0; l < 3; ++l) {                          // as Builder::head_level: cv2[l][2] with its four groups densified, cv3[l][2]
      HostTensor t2, u2, t3, u3;
      t2.shape = {64, 16, 1, 1}; t2.data.assign(w2[l], w2[l] + 64 * 16); u2.shape = {64}; u2.data.assign(b2[l], b2[l] + 64);
      t3.shape = {80, ch, 1, 1}; t3.data.assign(w3[l], w3[l] + (size_t)80 * ch); u3.shape = {80}; u3.data.assign(b3[l], b3[l] + 80);
      packed.push_back(pack_convs(dt, {&t2}, {&u2}, {4}, 0, split));
      const PackedConv c2 = packed.back();
      packed.push_back(pack_convs(dt, {&t3}, {&u3}, {1}, 0, split));
      const PackedConv c3 = packed.back();
      CC_CHECK(c2.cin == 64 && c2.cout == 64 && c2.k == 1 && c3.cin == ch && c3.cout == 80 && c3.k == 1, "fused DDetect tail: unexpected conv shapes");
      q.bx[l] = bx_dev[l]; q.cl[l] = cl_dev[l];
      q.w2[l] = c2.w; q.w3[l] = c3.w; q.b2[l] = c2.bias; q.b3[l] = c3.bias; q.kw2 = c2.kw; q.kw3 = c3.kw;
      q.split = c2.split; q.os2[l] = c2.oscale; q.os3[l] = c3.oscale;
      q.H[l] = H[l]; q.W[l] = W[l];
    }
    q.B = B; q.A = A; q.ch = ch; q.dfl_w = own.upload(dfl_w16, 16); q.conf = conf; q.det = det_dev;
    Counter cnt(own);
    q.nonfinite = cnt.dev;
    launch_head_tail(dt, q, (hipStream_t)stream);
    CC_HIP(hipStreamSynchronize((hipStream_t)stream));
    *nonfinite = cnt.read();
    release();
    return 0;
  } catch (const cc::Error& e) { release(); cc::set_error(e.what()); return e.code; }
  catch (const std::exception& e) { release(); cc::set_error(e.what()); return -1; }
}

int cc_dev_topk_nms(const float* rows_dev, int B, int A, float iou_thr, const float* geometry, int ragged, float* out_dev, void* stream) {
  CC_API_BEGIN
  CC_CHECK(rows_dev && geometry && out_dev, "null argument");
  CC_CHECK(B > 0 && A > 0 && (long)B * A < (1L << 28), "bad shape");
  const int ng = ragged ? B : 1;
  for (int i = 0; i < ng; ++i) {
    const float* g = geometry + 5 * (size_t)i;
    CC_CHECK(std::isfinite(g[0]) && std::isfinite(g[1]) && g[2] > 0.f && std::isfinite(g[2]) && g[3] > 0.f && g[4] > 0.f, "bad geometry (pad_x, pad_y, gain, src_w, src_h)");
  }
  Owner own;
  NmsP p{};
  p.det = rows_dev; p.B = B; p.A = A; p.iou_thr = iou_thr; p.out = out_dev;
  if (!ragged) {
    p.pad_x = geometry[0]; p.pad_y = geometry[1]; p.gain = geometry[2]; p.src_w = geometry[3]; p.src_h = geometry[4];
    launch_topk_nms(p, (hipStream_t)stream);
  } else {
    std::vector<FrameDesc> desc((size_t)B, FrameDesc{});   // only the five scale fields: all the NMS launch reads
    for (int b = 0; b < B; ++b) {
      const float* g = geometry + 5 * (size_t)b;
      desc[b].fpad_x = g[0]; desc[b].fpad_y = g[1]; desc[b].gain = g[2]; desc[b].src_w = g[3]; desc[b].src_h = g[4];
    }
    launch_topk_nms_ragged(p, own.upload(desc.data(), desc.size()), (hipStream_t)stream);
  }
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  CC_API_END
}

}  // extern "C"
