// Crop preprocessing for the CLIP image tower: OpenCV-compatible INTER_CUBIC resize of variable-size uint8 HWC crops
// to S x S, then /255, (x-0.5)/0.5 and HWC -> CHW.  Replaces the host-side `ObjectFinder.preprocess`
// (models/objects.py:237-242: cv2.resize(img,(224,224),INTER_CUBIC) -> f32/255 -> (x-0.5)/0.5 -> transpose), which at
// 10 k crops per search re-index is the step in front of `precompute_embedding`.
//
// The arithmetic follows cv::resize's portable 8-bit cubic path (OpenCV 4.10 imgproc/src/resize.cpp, the version
// requirements.txt:3 pins): source coordinate fx = (float)((d+0.5)*scale-0.5) with scale = 1/(dst/src) in double,
// four float cubic weights (A = -0.75) rounded to 11-bit fixed point (short), borders replicated, horizontal pass in
// int32 without rounding, vertical pass (sum + 2^21) >> 22, saturate to uint8.  Integer accumulation makes the two
// separable passes equal to one 16-tap double sum, which is what each thread evaluates.  HBM-bound byte work: no LDS,
// one thread per output pixel, taps served by L1/L2 (a crop is a few hundred KB).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "kernels.h"
#include "../../include/clearcam_hip.h"

namespace cc {
namespace {

struct CropTab { long long off; int h, w; int pad; };

__device__ __forceinline__ void cubic_coeffs(float x, short (&c)[4]) {
  const float A = -0.75f;
  float f[4];
  f[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
  f[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  f[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
  f[3] = 1.f - f[0] - f[1] - f[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int v = __float2int_rn(f[k] * 2048.f);                 // saturate_cast<short>(float) = cvRound then clamp
    v = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
    c[k] = (short)v;
  }
}

// one axis: destination index d -> first source tap (s-1) and the four fixed-point weights
__device__ __forceinline__ int axis(int d, int src, int dst, short (&c)[4]) {
  const double inv_scale = (double)dst / (double)src;
  const double scale = 1.0 / inv_scale;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  cubic_coeffs(f, c);
  return s;
}

__global__ __launch_bounds__(256) void crop_cubic_kernel(const uint8_t* __restrict__ pix, const CropTab* __restrict__ tab,
                                                         int S, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= S * S) return;
  const int dy = idx / S, dx = idx - dy * S;
  const CropTab t = tab[b];
  const uint8_t* src = pix + t.off;
  short ax[4], ay[4];
  const int sx = axis(dx, t.w, S, ax), sy = axis(dy, t.h, S, ay);
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int y = sy - 1 + r; y = y < 0 ? 0 : (y >= t.h ? t.h - 1 : y);
    const uint8_t* row = src + (size_t)y * t.w * 3;
    int hs[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int x = sx - 1 + k; x = x < 0 ? 0 : (x >= t.w ? t.w - 1 : x);
      const uint8_t* p = row + x * 3;
      hs[0] += (int)p[0] * ax[k]; hs[1] += (int)p[1] * ax[k]; hs[2] += (int)p[2] * ax[k];
    }
    acc[0] += hs[0] * ay[r]; acc[1] += hs[1] * ay[r]; acc[2] += hs[2] * ay[r];
  }
  float* o = out + (size_t)b * 3 * S * S + idx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int v = (acc[c] + (1 << 21)) >> 22;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    o[(size_t)c * S * S] = __fdiv_rn(__fdiv_rn((float)v, 255.0f) - 0.5f, 0.5f);
  }
}

// ---- cv2.resize(INTER_LINEAR) and cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) for 8-bit 3-channel images ----------
// The two OpenCV calls `ObjectFinder.img_to_face` makes around BlazeFace (models/objects.py:247,318,332), restated from
// OpenCV 4.10's fixed-point paths (oracle/cv_warp_oracle.py has the derivation); one thread per output pixel.
struct ResizeP { const uint8_t* src; int H, W; uint8_t* dst; int dh, dw; int area2; };
struct WarpP { const uint8_t* src; int H, W; uint8_t* dst; int dh, dw; double m[6]; };   // m = the INVERTED 2x3 matrix
constexpr int kFace = 112;     // side of the aligned face (ObjectFinder.FACE_SIZE)

__device__ __forceinline__ void linear_axis(int d, int src, int dst, int& s0, int& s1, int& a0, int& a1) {
  const double inv_scale = (double)dst / (double)src;
  const double scale = 1.0 / inv_scale;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; }
  s0 = s; s1 = min(s + 1, src - 1);
  a0 = max(-32768, min(32767, __float2int_rn((1.0f - f) * 2048.f)));
  a1 = max(-32768, min(32767, __float2int_rn(f * 2048.f)));
}

// one pixel (dy, dx) of cv2.resize(src H x W -> dh x dw, INTER_LINEAR) written to o[0..2]; area2 = the exact 2x2 decimation,
// which OpenCV switches to INTER_AREA.  Shared by resize_linear_kernel and face_letterbox_kernel: one definition, the same bytes.
// (dh, dw) == (H, W) needs no case of its own: the weights come out as (2048, 0) and ((2048 * (v * 128)) >> 16) + 2 >> 2 = v.
__device__ __forceinline__ void resize_linear_px(const uint8_t* __restrict__ src, int H, int W, int dh, int dw, int area2, int dy, int dx,
                                                 uint8_t* __restrict__ o) {
  if (area2) {
    const uint8_t* r0 = src + ((size_t)(2 * dy) * W + 2 * dx) * 3;
    const uint8_t* r1 = r0 + (size_t)W * 3;
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(((int)r0[c] + r0[3 + c] + r1[c] + r1[3 + c] + 2) >> 2);
    return;
  }
  int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
  linear_axis(dx, W, dw, x0, x1, ax0, ax1);
  linear_axis(dy, H, dh, y0, y1, ay0, ay1);
  const uint8_t* r0 = src + (size_t)y0 * W * 3;
  const uint8_t* r1 = src + (size_t)y1 * W * 3;
  for (int c = 0; c < 3; ++c) {
    const int h0 = (int)r0[x0 * 3 + c] * ax0 + (int)r0[x1 * 3 + c] * ax1;
    const int h1 = (int)r1[x0 * 3 + c] * ax0 + (int)r1[x1 * 3 + c] * ax1;
    const int v = (((ay0 * (h0 >> 4)) >> 16) + ((ay1 * (h1 >> 4)) >> 16) + 2) >> 2;
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

__global__ __launch_bounds__(256) void resize_linear_kernel(const ResizeP p) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.dh * p.dw) return;
  const int dy = idx / p.dw, dx = idx - dy * p.dw;
  resize_linear_px(p.src, p.H, p.W, p.dh, p.dw, p.area2, dy, dx, p.dst + (size_t)idx * 3);
}

// Ragged letterbox of the batched face path: crop b of the packed buffer -> resize_linear to (dh, dw) -> centred in an S x S frame of
// zeros (ObjectFinder.img_to_face's resize_linear + copy_make_border), every pixel of the frame written: no memset.  grid (S*S/256, B).
__global__ __launch_bounds__(256) void face_letterbox_kernel(const uint8_t* __restrict__ pix, const FaceBoxRec* __restrict__ rec, int S,
                                                             uint8_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= S * S) return;
  const int y = idx / S, x = idx - y * S;
  const FaceBoxRec r = rec[b];
  uint8_t* o = out + ((size_t)b * S * S + idx) * 3;
  const int dy = y - r.top, dx = x - r.left;
  if ((unsigned)dy >= (unsigned)r.dh || (unsigned)dx >= (unsigned)r.dw) { o[0] = 0; o[1] = 0; o[2] = 0; return; }
  resize_linear_px(pix + r.off, r.h, r.w, r.dh, r.dw, r.area2, dy, dx, o);
}

// rows of a uint8 HWC image `stride` bytes apart (a view into a larger image has stride > 3 W); outside pixels are the constant border 0
struct MemFetch {
  const uint8_t* src; int H, W; size_t stride;
  __device__ __forceinline__ void operator()(int yy, int xx, int (&t)[3]) const {
    if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H) {
      const uint8_t* q = src + (size_t)yy * stride + (size_t)xx * 3;
      t[0] = q[0]; t[1] = q[1]; t[2] = q[2];
    } else { t[0] = 0; t[1] = 0; t[2] = 0; }
  }
};

// one pixel (dy, dx) of cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0), m = the INVERTED 2x3 matrix; `fetch(y, x, t)` gives the source
// pixel at an integer position (0 outside).  Shared by warp_affine_kernel and both levels of face_align_kernel.
template <class Fetch>
__device__ __forceinline__ void warp_affine_px(const double* m, int dy, int dx, const Fetch& fetch, int (&v)[3]) {
  const long long adelta = __double2ll_rn(m[0] * (double)dx * 1024.0), bdelta = __double2ll_rn(m[3] * (double)dx * 1024.0);
  const long long X0 = __double2ll_rn((m[1] * (double)dy + m[2]) * 1024.0) + 16, Y0 = __double2ll_rn((m[4] * (double)dy + m[5]) * 1024.0) + 16;
  const long long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  long long sxl = X >> 5, syl = Y >> 5;
  sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl); syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
  const int sx = (int)sxl, sy = (int)syl, fx = (int)(X & 31), fy = (int)(Y & 31);
  const int w00 = 32 * (32 - fy) * (32 - fx), w01 = 32 * (32 - fy) * fx, w10 = 32 * fy * (32 - fx), w11 = 32 * fy * fx;
  int t00[3], t01[3], t10[3], t11[3];
  fetch(sy, sx, t00); fetch(sy, sx + 1, t01); fetch(sy + 1, sx, t10); fetch(sy + 1, sx + 1, t11);
  for (int c = 0; c < 3; ++c) {
    const int s = (t00[c] * w00 + t01[c] * w01 + t10[c] * w10 + t11[c] * w11 + (1 << 14)) >> 15;
    v[c] = s < 0 ? 0 : (s > 255 ? 255 : s);
  }
}

__global__ __launch_bounds__(256) void warp_affine_kernel(const WarpP p) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.dh * p.dw) return;
  const int dy = idx / p.dw, dx = idx - dy * p.dw;
  int v[3];
  warp_affine_px(p.m, dy, dx, MemFetch{p.src, p.H, p.W, (size_t)p.W * 3}, v);
  uint8_t* o = p.dst + (size_t)idx * 3;
  o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
}

// The alignment tail of img_to_face for n faces at once: cut = crop[cy1:cy1+ch, cx1:cx1+cw]; level = warpAffine(cut, rot, (out_w, out_h));
// face = warpAffine(level, place, (112, 112))[:, :, ::-1].  A pixel of `level` is a pure function of its integer position - the first
// warp's rounded uint8 value inside [0, out_w) x [0, out_h), the border 0 outside - so the four taps the second warp needs are evaluated
// from the crop on the fly and `level` is never written: 4 x 12544 first-warp pixels per face instead of out_w x out_h.
// grid (49, n), one thread per output pixel (49 x 256 = 112 x 112).
struct AlignRec { long long off; int h, w, cx1, cy1, cw, ch, out_w, out_h; double rot[6], place[6]; };   // both matrices INVERTED

__global__ __launch_bounds__(256) void face_align_kernel(const uint8_t* __restrict__ pix, const AlignRec* __restrict__ rec, uint8_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int dy = idx / kFace, dx = idx - dy * kFace;
  const AlignRec r = rec[b];
  const MemFetch cut{pix + r.off + ((size_t)r.cy1 * r.w + r.cx1) * 3, r.ch, r.cw, (size_t)r.w * 3};
  auto level = [&](int yy, int xx, int (&t)[3]) {
    if ((unsigned)xx < (unsigned)r.out_w && (unsigned)yy < (unsigned)r.out_h) warp_affine_px(r.rot, yy, xx, cut, t);
    else { t[0] = 0; t[1] = 0; t[2] = 0; }
  };
  int v[3];
  warp_affine_px(r.place, dy, dx, level, v);
  uint8_t* o = out + ((size_t)b * kFace * kFace + idx) * 3;
  o[0] = (uint8_t)v[2]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[0];       // channels reversed: img_to_face's final [:, :, ::-1]
}

// cv::warpAffine inverts the forward matrix it is given (imgwarp.cpp): the one place both entry points do it
void invert_affine(const double* M, double* m) {
  for (int i = 0; i < 6; ++i) m[i] = M[i];
  double D = m[0] * m[4] - m[1] * m[3];
  D = D != 0 ? 1.0 / D : 0.0;
  const double A11 = m[4] * D, A22 = m[0] * D;
  m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22;
  const double b1 = -m[0] * m[2] - m[1] * m[5], b2 = -m[3] * m[2] - m[4] * m[5];
  m[2] = b1; m[5] = b2;
}

// cv::resize's test for the exact 2x2 decimation (resize.cpp: INTER_LINEAR becomes INTER_AREA)
int resize_is_area2(int H, int W, int dh, int dw) {
  const double sx = 1.0 / ((double)dw / W), sy = 1.0 / ((double)dh / H);
  return std::fabs(sx - 2.0) < 2.220446049250313e-16 && std::fabs(sy - 2.0) < 2.220446049250313e-16 && W % 2 == 0 && H % 2 == 0;
}

}  // namespace
}  // namespace cc

extern "C" int cc_crop_preprocess(const uint8_t* pixels, const int64_t* offsets, const int32_t* heights, const int32_t* widths,
                                  int B, int pixels_on_device, int out_size, float* out_dev, int device, void* stream) {
  using namespace cc;
  CC_API_BEGIN
  CC_CHECK(pixels && offsets && heights && widths && out_dev && B > 0 && out_size > 0, "bad argument");
  int n = 0; CC_HIP(hipGetDeviceCount(&n));
  CC_CHECK(n > 0 && device >= 0 && device < n, "no such HIP device");
  CC_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<CropTab> tab(B);
  size_t total = 0;
  for (int b = 0; b < B; ++b) {
    CC_CHECK(heights[b] > 0 && widths[b] > 0 && offsets[b] >= 0, "empty crop");
    tab[b] = CropTab{(long long)offsets[b], heights[b], widths[b], 0};
    total = std::max(total, (size_t)offsets[b] + (size_t)heights[b] * widths[b] * 3);
  }
  CropTab* dtab = nullptr; uint8_t* dpix = nullptr;
  CC_HIP(hipMallocAsync((void**)&dtab, sizeof(CropTab) * B, s));
  CC_HIP(hipMemcpyAsync(dtab, tab.data(), sizeof(CropTab) * B, hipMemcpyHostToDevice, s));
  const uint8_t* src = pixels;
  if (!pixels_on_device) {
    CC_HIP(hipMallocAsync((void**)&dpix, total, s));
    CC_HIP(hipMemcpyAsync(dpix, pixels, total, hipMemcpyHostToDevice, s));
    src = dpix;
  }
  const int px = out_size * out_size;
  hipLaunchKernelGGL(crop_cubic_kernel, dim3((px + 255) / 256, B), dim3(256), 0, s, src, dtab, out_size, out_dev);
  CC_HIP(hipGetLastError());
  CC_HIP(hipFreeAsync(dtab, s));
  if (dpix) CC_HIP(hipFreeAsync(dpix, s));
  CC_HIP(hipStreamSynchronize(s));          // `tab` and the caller's host buffers may go away on return
  CC_API_END
}


namespace {
// host image in -> kernel -> host image out, on `device`; small images, synchronous by design (the reference's cv2 calls are too)
template <class Launch>
void run_image_op(int device, const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t dst_bytes, Launch launch) {
  using namespace cc;
  int n = 0; CC_HIP(hipGetDeviceCount(&n));
  CC_CHECK(n > 0 && device >= 0 && device < n, "no such HIP device");
  CC_HIP(hipSetDevice(device));
  uint8_t *ds = nullptr, *dd = nullptr;
  CC_HIP(hipMalloc((void**)&ds, src_bytes + 16));
  if (hipMalloc((void**)&dd, dst_bytes + 16) != hipSuccess) { hipFree(ds); throw Error(-5, "hipMalloc failed"); }
  try {
    CC_HIP(hipMemcpy(ds, src, src_bytes, hipMemcpyHostToDevice));
    launch(ds, dd);
    CC_HIP(hipGetLastError());
    CC_HIP(hipMemcpy(dst, dd, dst_bytes, hipMemcpyDeviceToHost));
  } catch (...) { hipFree(ds); hipFree(dd); throw; }
  hipFree(ds); hipFree(dd);
}
}  // namespace

extern "C" int cc_cv_resize_linear_u8(const uint8_t* src, int H, int W, uint8_t* dst, int dh, int dw, int device) {
  using namespace cc;
  CC_API_BEGIN
  CC_CHECK(src && dst && H > 0 && W > 0 && dh > 0 && dw > 0, "bad argument");
  const int area2 = resize_is_area2(H, W, dh, dw);
  run_image_op(device, src, (size_t)H * W * 3, dst, (size_t)dh * dw * 3, [&](uint8_t* ds, uint8_t* dd) {
    if (dh == H && dw == W) { CC_HIP(hipMemcpy(dd, ds, (size_t)H * W * 3, hipMemcpyDeviceToDevice)); return; }
    const ResizeP p{ds, H, W, dd, dh, dw, area2};
    hipLaunchKernelGGL(resize_linear_kernel, dim3((dh * dw + 255) / 256), dim3(256), 0, 0, p);
  });
  CC_API_END
}

extern "C" int cc_cv_warp_affine_u8(const uint8_t* src, int H, int W, const double* M, uint8_t* dst, int dh, int dw, int device) {
  using namespace cc;
  CC_API_BEGIN
  CC_CHECK(src && dst && M && H > 0 && W > 0 && dh > 0 && dw > 0, "bad argument");
  double m[6]; invert_affine(M, m);
  run_image_op(device, src, (size_t)H * W * 3, dst, (size_t)dh * dw * 3, [&](uint8_t* ds, uint8_t* dd) {
    WarpP p{ds, H, W, dd, dh, dw, {m[0], m[1], m[2], m[3], m[4], m[5]}};
    hipLaunchKernelGGL(warp_affine_kernel, dim3((dh * dw + 255) / 256), dim3(256), 0, 0, p);
  });
  CC_API_END
}

// ---- batched face path: ragged letterbox in front of BlazeFace (blaze.hip: cc_face_locate) and the fused alignment behind it -----------
namespace cc {

void face_box_records(const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B, size_t pix_bytes, std::vector<FaceBoxRec>& rec) {
  rec.resize(B);
  for (int b = 0; b < B; ++b) {
    const int h = heights[b], w = widths[b];
    CC_CHECK(h > 0 && w > 0 && offsets[b] >= 0, "crop " + std::to_string(b) + ": empty crop");
    CC_CHECK((size_t)offsets[b] + (size_t)h * w * 3 <= pix_bytes, "crop " + std::to_string(b) + ": lies outside the packed buffer");
    const double scale = (double)kFaceBox / (double)std::max(h, w);          // img_to_face: 640 / max(h, w), int(h * scale) in double
    const int dh = (int)((double)h * scale), dw = (int)((double)w * scale);
    CC_CHECK(dh > 0 && dw > 0 && dh <= kFaceBox && dw <= kFaceBox, "crop " + std::to_string(b) + ": letterboxed side would be 0");
    rec[b] = FaceBoxRec{(long long)offsets[b], h, w, dh, dw, (kFaceBox - dh) / 2, (kFaceBox - dw) / 2, resize_is_area2(h, w, dh, dw), 0};
  }
}

void launch_face_letterbox(const uint8_t* pix_dev, const FaceBoxRec* rec_dev, int B, uint8_t* out_dev, hipStream_t stream) {
  hipLaunchKernelGGL(face_letterbox_kernel, dim3((kFaceBox * kFaceBox + 255) / 256, B), dim3(256), 0, stream, pix_dev, rec_dev, kFaceBox, out_dev);
  CC_HIP(hipGetLastError());
}

}  // namespace cc

extern "C" int cc_face_align(const uint8_t* pixels, int64_t pixels_bytes, int pixels_on_device, const cc_face_align_rec* records, int n,
                             uint8_t* out_dev, int device, void* stream) {
  using namespace cc;
  CC_API_BEGIN
  CC_CHECK(pixels && records && out_dev && n > 0 && pixels_bytes > 0, "bad argument");
  int nd = 0; CC_HIP(hipGetDeviceCount(&nd));
  CC_CHECK(nd > 0 && device >= 0 && device < nd, "no such HIP device");
  CC_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<AlignRec> rec(n);
  for (int i = 0; i < n; ++i) {
    const cc_face_align_rec& q = records[i];
    const std::string who = "face " + std::to_string(i) + ": ";
    CC_CHECK(q.h > 0 && q.w > 0 && q.offset >= 0 && (size_t)q.offset + (size_t)q.h * q.w * 3 <= (size_t)pixels_bytes, who + "crop lies outside the packed buffer");
    CC_CHECK(q.cw > 0 && q.ch > 0 && q.cx1 >= 0 && q.cy1 >= 0 && (long long)q.cx1 + q.cw <= q.w && (long long)q.cy1 + q.ch <= q.h, who + "cut lies outside the crop");
    CC_CHECK(q.out_w > 0 && q.out_h > 0, who + "empty levelled image");
    AlignRec& r = rec[i];
    r.off = q.offset; r.h = q.h; r.w = q.w; r.cx1 = q.cx1; r.cy1 = q.cy1; r.cw = q.cw; r.ch = q.ch; r.out_w = q.out_w; r.out_h = q.out_h;
    invert_affine(q.rot, r.rot); invert_affine(q.place, r.place);
  }
  AlignRec* drec = nullptr; uint8_t* dpix = nullptr;
  CC_HIP(hipMallocAsync((void**)&drec, sizeof(AlignRec) * n, s));
  CC_HIP(hipMemcpyAsync(drec, rec.data(), sizeof(AlignRec) * n, hipMemcpyHostToDevice, s));
  const uint8_t* src = pixels;
  if (!pixels_on_device) {
    CC_HIP(hipMallocAsync((void**)&dpix, (size_t)pixels_bytes, s));
    CC_HIP(hipMemcpyAsync(dpix, pixels, (size_t)pixels_bytes, hipMemcpyHostToDevice, s));
    src = dpix;
  }
  hipLaunchKernelGGL(face_align_kernel, dim3(kFace * kFace / 256, n), dim3(256), 0, s, src, drec, out_dev);
  CC_HIP(hipGetLastError());
  CC_HIP(hipFreeAsync(drec, s));
  if (dpix) CC_HIP(hipFreeAsync(dpix, s));
  CC_HIP(hipStreamSynchronize(s));          // `rec` and the caller's host buffers may go away on return
  CC_API_END
}
