// Calibration-aware weight rounding for the detector's 1x1 convs (C-ABI dtype 5, "f16c"; round 5).
//
// Plain f16 weights (11 bits) move boxes by up to a pixel on a float32 checkpoint; dtype "f16h" buys the tolerance back with a second
// weight plane in the backbone's 1x1 convs at 8 % of the frame rate.  Here every 1x1 conv keeps ONE f16 plane, but its weights are rounded
// with the rounding errors steered by the second moments of the conv's own input, H = E[x x^T] (the GPTQ recursion: Frantar et al. 2022,
// restated from the paper; columns in input-channel order, error fed forward through the Cholesky factor of H^-1): the error of the
// conv's OUTPUT on inputs that look like the calibration inputs shrinks 10-15x against nearest rounding (tools/dev/gptq_emulation.py,
// profiles/r04w_gptq_emulation.txt; on the real kernels: profiles/r05a_gptq_gpu.txt).
//   * sample_rows_kernel  gathers S pixel rows of a conv's input view (channel slice of an NHWC f32 tensor, two-source Concat, Upsample as
//                         an index shift - the ConvP::s0 / s1 views of the f32 calibration plan) into a dense (S, Cin) f32 matrix;
//   * gptq_round_f16      host, double precision, no LAPACK (K <= 1024): H + damp mean(diag) I = L L^T, H^-1 = L^-T L^-1 = G G^T, then the
//                         column walk.  Bit-compatible with oracle/lowprec_oracle.py::gptq_f16 up to the factorisations' rounding
//                         (tests/test_abi_and_host.py: identical on >= 99.5 % of the weights, same expected output error).
// The reference (detection/yolov9.py:372-373) loads float32 safetensors and computes in float32; which 16-bit values stand in for them is
// this library's business, and the parity bar (tests/test_gpu_yolo.py::test_calibrated_mode_*) is the one "f16h" is held to.
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <thread>
#include <vector>
#include "yolo_plan.h"

using namespace cc;

namespace cc {

// out[j][c] = input channel c (over s0 then s1) of output pixel rows[j] of a 1x1 stride-1 conv over f32 activations
__global__ __launch_bounds__(256) void sample_rows_kernel(const ConvP p, const int* rows, int S, float* out) {
  const int j = blockIdx.x;
  if (j >= S) return;
  const int m = rows[j], hw = p.Ho * p.Wo;
  const int b = m / hw, rem = m - b * hw, ho = rem / p.Wo, wo = rem - ho * p.Wo;
  const float* a0 = reinterpret_cast<const float*>(p.s0.ptr) + (((size_t)b * p.s0.H + (ho >> p.s0.shift)) * p.s0.W + (wo >> p.s0.shift)) * p.s0.cstride + p.s0.coff;
  const float* a1 = p.s1.C ? reinterpret_cast<const float*>(p.s1.ptr) + (((size_t)b * p.s1.H + (ho >> p.s1.shift)) * p.s1.W + (wo >> p.s1.shift)) * p.s1.cstride + p.s1.coff : nullptr;
  for (int c = threadIdx.x; c < p.Cin; c += 256) out[(size_t)j * p.Cin + c] = c < p.s0.C ? a0[c] : a1[c - p.s0.C];
}

void launch_sample_rows(const ConvP& p, const int* rows_dev, int S, float* out_dev, hipStream_t stream) {
  CC_CHECK(p.ks == 1 && p.stride == 1 && p.pad == 0 && p.s0.shift >= 0 && p.s1.shift >= 0, "sample_rows: 1x1 stride-1 convs only");
  hipLaunchKernelGGL(sample_rows_kernel, dim3(S), dim3(256), 0, stream, p, rows_dev, S, out_dev);
  CC_HIP(hipGetLastError());
}

static inline float f16_round(float f) { return (float)(f16_t)f; }   // round to nearest even, overflow to inf, subnormals exact

// lower Cholesky factor of the symmetric positive definite n x n matrix a (row major), in place in the lower triangle; false if not PD
static bool cholesky_lower(std::vector<double>& a, int n) {
  for (int j = 0; j < n; ++j) {
    double d = a[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= a[(size_t)j * n + k] * a[(size_t)j * n + k];
    if (!(d > 0)) return false;
    d = std::sqrt(d); a[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double s = a[(size_t)i * n + j];
      const double *ri = &a[(size_t)i * n], *rj = &a[(size_t)j * n];
      for (int k = 0; k < j; ++k) s -= ri[k] * rj[k];
      a[(size_t)i * n + j] = s / d;
    }
  }
  return true;
}

// H (ci x ci, row major) = X^T X / rows for X (rows x ci) f32, accumulated in double
void second_moments(const float* X, int rows, int ci, std::vector<double>& H) {
  H.assign((size_t)ci * ci, 0.0);
  std::vector<double> xr(ci);
  for (int r = 0; r < rows; ++r) {
    const float* x = X + (size_t)r * ci;
    for (int i = 0; i < ci; ++i) xr[i] = x[i];
    for (int i = 0; i < ci; ++i) {
      const double xi = xr[i];
      if (xi == 0.0) continue;
      double* h = &H[(size_t)i * ci];
      for (int j = i; j < ci; ++j) h[j] += xi * xr[j];
    }
  }
  const double inv = rows > 0 ? 1.0 / rows : 0.0;
  for (int i = 0; i < ci; ++i)
    for (int j = i; j < ci; ++j) { const double v = H[(size_t)i * ci + j] * inv; H[(size_t)i * ci + j] = v; H[(size_t)j * ci + i] = v; }
}

// w (co x ci) f32 -> out: f16-representable f32 values.  0 ok, -1 / -2: H (damped) or its inverse not positive definite - the caller then
// leaves the conv to the library's controlled rounding.
int gptq_round_f16(const float* w, int co, int ci, const double* H, double damp, float* out) {
  const int n = ci;
  std::vector<double> A((size_t)n * n);
  double mean_diag = 0;
  for (int i = 0; i < n; ++i) mean_diag += H[(size_t)i * n + i];
  mean_diag /= n;
  if (!(mean_diag > 0) || !std::isfinite(mean_diag)) return -1;
  for (size_t i = 0; i < (size_t)n * n; ++i) A[i] = H[i];
  for (int i = 0; i < n; ++i) A[(size_t)i * n + i] += damp * mean_diag;
  if (!cholesky_lower(A, n)) return -1;
  std::vector<double> Li((size_t)n * n, 0.0);              // Li = L^-1 (lower): forward substitution, column c of the identity
  for (int c = 0; c < n; ++c)
    for (int i = c; i < n; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) s -= A[(size_t)i * n + k] * Li[(size_t)k * n + c];
      Li[(size_t)i * n + c] = s / A[(size_t)i * n + i];
    }
  std::vector<double>& Hinv = A;                           // H^-1 = Li^T Li (A is done)
  std::fill(Hinv.begin(), Hinv.end(), 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0;
      for (int k = i; k < n; ++k) s += Li[(size_t)k * n + i] * Li[(size_t)k * n + j];
      Hinv[(size_t)i * n + j] = Hinv[(size_t)j * n + i] = s;
    }
  if (!cholesky_lower(Hinv, n)) return -2;                 // H^-1 = G G^T, G lower; U = G^T is the upper factor the walk uses: U[i][j] = G[j][i]
  std::vector<double> W((size_t)co * n);
  for (size_t i = 0; i < (size_t)co * n; ++i) W[i] = w[i];
  for (int i = 0; i < n; ++i) {
    const double uii = Hinv[(size_t)i * n + i];
    for (int o = 0; o < co; ++o) {
      double* row = &W[(size_t)o * n];
      const float q = f16_round((float)row[i]);
      out[(size_t)o * n + i] = q;
      if (!std::isfinite(q)) continue;
      const double err = (row[i] - (double)q) / uii;
      for (int j = i + 1; j < n; ++j) row[j] -= err * Hinv[(size_t)j * n + i];
    }
  }
  return 0;
}

// dtype "f16c": the float32 weights of the 1x1 convs in h->host are replaced by f16-representable values chosen by the GPTQ recursion
// (gptq_round_f16 above) on the second moments of each conv's own input - measured on an f32 twin of the handle running the calibration frames
// launch by launch (the inputs of conv i are in the arena right before launch i) - before the usual finalize packs them.  Convs that share
// an input and were packed together (RepNCSP's cv1 | cv2) share H.  Left to controlled rounding: 3x3 convs, grouped convs, DDetect.
void calibrate_1x1(cc_yolo* h) {
  cc_yolo* t = nullptr;
  if (cc_yolo_create(&t, h->arch->size, h->res, F32, h->device) != 0) throw cc::Error(-5, std::string("calibration twin: ") + cc_last_error());
  struct Guard { cc_yolo* t; ~Guard() { if (t) cc_yolo_destroy(t); } } guard{t};
  t->host = h->host;
  if (cc_yolo_finalize(t) != 0) throw cc::Error(-5, std::string("calibration twin: ") + cc_last_error());
  // calibration frames: the caller's (cc_yolo_calibrate) PLUS two frames of seeded white noise, or four noise frames alone.  The noise
  // frames keep every input direction of every conv excited: with calibration frames from one narrow distribution only (heavily blurred
  // input), H is nearly singular along directions the test inputs do use and the recursion pushes its rounding errors there.
  int B = h->calib_B, H = h->calib_H, W = h->calib_W, f32 = h->calib_f32;
  const int n_noise = h->calib_frames.empty() ? 4 : 2;
  if (h->calib_frames.empty()) { B = 0; H = W = h->res; f32 = 0; }
  const size_t per = (size_t)H * W * 3, es = f32 ? 4 : 1;
  std::vector<unsigned char> all((size_t)(B + n_noise) * per * es);
  if (B) memcpy(all.data(), h->calib_frames.data(), (size_t)B * per * es);
  {
    uint32_t st = 0x9E3779B9u;
    for (size_t i = (size_t)B * per; i < (size_t)(B + n_noise) * per; ++i) {
      st = st * 1664525u + 1013904223u;
      const unsigned char v = (unsigned char)(st >> 24);
      if (f32) reinterpret_cast<float*>(all.data())[i] = (float)v; else all[i] = v;
    }
  }
  B += n_noise;
  const void* frames = all.data();
  CC_HIP(hipSetDevice(h->device));
  Plan* P = get_plan(t, B, H, W, f32);
  hipStream_t s = t->stream;
  CC_HIP(hipMemcpyAsync(P->frames_dev, frames, P->frames_bytes, hipMemcpyHostToDevice, s));
  input_step(t, P, s, P->frames_dev);
  int head_blk = 0;
  for (auto& kv : h->host) if (kv.first.rfind("model.list.", 0) == 0) head_blk = std::max(head_blk, atoi(kv.first.c_str() + 11));
  std::map<const void*, std::string> by_w;
  for (auto& kv : t->packed) by_w[kv.second.w] = kv.first;
  struct Item { std::vector<std::string> names; int ci = 0, rows = 0; std::vector<float> X; int rc = 0; };
  std::vector<Item> items; std::set<std::string> seen;
  constexpr int SMAX = 4096;                              // pixels per conv: the expected output error stops moving well below this (r04w_gptq_emulation.txt)
  int* rows_dev = nullptr; float* x_dev = nullptr; size_t x_cap = 0;
  CC_HIP(hipMalloc((void**)&rows_dev, SMAX * sizeof(int)));
  struct Free { int*& r; float*& x; ~Free() { if (r) hipFree(r); if (x) hipFree(x); } } fr{rows_dev, x_dev};
  for (const Op& op : P->ops) {
    const ConvP& c = op.conv;
    if (op.kind == Conv && c.ks == 1 && c.stride == 1 && c.pad == 0 && c.s0.shift >= 0 && c.s1.shift >= 0) {
      auto it = by_w.find(c.w);
      if (it != by_w.end() && !seen.count(it->second)) {
        seen.insert(it->second);
        Item item; bool ok = true;
        for (size_t a = 0, b; a < it->second.size(); a = b + 1) { b = it->second.find('+', a); item.names.push_back(it->second.substr(a, b - a)); }
        for (auto& n : item.names) {
          auto w = h->host.find(n + ".weight");
          ok = ok && w != h->host.end() && w->second.shape.size() == 4 && w->second.shape[2] == 1 && w->second.shape[1] == c.Cin && atoi(n.c_str() + 11) != head_blk;
        }
        if (ok) {
          const long M = (long)c.B * c.Ho * c.Wo;
          const int S = (int)std::min<long>(M, SMAX);
          const long seg = M / S;                          // one pixel per segment of the flattened (image, row, column) index, position hashed
          std::vector<int> rows(S);
          for (int j = 0; j < S; ++j) rows[j] = (int)(j * seg + (long)(((uint32_t)j * 2654435761u) >> 8) % seg);
          if ((size_t)S * c.Cin > x_cap) { if (x_dev) hipFree(x_dev); x_dev = nullptr; x_cap = (size_t)S * c.Cin; CC_HIP(hipMalloc((void**)&x_dev, x_cap * 4)); }
          CC_HIP(hipMemcpyAsync(rows_dev, rows.data(), S * sizeof(int), hipMemcpyHostToDevice, s));
          launch_sample_rows(c, rows_dev, S, x_dev, s);
          item.ci = c.Cin; item.rows = S; item.X.resize((size_t)S * c.Cin);
          CC_HIP(hipMemcpyAsync(item.X.data(), x_dev, item.X.size() * 4, hipMemcpyDeviceToHost, s));
          CC_HIP(hipStreamSynchronize(s));
          items.push_back(std::move(item));
        }
      }
    }
    launch_op(F32, P, op, s, false);
  }
  CC_HIP(hipStreamSynchronize(s));
  // the recursion: convs are independent - one host thread each, up to 16
  static const double damp = [] { const char* e = getenv("CLEARCAM_CALIB_DAMP"); return e ? atof(e) : 0.03; }();
  // (ridge added to H as a share of its mean diagonal.  Measured on 256 frames x three checkpoints x three kinds of calibration frames,
  //  anchors beyond the 0.64 px tolerance out of ~179 k: 0.01 (the usual GPTQ value) 82 with matched calibration / 355 with mismatched,
  //  0.03 113 / 275, 0.1 130 / 243; "f16h" 101, plain f16 597 - profiles/r05n_tail_256.txt.  The tail is heavy and these are single draws.)
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < items.size();) {
      Item& it = items[i];
      try {
        std::vector<double> Hm;
        second_moments(it.X.data(), it.rows, it.ci, Hm);
        std::vector<float>().swap(it.X);
        for (auto& n : it.names) {
          HostTensor& w = h->host.at(n + ".weight");                  // every key exists (checked above); at() does not modify the map: safe from several threads
          std::vector<float> q(w.data.size());
          const int rc = gptq_round_f16(w.data.data(), (int)w.shape[0], it.ci, Hm.data(), damp, q.data());
          if (rc == 0) w.data.swap(q); else it.rc = rc;
        }
      } catch (...) { it.rc = -3; }                                  // out of memory on a worker: the conv keeps controlled rounding
    }
  };
  const unsigned nt = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)items.size()}));
  std::vector<std::thread> pool;
  for (unsigned i = 1; i < nt; ++i) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
  h->calib_convs = 0; h->calib_fallback = 0;
  for (auto& it : items) { if (it.rc == 0) ++h->calib_convs; else ++h->calib_fallback; }
  if (getenv("CLEARCAM_VERBOSE")) fprintf(stderr, "[clearcam] calibration: %d packed 1x1 convs rounded on %d frames (%d left to controlled rounding)\n", h->calib_convs, B, h->calib_fallback);
}

}  // namespace cc

extern "C" {

int cc_yolo_calibrate(cc_yolo* h, const void* frames, int B, int H, int W, int frame_f32) {
  CC_API_BEGIN
  CC_CHECK(h && frames && B > 0 && H > 0 && W > 0, "bad argument");
  CC_CHECK(h->calibrated, "cc_yolo_calibrate: the handle was not created with dtype 5 (f16c)");
  CC_CHECK(!h->finalized, "cc_yolo_calibrate after cc_yolo_finalize (the float32 weights are gone)");
  const size_t nb = (size_t)B * H * W * 3 * (frame_f32 ? 4 : 1);
  h->calib_frames.assign((const unsigned char*)frames, (const unsigned char*)frames + nb);
  h->calib_B = B; h->calib_H = H; h->calib_W = W; h->calib_f32 = frame_f32 ? 1 : 0;
  CC_API_END
}

int cc_yolo_calibration_info(cc_yolo* h, int* n_calibrated, int* n_fallback) {
  CC_API_BEGIN
  CC_CHECK(h && h->finalized, "no finalized handle");
  if (n_calibrated) *n_calibrated = h->calib_convs;
  if (n_fallback) *n_fallback = h->calib_fallback;
  CC_API_END
}

int cc_gptq_round_f16(const float* w, int64_t cout, int64_t cin, const double* H, double damp, float* out) {
  CC_API_BEGIN
  CC_CHECK(w && H && out && cout > 0 && cin > 0 && cin <= 4096, "bad argument");
  const int rc = cc::gptq_round_f16(w, (int)cout, (int)cin, H, damp, out);
  CC_CHECK(rc == 0, "H (damped) is not positive definite");
  CC_API_END
}

}  // extern "C"
