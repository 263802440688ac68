// Detector runtime: YOLOv9 t/s/m/c graph -> flat kernel list -> hipGraph, behind the C ABI.
//
// Stands behind YOLOv9.__init__/__call__ (detection/yolov9.py:298-388) and jit_infer's
// shape-keyed cache (utils/helpers.py:214-221): one Plan (buffers + launch list + captured
// hipGraph) per (B,H,W,frame dtype), replayed on later calls.
//
// MI355X-first choices (vs. the reference's op-by-op tensor graph):
//   * NHWC activations; every Concat/chunk (yolov9.py:52,78,104,124,148,155) is a channel-offset
//     view: producers write straight into the consumer's concat buffer, or the consumer conv reads
//     two sources.  Upsample (:285-292) is folded into the consumer's loader (index>>1).
//   * RepNCSP's two 1x1 convs over the same input (:101,103) and the head's two 3x3 convs over the
//     same feature map (:205-206) are fused into one GEMM each (weights concatenated along Cout).
//   * RepNBottleneck's residual (:89) is the conv epilogue, written in place.
//   * grouped head convs (:172-181, K=144/16 per group) are densified to block-diagonal weights.
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <thread>
#include <atomic>
#include <string>
#include <vector>
#include <cmath>
#include <cstring>
#include "conv_select.h"
#include "kernels.h"
#include "../../include/clearcam_hip.h"

namespace cc {

struct Arch {
  const char* size; int stem; bool elan1; int b2_hidden, b2_out; bool adown; int d3_out, e4_hidden, p3, b4_out,
      d5_out, e6_hidden, p4, d7_out, e8_hidden, p5, spp_hidden, d16_out, d19_out, cls_hidden, rep_n;
};
// detection/yolov9.py:461-464 (SIZES) by role; same table as clearcam_amd/arch.py.
static const Arch kArch[] = {
    {"t", 16, true, 32, 32, false, 64, 16, 64, 64, 96, 24, 96, 128, 32, 128, 64, 48, 64, 80, 3},
    {"s", 32, true, 64, 64, false, 128, 32, 128, 128, 192, 48, 192, 256, 64, 256, 128, 96, 128, 128, 3},
    {"m", 32, false, 32, 128, false, 240, 60, 240, 240, 360, 90, 360, 480, 120, 480, 240, 184, 240, 240, 1},
    {"c", 64, false, 32, 256, true, 256, 64, 256, 512, 512, 128, 512, 512, 128, 512, 256, 256, 512, 256, 1},
    // "e" (yolov9.py:328-371) has its own 43-block builder; only adown / cls_hidden / rep_n are read from this row
    {"e", 64, false, 32, 256, true, 0, 0, 256, 0, 0, 0, 512, 0, 0, 512, 256, 0, 0, 256, 2},
};

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };
struct PackedConv { void* w = nullptr; float* bias = nullptr; int cin = 0, cout = 0, k = 0, kw = 0; double macs_px = 0; int split = 0; float oscale = 1.0f; };

struct Buf { int H, W, C; bool f32; size_t off; };
struct View { int buf; int coff; int C; };
struct In { View v; int shift; };

struct Op {
  int kind;  // 0 conv, 1 pool, 2 decode, 3 nms, 4 fuse, 5 letterbox + first conv (launched before the graph: it reads the caller's frames), 6 fused RepNCSP,
             // 7 fused DDetect tail (last 1x1 convs of both branches + decode)
  ConvP conv; PoolP pool; DecodeP dec; NmsP nms; FuseP fuse; StemP stem; CspP csp; HeadTailP tail;
  double alg_macs = 0;   // algorithmic multiply-accumulates of this launch (no padding / densification)
  // Concurrency inside the captured graph: launches of one lane run in list order; a launch waits for the launches of OTHER lanes
  // it conflicts with (read-after-write, write-after-read, write-after-write on overlapping channel ranges of a tensor, or on
  // overlapping arena bytes of two tensors).  Lane 0 is the trunk; the list order itself is always a valid serial schedule.
  struct Access { int buf, coff, C; bool write; };     // buf < 0: -2 = the (B, A, 6) decoded rows, -3 = the (B, 300, 6) result
  int lane = 0;
  std::vector<Access> acc;
};

struct Plan {
  int B, H, W, frame_f32;
  int nh, nw, pad_y, pad_x, Hn, Wn, A;
  std::vector<Buf> bufs;
  size_t arena_bytes = 0;
  char* arena = nullptr;
  std::vector<Op> ops;
  std::map<std::string, int> taps;
  int in_buf = -1;
  int *xlo = nullptr, *xhi = nullptr, *ylo = nullptr, *yhi = nullptr; float *xfr = nullptr, *yfr = nullptr;
  void* frames_dev = nullptr; size_t frames_bytes = 0;
  bool fused_stem = false; const void* last_frames = nullptr;   // no materialised network input; frames of the last detect call
  float* det = nullptr; float* out_dev = nullptr;
  int* nonfinite = nullptr;                            // device counter of anchors with non-finite logits (decode / DDetect tail), summed over the plan's life
  hipGraphExec_t exec = nullptr;
  std::vector<hipEvent_t> lane_ev;                     // the cross-lane edges of the captured graph (run_ops_lanes)
  // Ragged plan (cc_yolo_detect_ragged): B frames of ANY source sizes that letterbox to Hn x Wn; H, W, nh, nw = Hn, Wn and the pads are 0
  // (placeholders).  The per-frame records live at the FIXED device address desc_dev - the NMS launch inside the captured graph reads it -
  // and are refreshed from the pinned desc_host on the plan's stream before each replay.  desc_host is a single buffer, not a ring: before
  // it is overwritten the host waits for desc_up, recorded right after the previous upload on this plan (a refinement of waiting for the
  // slot's slot_done: the upload is the first thing a submission does, so the wait ends when the previous batch of the slot STARTS).
  bool ragged = false;
  FrameDesc* desc_dev = nullptr; FrameDesc* desc_host = nullptr; hipEvent_t desc_up = nullptr; bool desc_pending = false;
  size_t packed_bytes = 0; bool stem_big = false;      // of the last call: size of the packed buffer, scratch size of the stem launch
  ~Plan() {
    if (exec) hipGraphExecDestroy(exec);
    if (desc_up) hipEventDestroy(desc_up);
    if (desc_host) hipHostFree(desc_host);
    if (desc_dev) hipFree(desc_dev);
    for (hipEvent_t e : lane_ev) if (e) hipEventDestroy(e);
    for (void* p : {(void*)arena, (void*)xlo, (void*)xhi, (void*)ylo, (void*)yhi, (void*)xfr, (void*)yfr, frames_dev, (void*)det, (void*)out_dev, (void*)nonfinite})
      if (p) hipFree(p);
  }
};

}  // namespace cc

using namespace cc;

struct cc_yolo {
  const Arch* arch = nullptr;
  int res = 640, dtype = BF16, device = 0;              // dtype: STORAGE type of activations and weights
  int wsplit = 0;                                      // C-ABI dtype 3 ("f16s"): f16 storage, every conv weight as two f16 planes (ConvP::split)
  // ... dtype 3 ("f16s"): everywhere.  dtype 4 ("f16h"): every conv up to block split_all_last (the stem conv), the 1x1 convs up to block
  // split_1x1_last (the backbone); everything else carries one plane with controlled rounding
  int split_all_last = 1 << 30, split_1x1_last = 1 << 30;
  // dtype 5 ("f16c"): cc_yolo_finalize first rounds the 1x1 convs' float32 weights to f16 values chosen on calibration frames (calibrate_1x1)
  bool calibrated = false;
  std::vector<unsigned char> calib_frames; int calib_B = 0, calib_H = 0, calib_W = 0, calib_f32 = 0;   // cc_yolo_calibrate; empty: seeded noise
  int calib_convs = 0, calib_fallback = 0;             // packed 1x1 convs rounded by the recursion / left to controlled rounding (H not positive definite)
  hipStream_t stream = nullptr;
  std::vector<hipStream_t> side;                       // streams of lanes 1.. while a plan is captured (run_ops_lanes)
  // Batches in flight (cc_yolo_submit / cc_yolo_wait): slot i > 0 has its own stream and its own plans (arena, graph), so the tail of
  // one batch overlaps the head of the next; slot 0 is `stream` and the plans cc_yolo_detect uses.
  std::vector<hipStream_t> slot_stream;
  std::vector<hipEvent_t> slot_done;
  long long submitted = 0;
  hipStream_t stream_of_slot(int i) const { return i == 0 ? stream : slot_stream[i - 1]; }
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int* nonfinite_host = nullptr;                       // pinned: the plan's counter lands here with the rows of a host-output call
  std::map<std::string, HostTensor> host;
  std::map<std::string, PackedConv> packed;
  float* dfl_w = nullptr;
  bool finalized = false;
  PlanCache<std::vector<int>, Plan> plans;
  Plan* last = nullptr;
  int plans_built = 0;                                 // plans built (arena + graph capture) over the handle's life: cc_yolo_plans_built
  // Axis tables of the ragged entry points, one device allocation (lo | hi | fr) per distinct (n_in, n_out), least recently used dropped
  // beyond kMaxAxisTabs (ragged_prepare): a site has a handful of camera models, so a frame's tables are almost always already there.
  struct AxisTab { int* lo; int* hi; float* fr; unsigned long long used; };
  std::map<std::pair<int, int>, AxisTab> axis_tabs;
  unsigned long long axis_tick = 0;
  int cin_pad() const { return dtype == F32 ? 4 : 8; }
};

namespace cc {

void convert_f32_to(int dt, const float* src, void* dst, size_t n) {
  if (dt == F32) memcpy(dst, src, n * 4);
  else if (dt == F16) { f16_t* d = (f16_t*)dst; for (size_t i = 0; i < n; ++i) d[i] = (f16_t)src[i]; }
  else { uint16_t* d = (uint16_t*)dst; for (size_t i = 0; i < n; ++i) d[i] = f32_to_bf16_bits(src[i]); }
}

// 16-bit storage of a float32 filter bank with CONTROLLED rounding.  Round-to-nearest treats every weight alone; its residuals are
// independent of each other but NOT of the activations they multiply (post-SiLU maps have a positive mean and are smooth across taps
// and, within a layer, similar across channels), and that coherent part - a gain error per filter - is what survives a deep low-pass
// network.  So each weight goes to one of its two neighbours in the storage type (the nearest one unless the sums say otherwise), chosen
// per output channel to keep several sums of the rounding residuals near zero at once: the channel's TOTAL (its DC gain, double weight),
// the sum over the taps of each INPUT CHANNEL's k x k filter, the sum over the input channels at each TAP, and the two first moments
// over the tap coordinates - "controlled rounding" of a (Cin x k*k) table with its margins preserved, every margin within about an ulp of
// the float32 value instead of random-walking away from it.  Same storage, same kernels, same speed.  Measured on the conditioned
// checkpoint with un-rounded weights against the f32 oracle (CPU emulation, 48 frames, 761 detections), strict matches / per-anchor box
// error p99 / max: nearest 92.1 % / 1.26 / 2.6 px; one-dimensional error feedback (`feedback`) 97.7 % / 0.64 / 1.5 px; controlled 99.0 % /
// 0.42 / 0.77 px, scores within 1.9e-3; bf16 (16 frames): 26.9 % / 69.2 % / 75.4 % strict.  Still not inside the 0.64 px bar for every
// anchor - that is what the split-weight mode is for - but the speed modes become far better detectors for nothing.  Values the type holds exactly stay (both
// neighbours coincide).  CLEARCAM_WEIGHT_ROUNDING=nearest | feedback selects the other two.
static int weight_rounding() {                          // 0 nearest, 1 feedback, 2 controlled
  static const int mode = [] {
    const char* e = getenv("CLEARCAM_WEIGHT_ROUNDING");
    return !e ? 2 : (!strcmp(e, "nearest") ? 0 : (!strcmp(e, "feedback") ? 1 : 2));
  }();
  return mode;
}
static inline float round_storage(int dt, float t) { return dt == F16 ? (float)(f16_t)t : bf16_bits_to_f32(f32_to_bf16_bits(t)); }
static inline uint16_t storage_bits(int dt, float r) { return dt == F16 ? __builtin_bit_cast(uint16_t, (f16_t)r) : f32_to_bf16_bits(r); }
static inline float storage_value(int dt, uint16_t b) { return dt == F16 ? (float)__builtin_bit_cast(f16_t, b) : bf16_bits_to_f32(b); }
// the neighbour of the storage-type value `r` towards +inf (up) or -inf: sign-magnitude bit patterns
static inline float storage_next(int dt, float r, bool up) {
  uint16_t b = storage_bits(dt, r);
  const bool neg = b & 0x8000u;
  const uint16_t mag = b & 0x7fffu;
  if (mag == 0) return storage_value(dt, (uint16_t)((up ? 0x0000u : 0x8000u) | 1u));       // +-0 -> smallest subnormal of that sign
  if (neg == up) b = (uint16_t)(b - 1u); else b = (uint16_t)(b + 1u);                          // towards zero / away from zero
  return storage_value(dt, b);
}
static std::vector<float> round_with_feedback(int dt, const HostTensor& w) {
  std::vector<float> q(w.data.size());
  const size_t co = (size_t)w.shape[0], per = co ? w.data.size() / co : 0;
  for (size_t n = 0; n < co; ++n) {
    float e = 0.f;
    for (size_t k = 0; k < per; ++k) {
      const float t = w.data[n * per + k] + e;
      const float r = round_storage(dt, t);
      q[n * per + k] = r;
      e = std::isfinite(r) ? t - r : 0.f;              // exact: r is t rounded to fewer bits
    }
  }
  return q;
}
// w: (cout, cin, k*k) float32, row-major (OIHW with the k x k taps flattened).  Per output channel the residuals d = q - w are steered by
//   cost = (row sum)^2 + (tap sum)^2 + 2 (total)^2 + (first moments over the tap coordinates)^2   [row = one input channel's k x k filter]
// in two passes: a sequential greedy pass with running sums, then one refinement pass that re-decides every weight with all others fixed.
// The moments keep the filter's response to a linear ramp (smooth activations) as well as to a constant.  float32 arithmetic in a fixed
// order: oracle/lowprec_oracle.py::q_feedback reproduces it bit for bit (tests/test_abi_and_host.py).
static std::vector<float> round_controlled(int dt, const float* w, size_t co, size_t ci, size_t k) {
  const size_t taps = k * k;
  std::vector<float> q(co * ci * taps), d(ci * taps), lo(ci * taps), hi(ci * taps), e_row(ci), e_col(taps), rr(taps), ss(taps);
  for (size_t t = 0; t < taps; ++t) { rr[t] = (float)(t / k) - (float)(k - 1) / 2.0f; ss[t] = (float)(t % k) - (float)(k - 1) / 2.0f; }
  const bool mom = taps > 1;
  auto sq = [](float x) { return x * x; };
  for (size_t n = 0; n < co; ++n) {
    float e_tot = 0.f, m_r = 0.f, m_s = 0.f;
    std::fill(e_col.begin(), e_col.end(), 0.f);
    auto cost = [&](float er, float ec, float dd, size_t t) {
      float v = sq(er + dd) + sq(ec + dd) + 2.0f * sq(e_tot + dd);
      if (mom) v = v + (sq(m_r + dd * rr[t]) + sq(m_s + dd * ss[t]));
      return v;
    };
    for (size_t c = 0; c < ci; ++c) {                    // pass 1: sequential, running sums
      float er = 0.f;
      for (size_t t = 0; t < taps; ++t) {
        const size_t j = c * taps + t, i = n * ci * taps + j;
        const float v = w[i], r = round_storage(dt, v);
        float l = r, h = r;                              // the storage-type neighbours of v: l <= v <= h (equal when v is representable)
        if (std::isfinite(r) && std::isfinite(v)) { if (r < v) h = storage_next(dt, r, true); else if (r > v) l = storage_next(dt, r, false); }
        lo[j] = l; hi[j] = h;
        const float dl = l - v, dh = h - v;
        const bool up = cost(er, e_col[t], dh, t) < cost(er, e_col[t], dl, t);
        const float dd = up ? dh : dl;
        q[i] = up ? h : l; d[j] = dd;
        er = er + dd; e_col[t] = e_col[t] + dd; e_tot = e_tot + dd;
        if (mom) { m_r = m_r + dd * rr[t]; m_s = m_s + dd * ss[t]; }
      }
      e_row[c] = er;
    }
    for (size_t c = 0; c < ci; ++c)                      // pass 2: every weight again, all others fixed
      for (size_t t = 0; t < taps; ++t) {
        const size_t j = c * taps + t, i = n * ci * taps + j;
        const float v = w[i], dcur = d[j];
        const float dl = (lo[j] - v) - dcur, dh = (hi[j] - v) - dcur;          // change of the residual if this weight goes down / up
        const bool up = cost(e_row[c], e_col[t], dh, t) < cost(e_row[c], e_col[t], dl, t);
        const float de = up ? dh : dl;
        q[i] = up ? hi[j] : lo[j]; d[j] = dcur + de;
        e_row[c] = e_row[c] + de; e_col[t] = e_col[t] + de; e_tot = e_tot + de;
        if (mom) { m_r = m_r + de * rr[t]; m_s = m_s + de * ss[t]; }
      }
  }
  return q;
}
static std::vector<float> round_weights(int dt, const HostTensor& w) {
  if (weight_rounding() == 1) return round_with_feedback(dt, w);
  const size_t co = (size_t)w.shape[0], ci = w.shape.size() > 1 ? (size_t)w.shape[1] : 1, k = w.shape.size() > 2 ? (size_t)w.shape[2] : 1;
  return round_controlled(dt, w.data.data(), co, ci, k);
}

// Pack a list of OIHW convs over the same input into one [sum Cout][k*k*cin_pad] matrix (+ bias).
// groups>1 convs become block-diagonal.  cin_pad >= cin zero-pads the channel axis (stem).
// split (f16 storage only): every tap's cin_pad channels appear twice, [hi | lo] with  w * 2^e = hi + lo  (hi = f16(w 2^e), lo =
// f16(w 2^e - hi)); 2^e is the power of two that puts the matrix's largest magnitude in [2^14, 2^15), so that lo (~2^-11 of hi)
// stays a NORMAL f16 number for every weight down to ~4e-6 of the largest - the planes hold ~22 significant bits of w, and
// PackedConv::oscale = 2^-e (exact) is applied to the f32 accumulator in the conv epilogue.
static PackedConv pack_convs(int dt, const std::vector<const HostTensor*>& ws, const std::vector<const HostTensor*>& bs,
                             const std::vector<int>& groups, int cin_pad, int split = 0) {
  PackedConv pc;
  CC_CHECK(!split || dt == F16, "split weights need f16 storage");
  const int k = (int)ws[0]->shape[2];
  int cin = 0, cout = 0;
  for (size_t t = 0; t < ws.size(); ++t) {
    CC_CHECK(ws[t]->shape.size() == 4 && ws[t]->shape[2] == k && ws[t]->shape[3] == k, "conv weight must be OIHW");
    const int ci = (int)ws[t]->shape[1] * groups[t];
    CC_CHECK(cin == 0 || cin == ci, "fused convs must share Cin");
    cin = ci; cout += (int)ws[t]->shape[0];
  }
  const int cp = cin_pad > cin ? cin_pad : cin;
  const int planes = split ? 2 : 1;
  const size_t kreal = (size_t)k * k * cp * planes;
  const size_t ktot = (kreal + 63) / 64 * 64;          // row stride: zero padded to a whole number of K steps
  std::vector<float> w((size_t)cout * ktot, 0.f), bias(cout, 0.f);
  float scale = 1.0f;
  if (split) {
    float mx = 0.f;
    for (size_t t = 0; t < ws.size(); ++t) for (float v : ws[t]->data) mx = std::max(mx, std::fabs(v));
    if (mx > 0.f && std::isfinite(mx)) scale = std::ldexp(1.0f, 14 - std::ilogb(mx));      // mx * scale in [2^14, 2^15)
    pc.split = 1; pc.oscale = 1.0f / scale;
  }
  int n0 = 0;
  for (size_t t = 0; t < ws.size(); ++t) {
    const int co = (int)ws[t]->shape[0], cig = (int)ws[t]->shape[1], g = groups[t], cog = co / g;
    pc.macs_px += (double)co * cig * k * k;
    std::vector<float> fb;                               // plain 16-bit storage: the values after controlled rounding (above)
    if (!split && dt != F32 && weight_rounding() != 0) fb = round_weights(dt, *ws[t]);
    const float* src = fb.empty() ? ws[t]->data.data() : fb.data();
    for (int n = 0; n < co; ++n) {
      const int grp = n / cog;
      for (int c = 0; c < cig; ++c)
        for (int r = 0; r < k; ++r)
          for (int s = 0; s < k; ++s) {
            const float v = src[(((size_t)n * cig + c) * k + r) * k + s];
            float* row = &w[(size_t)(n0 + n) * ktot];
            if (!split) row[(size_t)(r * k + s) * cp + grp * cig + c] = v;
            else {
              const float vs = v * scale;                        // exact: a power of two
              const float hi = (float)(f16_t)vs;
              row[(size_t)((r * k + s) * 2 + 0) * cp + grp * cig + c] = hi;
              row[(size_t)((r * k + s) * 2 + 1) * cp + grp * cig + c] = vs - hi;   // exact in f32; rounded to f16 below
            }
          }
      if (bs[t]) bias[n0 + n] = bs[t]->data[n];
    }
    n0 += co;
  }
  std::vector<char> tmp(w.size() * dtype_size(dt));
  convert_f32_to(dt, w.data(), tmp.data(), w.size());
  CC_HIP(hipMalloc(&pc.w, tmp.size() + 256));
  CC_HIP(hipMemcpy(pc.w, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
  CC_HIP(hipMalloc((void**)&pc.bias, cout * 4));
  CC_HIP(hipMemcpy(pc.bias, bias.data(), cout * 4, hipMemcpyHostToDevice));
  pc.cin = cp; pc.cout = cout; pc.k = k; pc.kw = (int)ktot;
  return pc;
}

struct Builder {
  cc_yolo* Y; Plan* P; const Arch& a;
  Builder(cc_yolo* y, Plan* p) : Y(y), P(p), a(*y->arch) {}

  int cur_lane = 0;
  // Which independent chains leave the trunk (CLEARCAM_LANES, read per plan): bit 1 = each DDetect level on its own lane (2-4), bit 2 =
  // the three levels share lane 2, bit 0 = ADown's pooled half on lane 1.  OFF by default.  Measured with nothing else on the GPU:
  // DDetect lanes B = 64: 11.39 -> 11.24 ms, B = 16: 3.75 -> 3.67 (P3's 3x3 convs fill the CUs the neck's 40x40 / 20x20 launches
  // leave idle); a graph with branches costs ~50 us per replay (B = 8: 2.35 -> 2.39 ms, one frame 1.30 -> 1.35); ADown's halves gain
  // nothing (both open with a bandwidth-bound pool); profiles/r03o_lanes_ab*.txt.  But the runtime replays the branches on
  // internal streams that share its few hardware queues with every other stream of the process, and inside a camera pipeline
  // (upload, download and caller streams) a branch that lands behind another stream's barrier costs far more than the lanes gain
  // (64 x 1080p cameras, frames resident: 6.1 k frames/s with lanes against 8.5-9 k without, profiles/r03s_*).  Batches in flight
  // (cc_yolo_submit, slots on probed queues) are the robust way to fill those CUs.  Outputs are bit-identical either way.
  int lanes_mask() const {
    const char* e = getenv("CLEARCAM_LANES");
    return e ? atoi(e) : 0;
  }
  struct Lane {                                            // scope guard: launches pushed inside run on lane `l`
    Builder& b; int saved;
    Lane(Builder& b_, int l) : b(b_), saved(b_.cur_lane) {
      const int m = b.lanes_mask();
      if (l == 1 ? (m & 1) : (m & 6)) b.cur_lane = (l > 2 && (m & 4)) ? 2 : l;    // bit 2: all DDetect levels share lane 2
    }
    ~Lane() { b.cur_lane = saved; }
  };
  static Op::Access rd(View v) { return Op::Access{v.buf, v.coff, v.C, false}; }
  static Op::Access wr(View v) { return Op::Access{v.buf, v.coff, v.C, true}; }
  void push(Op& op, std::vector<Op::Access> acc) { op.lane = cur_lane; op.acc = std::move(acc); P->ops.push_back(op); }

  int new_buf(int H, int W, int C, bool f32 = false) {
    Buf b{H, W, C, f32, P->arena_bytes};
    size_t bytes = (size_t)P->B * H * W * C * (f32 ? 4 : dtype_size(Y->dtype));
    P->arena_bytes += (bytes + 255) & ~(size_t)255;
    P->bufs.push_back(b);
    return (int)P->bufs.size() - 1;
  }
  View whole(int buf) { return View{buf, 0, P->bufs[buf].C}; }
  static View slice(View v, int c0, int C) { return View{v.buf, v.coff + c0, C}; }

  static int block_of(const std::string& name) {                    // "model.list.<block>. ..."
    const size_t at = name.find("model.list.");
    CC_CHECK(at == 0 && isdigit((unsigned char)name[11]), "conv parameter outside model.list.<block>: " + name);
    return atoi(name.c_str() + 11);
  }
  const PackedConv& pconv(const std::vector<std::string>& names, const std::vector<int>& groups, int cin_pad = 0) {
    std::string key;
    for (auto& n : names) key += n + "+";
    auto it = Y->packed.find(key);
    if (it != Y->packed.end()) return it->second;
    std::vector<const HostTensor*> ws, bs;
    for (auto& n : names) {
      auto w = Y->host.find(n + ".weight");
      CC_CHECK(w != Y->host.end(), "missing parameter " + n + ".weight");
      auto b = Y->host.find(n + ".bias");
      CC_CHECK(b != Y->host.end(), "missing parameter " + n + ".bias");
      ws.push_back(&w->second); bs.push_back(&b->second);
    }
    const int blk = block_of(names[0]);
    const bool k1 = ws[0]->shape.size() == 4 && ws[0]->shape[2] == 1;
    const bool split = Y->wsplit && (blk <= Y->split_all_last || (k1 && blk <= Y->split_1x1_last));
    return Y->packed[key] = pack_convs(Y->dtype, ws, bs, groups, cin_pad, split);
  }

  Src src(const In& in) {
    const Buf& b = P->bufs[in.v.buf];
    return Src{nullptr, b.H, b.W, b.C, in.v.coff, in.v.C, in.shift};   // ptr patched after arena alloc
  }

  // conv op; pointers hold buffer ids until resolve()
  void conv(const std::vector<In>& ins, const PackedConv& pc, View out, int stride, int act, const View* res = nullptr) {
    Op op{}; op.kind = 0; ConvP& c = op.conv;
    c.s0 = src(ins[0]); c.s0.ptr = (const void*)(intptr_t)ins[0].v.buf;
    if (ins.size() > 1) { c.s1 = src(ins[1]); c.s1.ptr = (const void*)(intptr_t)ins[1].v.buf; }
    else { c.s1 = Src{nullptr, 1, 1, 0, 0, 0, 0}; c.s1.ptr = (const void*)(intptr_t)-1; }
    const Buf& b0 = P->bufs[ins[0].v.buf];
    c.B = P->B;
    if (ins[0].shift < 0) { c.Hin = b0.H - 1; c.Win = b0.W - 1; }          // the 2x2 stride-1 average of the source (conv_adown.hip)
    else { c.Hin = b0.H << ins[0].shift; c.Win = b0.W << ins[0].shift; }
    c.Cin = c.s0.C + c.s1.C;
    CC_CHECK(c.Cin == pc.cin, "conv input channels do not match weights");
    if (ins.size() > 1) {
      const Buf& b1 = P->bufs[ins[1].v.buf];
      CC_CHECK((b1.H << ins[1].shift) == c.Hin && (b1.W << ins[1].shift) == c.Win, "concat sources differ in size");
    }
    c.ks = pc.k; c.stride = stride; c.pad = pc.k / 2;
    c.Ho = (c.Hin + 2 * c.pad - c.ks) / stride + 1; c.Wo = (c.Win + 2 * c.pad - c.ks) / stride + 1;
    const Buf& ob = P->bufs[out.buf];
    CC_CHECK(ob.H == c.Ho && ob.W == c.Wo && out.C == pc.cout, "conv output view mismatch");
    c.Cout = pc.cout; c.Ktot = c.ks * c.ks * c.Cin * (pc.split ? 2 : 1); c.Kw = pc.kw;
    c.split = pc.split; c.oscale = pc.oscale;
    c.w = pc.w; c.bias = pc.bias;
    c.out = (void*)(intptr_t)out.buf; c.out_cstride = ob.C; c.out_coff = out.coff; c.out_f32 = ob.f32;
    if (res) { const Buf& rb = P->bufs[res->buf]; c.res = (const void*)(intptr_t)res->buf; c.res_cstride = rb.C; c.res_coff = res->coff; c.res_f32 = rb.f32; }
    else { c.res = (const void*)(intptr_t)-1; }
    c.act = act;
    op.alg_macs = (double)c.B * c.Ho * c.Wo * pc.macs_px;
    std::vector<Op::Access> acc{wr(out)};
    for (const In& in : ins) acc.push_back(rd(in.v));
    if (res) acc.push_back(rd(*res));
    push(op, std::move(acc));
  }

  // The detector's first conv straight from the frames (stem_fused_kernel); 16-bit storage only, CLEARCAM_FUSE_STEM=0 disables.
  bool fuse_stem(int cout) const {
    static const bool on = [] { const char* e = getenv("CLEARCAM_FUSE_STEM"); return e ? atoi(e) != 0 : true; }();
    return on && Y->cin_pad() == 8 && stem_fused_supported(Y->dtype, cout);
  }
  // the fused kernel's weight layout ([Cout][32], k = r*9 + s*3 + c), derived once per handle from the packed conv weights; split
  // weights: one such matrix per plane (plane 1 = the low plane)
  const void* stem_weights(const std::string& name, const PackedConv& pc, int plane = 0) {
    const std::string key = name + (plane ? "#stem_lo" : "#stem");
    auto it = Y->packed.find(key);
    if (it != Y->packed.end()) return it->second.w;
    PackedConv f; f.cout = pc.cout;
    CC_HIP(hipMalloc(&f.w, (size_t)pc.cout * 32 * dtype_size(Y->dtype) + 256));
    stem_pack_weights(Y->dtype, pc.w, pc.kw, pc.split ? 16 : 8, plane ? 8 : 0, pc.cout, f.w, Y->stream);
    CC_HIP(hipStreamSynchronize(Y->stream));
    return (Y->packed[key] = f).w;
  }
  void stem_fused(const std::string& name, const PackedConv& pc, View out) {
    Op op{}; op.kind = 5; StemP& q = op.stem;
    const Buf& ob = P->bufs[out.buf];
    CC_CHECK(pc.k == 3 && pc.cin == 8 && ob.H == P->Hn / 2 && ob.W == P->Wn / 2 && out.C == pc.cout, "fused stem: shape mismatch");
    PreP& pp = q.pre;
    pp.frame_f32 = P->frame_f32; pp.B = P->B; pp.H = P->H; pp.W = P->W;
    pp.nh = P->nh; pp.nw = P->nw; pp.pad_y = P->pad_y; pp.pad_x = P->pad_x; pp.Hn = P->Hn; pp.Wn = P->Wn;
    pp.xlo = P->xlo; pp.xhi = P->xhi; pp.xfr = P->xfr; pp.ylo = P->ylo; pp.yhi = P->yhi; pp.yfr = P->yfr;
    pp.flip = 1; pp.div = 255.0f; pp.sub = 0.0f; pp.pad_val = 0.0f;            // as cc_yolo_detect's preprocess launch
    q.w = stem_weights(name, pc); q.bias = pc.bias; q.Cout = pc.cout;
    q.w_lo = pc.split ? stem_weights(name, pc, 1) : nullptr; q.oscale = pc.oscale;
    q.out = (void*)(intptr_t)out.buf; q.out_cstride = ob.C; q.out_coff = out.coff; q.Ho = ob.H; q.Wo = ob.W;
    op.alg_macs = (double)P->B * ob.H * ob.W * pc.macs_px;
    push(op, {wr(out)});
    P->fused_stem = true;
  }

  void pool(View in, View out, int k, int stride, int pad, int mode) {
    Op op{}; op.kind = 1; PoolP& q = op.pool;
    const Buf& ib = P->bufs[in.buf]; const Buf& ob = P->bufs[out.buf];
    q.in = (const void*)(intptr_t)in.buf; q.in_cstride = ib.C; q.in_coff = in.coff;
    q.out = (void*)(intptr_t)out.buf; q.out_cstride = ob.C; q.out_coff = out.coff;
    q.B = P->B; q.H = ib.H; q.W = ib.W; q.C = in.C; q.Ho = ob.H; q.Wo = ob.W; q.k = k; q.stride = stride; q.pad = pad; q.mode = mode;
    const int ph = mode == 2 ? ib.H - 1 : ib.H, pw = mode == 2 ? ib.W - 1 : ib.W;     // mode 2 pools the avg-pooled (H-1, W-1) map
    CC_CHECK(in.C == out.C && ob.H == (ph + 2 * pad - k) / stride + 1 && ob.W == (pw + 2 * pad - k) / stride + 1, "pool view mismatch");
    push(op, {rd(in), wr(out)});
  }

  // ---- blocks (detection/yolov9.py:40-149) ---------------------------------------------------
  int dimH(const In& in) { return P->bufs[in.v.buf].H << in.shift; }
  int dimW(const In& in) { return P->bufs[in.v.buf].W << in.shift; }

  // The four launches of a RepNCSP with one bottleneck as one kernel (csp_fused.hip); 16-bit storage.  Default (level 2): hidden
  // widths 32 (weights resident in LDS: 0.296 ms against 0.394 for the four launches at 160x160) and 64 (weights streamed
  // through a two-slot ring: 0.225 against 0.239 at 80x80); CLEARCAM_FUSE_CSP=1 fuses hidden 32 only, =0
  // keeps the layer-at-a-time path everywhere.  Read per plan, so a test can build both in one process.
  // Development-only switches are honoured only under CLEARCAM_DEV=1.
  static const char* dev_env(const char* name) {
    static const bool dev = [] { const char* e = getenv("CLEARCAM_DEV"); return e && atoi(e) != 0; }();
    return dev ? getenv(name) : nullptr;
  }
  // Round 6: at hidden width 64 the layer-at-a-time path has caught up wherever conv_tile64.hip takes the block's two 3x3 64 -> 64 convs (one round of its
  // 8 x 32 tiles: B >= 11 at 80x80, unsplit 3x3 weights) - whole step, B = 64, f16h, twice each: 6582 / 6582 frames/s against 6531 / 6452 fused
  // (profiles/r06x_fuse_csp.txt).  Level 2 (default) therefore fuses hidden 64 only below that; 3 = always (the round-2..5 behaviour).  Both forms
  // produce the same bits (test_fused_csp_equals_unfused), so the choice may depend on the batch.
  bool fuse_csp(View in, int hid, int index, const std::string& r) {
    const char* e = getenv("CLEARCAM_FUSE_CSP");
    const int level = e ? atoi(e) : 2;
    if (level == 0 || (level == 1 && hid != 32)) return false;
    if (level == 2 && hid == 64 && !pconv({r + ".m.list.0.cv1.conv"}, {1}).split) {
      const Buf& ib = P->bufs[in.buf];
      if (conv_tile64_takes(P->B, ib.H, ib.W)) return false;
    }
    const char* only = dev_env("CLEARCAM_CSP_ONLY");                // development: fuse just this block (csp_debug.py)
    if (only && atoi(only) != index) return false;
    if (!(a.rep_n == 1 && csp_fused_supported(Y->dtype, hid, Y->wsplit) && in.C == 2 * hid && in.coff % 8 == 0 && P->bufs[in.buf].C % 8 == 0)) return false;
    // the fused kernel knows three split patterns: none, all four convs ("f16s"), the two 1x1 launches only ("f16h" in the backbone)
    const int s12 = pconv({r + ".cv1.conv", r + ".cv2.conv"}, {1, 1}).split, s3 = pconv({r + ".cv3.conv"}, {1}).split;
    const int sr = pconv({r + ".m.list.0.cv1.conv"}, {1}).split, sb = pconv({r + ".m.list.0.cv2.conv"}, {1}).split;
    return s12 == s3 && sr == sb && (sr == s12 || (s12 && !sr));
  }
  void csp_fused(const std::string& r, View in, View out, int hid) {
    Op op{}; op.kind = 6; CspP& q = op.csp;
    const Buf& ib = P->bufs[in.buf]; const Buf& ob = P->bufs[out.buf];
    CC_CHECK(ib.H == ob.H && ib.W == ob.W && out.C == 2 * hid, "fused RepNCSP: view mismatch");
    const std::string m = r + ".m.list.0";
    const PackedConv &c12 = pconv({r + ".cv1.conv", r + ".cv2.conv"}, {1, 1}), &cr = pconv({m + ".cv1.conv"}, {1}), &cb = pconv({m + ".cv2.conv"}, {1}),
                     &c3 = pconv({r + ".cv3.conv"}, {1});
    CC_CHECK(c12.cin == 2 * hid && c12.cout == 2 * hid && cr.cin == hid && cr.cout == hid && cr.k == 3 && cb.cin == hid && cb.cout == hid && cb.k == 3 &&
             c3.cin == 2 * hid && c3.cout == 2 * hid, "fused RepNCSP: unexpected conv shapes");
    q.x = (const void*)(intptr_t)in.buf; q.x_cstride = ib.C; q.x_coff = in.coff;
    q.out = (void*)(intptr_t)out.buf; q.out_cstride = ob.C; q.out_coff = out.coff;
    q.w12 = c12.w; q.kw12 = c12.kw; q.b12 = c12.bias; q.wr = cr.w; q.kwr = cr.kw; q.br = cr.bias;
    q.wb = cb.w; q.kwb = cb.kw; q.bb = cb.bias; q.w3 = c3.w; q.kw3 = c3.kw; q.b3 = c3.bias;
    q.B = P->B; q.H = ib.H; q.W = ib.W; q.hid = hid;
    q.split = !c12.split ? 0 : (cr.split ? 1 : 2); q.os12 = c12.oscale; q.osr = cr.oscale; q.osb = cb.oscale; q.os3 = c3.oscale;
    { const char* e = dev_env("CLEARCAM_CSP_DBG"); q.dbg = e ? atoi(e) : 0; }       // stops the kernel after stage 1-3: WRONG outputs
    { const char* e = dev_env("CLEARCAM_CSP_STREAM"); q.stream = e ? atoi(e) : 0; }
    op.alg_macs = (double)P->B * ib.H * ib.W * (c12.macs_px + cr.macs_px + cb.macs_px + c3.macs_px);
    push(op, {rd(in), wr(out)});
  }

  // RepNCSP (:92-105) + trailing 3x3 Conv (:112,115): in -> out
  int n_csp = 0;
  void csp_branch(const std::string& p, View in, View out, int hid) {
    const int H = P->bufs[in.buf].H, W = P->bufs[in.buf].W;
    const std::string r = p + ".list.0";
    const bool tap = getenv("CLEARCAM_TAP_CSP") != nullptr;          // tests: keep the block's tensors readable (costs arena)
    const std::string tn = "csp" + std::to_string(n_csp);
    if (fuse_csp(in, hid, n_csp++, r)) {
      const int u = new_buf(H, W, 2 * hid);
      if (tap) P->taps[tn + "_u"] = u;
      csp_fused(r, in, whole(u), hid);
      conv({{whole(u), 0}}, pconv({p + ".list.1.conv"}, {1}), out, 1, 1);
      return;
    }
    const int csp = new_buf(H, W, 2 * hid), t = new_buf(H, W, hid), u = new_buf(H, W, 2 * hid);
    if (tap) { P->taps[tn + "_ab"] = csp; P->taps[tn + "_t"] = t; P->taps[tn + "_u"] = u; }
    conv({{in, 0}}, pconv({r + ".cv1.conv", r + ".cv2.conv"}, {1, 1}), whole(csp), 1, 1);
    const View x1 = slice(whole(csp), 0, hid);
    for (int j = 0; j < a.rep_n; ++j) {
      const std::string q = r + ".m.list." + std::to_string(j);
      conv({{x1, 0}}, pconv({q + ".cv1.conv"}, {1}), whole(t), 1, 1);
      conv({{whole(t), 0}}, pconv({q + ".cv2.conv"}, {1}), x1, 1, 1, &x1);   // x + cv2(cv1(x)), in place
    }
    conv({{whole(csp), 0}}, pconv({r + ".cv3.conv"}, {1}), whole(u), 1, 1);
    conv({{whole(u), 0}}, pconv({p + ".list.1.conv"}, {1}), out, 1, 1);
  }

  View elan4(const std::string& p, const std::vector<In>& ins, int hid, int cout) {   // RepNCSPELAN4 :107-125
    const int H = dimH(ins[0]), W = dimW(ins[0]);
    const int cat = new_buf(H, W, 8 * hid), o = new_buf(H, W, cout);
    if (getenv("CLEARCAM_TAP_CSP")) P->taps["cat" + std::to_string(n_csp / 2)] = cat;     // tests: [y0 | y1 | y2 | y3] of the n-th RepNCSPELAN4
    conv(ins, pconv({p + ".cv1.conv"}, {1}), slice(whole(cat), 0, 4 * hid), 1, 1);
    csp_branch(p + ".cv2", slice(whole(cat), 2 * hid, 2 * hid), slice(whole(cat), 4 * hid, 2 * hid), hid);
    csp_branch(p + ".cv3", slice(whole(cat), 4 * hid, 2 * hid), slice(whole(cat), 6 * hid, 2 * hid), hid);
    conv({{whole(cat), 0}}, pconv({p + ".cv4.conv"}, {1}), whole(o), 1, 1);
    return whole(o);
  }

  View elan1(const std::string& p, View in, int hid, int cout) {   // ELAN1 :65-80
    const int H = P->bufs[in.buf].H, W = P->bufs[in.buf].W;
    const int cat = new_buf(H, W, 2 * hid), o = new_buf(H, W, cout);
    conv({{in, 0}}, pconv({p + ".cv1.conv"}, {1}), slice(whole(cat), 0, hid), 1, 1);
    conv({{slice(whole(cat), hid / 2, hid / 2), 0}}, pconv({p + ".cv2.conv"}, {1}), slice(whole(cat), hid, hid / 2), 1, 1);
    conv({{slice(whole(cat), hid, hid / 2), 0}}, pconv({p + ".cv3.conv"}, {1}), slice(whole(cat), hid + hid / 2, hid / 2), 1, 1);
    conv({{whole(cat), 0}}, pconv({p + ".cv4.conv"}, {1}), whole(o), 1, 1);
    return whole(o);
  }

  // ADown's avg_pool2d(2,1,0) inside the stride-2 conv that reads it (conv_adown.hip; same values, same K order: identical results).
  // OFF by default - measured slower than the two launches at every shape of the bench plan (0.497 vs 0.182 + 0.199 ms for the
  // 128-channel half at 160x160, batch 64: the loader pulls every source chunk through L2 nine times instead of 2.25);
  // CLEARCAM_FUSE_ADOWN=1 turns it on wherever the shape allows.  Read per plan.
  bool fuse_adown(View in) const {
    const char* e = getenv("CLEARCAM_FUSE_ADOWN");
    if (!e || atoi(e) == 0 || Y->wsplit) return false;
    return Y->dtype != F32 && in.C % 64 == 0 && in.coff % 8 == 0 && P->bufs[in.buf].C % 8 == 0;
  }
  View down(const std::string& p, View in, int cout) {   // ADown :40-52 / AConv :54-63
    const int H = P->bufs[in.buf].H, W = P->bufs[in.buf].W, C = in.C;
    const int Ho = (H - 1 + 2 - 3) / 2 + 1, Wo = (W - 1 + 2 - 3) / 2 + 1;
    const int o = new_buf(Ho, Wo, cout);
    if (a.adown) {
      CC_CHECK(C == cout, "ADown keeps the channel count");
      // x.avg_pool2d(2,1,0).chunk(2,1): only the half the strided conv reads is materialised at full resolution;
      // the other half goes avg -> max-pool in one pass (avgmax_pool_kernel).  The two halves are independent chains (a bandwidth-
      // bound pool + thin 1x1 beside a pool + 3x3): the pooled half is listed first and runs on lane 1 beside the trunk.
      {
        Lane lane(*this, 1);
        const int mp = new_buf(Ho, Wo, C / 2);
        const int E = Y->dtype == F32 ? 4 : 8;
        if ((C / 2) % E == 0 && in.coff % E == 0 && P->bufs[in.buf].C % E == 0) {
          pool(slice(in, C / 2, C / 2), whole(mp), 3, 2, 1, 2);
        } else {                                               // channel counts off the 16-byte grid (yolov9-m): two passes
          const int avg2 = new_buf(H - 1, W - 1, C / 2);
          pool(slice(in, C / 2, C / 2), whole(avg2), 2, 1, 0, 0);
          pool(whole(avg2), whole(mp), 3, 2, 1, 1);
        }
        conv({{whole(mp), 0}}, pconv({p + ".cv2.conv"}, {1}), slice(whole(o), C / 2, C / 2), 1, 1);
      }
      if (fuse_adown(slice(in, 0, C / 2))) {
        conv({{slice(in, 0, C / 2), -1}}, pconv({p + ".cv1.conv"}, {1}), slice(whole(o), 0, C / 2), 2, 1);   // average in the conv's loader
      } else {
        const int avg = new_buf(H - 1, W - 1, C / 2);
        pool(slice(in, 0, C / 2), whole(avg), 2, 1, 0, 0);
        conv({{whole(avg), 0}}, pconv({p + ".cv1.conv"}, {1}), slice(whole(o), 0, C / 2), 2, 1);
      }
    } else {
      const int avg = new_buf(H - 1, W - 1, C);
      pool(in, whole(avg), 2, 1, 0, 0);
      conv({{whole(avg), 0}}, pconv({p + ".cv1.conv"}, {1}), whole(o), 2, 1);
    }
    return whole(o);
  }

  View sppelan(const std::string& p, View in, int hid, int cout) {   // SPPELAN :127-149
    const int H = P->bufs[in.buf].H, W = P->bufs[in.buf].W;
    const int cat = new_buf(H, W, 4 * hid), o = new_buf(H, W, cout);
    conv({{in, 0}}, pconv({p + ".cv1.conv"}, {1}), slice(whole(cat), 0, hid), 1, 1);
    for (int i = 0; i < 3; ++i) pool(slice(whole(cat), i * hid, hid), slice(whole(cat), (i + 1) * hid, hid), 5, 1, 2, 1);
    conv({{whole(cat), 0}}, pconv({p + ".cv5.conv"}, {1}), whole(o), 1, 1);
    return whole(o);
  }

  // CBLinear (:222-228): bare 1x1 conv; the split is a set of channel-offset views of its output
  View cblinear(const std::string& p, View in) {
    const PackedConv& pc = pconv({p + ".conv"}, {1});
    const int o = new_buf(P->bufs[in.buf].H, P->bufs[in.buf].W, pc.cout);
    conv({{in, 0}}, pc, whole(o), 1, 0);
    return whole(o);
  }
  // CBFuse (:230-245): parts are nearest-upsampled to `last`'s size and summed with it
  View cbfuse(const std::vector<View>& parts, View last) {
    const Buf& lb = P->bufs[last.buf];
    const int o = new_buf(lb.H, lb.W, last.C);
    Op op{}; op.kind = 4; FuseP& f = op.fuse;
    f.n = (int)parts.size() + 1; CC_CHECK(f.n <= 6, "CBFuse: too many inputs");
    for (int k = 0; k < f.n; ++k) {
      const View& v = k + 1 < f.n ? parts[k] : last;
      const Buf& b = P->bufs[v.buf];
      CC_CHECK(v.C == last.C && lb.H % b.H == 0, "CBFuse input mismatch");
      int sh = 0; while ((b.H << sh) < lb.H) ++sh;
      CC_CHECK((b.H << sh) == lb.H && (b.W << sh) == lb.W, "CBFuse scale must be a power of two");
      f.in[k] = (const void*)(intptr_t)v.buf; f.H[k] = b.H; f.W[k] = b.W; f.cstride[k] = b.C; f.coff[k] = v.coff; f.shift[k] = sh;
    }
    f.out = (void*)(intptr_t)o; f.out_cstride = last.C; f.out_coff = 0; f.B = P->B; f.Ho = lb.H; f.Wo = lb.W; f.C = last.C;
    std::vector<Op::Access> acc{wr(whole(o)), rd(last)};
    for (const View& v : parts) acc.push_back(rd(v));
    push(op, std::move(acc));
    return whole(o);
  }

  // DDetect's last 1x1 convs + decode as ONE launch (detect.hip head_tail_kernel): the (B,A,144) f32 logits never reach HBM.
  // 16-bit storage, class-branch width a multiple of 32 up to 256 (sizes s, c, e); CLEARCAM_FUSE_HEAD=0 keeps the three launches per
  // level + decode_kernel (and with them the "raw<l>" parity taps, which the f32 mode always has).
  bool fuse_head_tail() const {
    const char* e = getenv("CLEARCAM_FUSE_HEAD");
    return (!e || atoi(e) != 0) && head_tail_supported(Y->dtype, a.cls_hidden, Y->wsplit);
  }
  // One level of DDetect (:157-220): the level's conv chain runs on its own lane - it only needs that level's feature map, so
  // P3's 1.3 ms of 3x3 convs overlap the neck's way down to P4 / P5 (whose 40x40 / 20x20 launches leave CUs idle) instead of queueing
  // behind it.  head_finish() joins the three lanes.
  Op head_dec{}, head_tail{};
  std::vector<Op::Access> head_acc;
  int head_levels = 0;
  void head_level(const std::string& H22, int l, View feat) {
    Lane lane(*this, 2 + l);
    const bool fused = fuse_head_tail();
    if (head_levels++ == 0) { head_dec = Op{}; head_dec.kind = 2; head_tail = Op{}; head_tail.kind = 7; head_acc.clear(); P->A = 0; }
    const std::string hb = H22 + "cv2.list." + std::to_string(l) + ".list.", hc = H22 + "cv3.list." + std::to_string(l) + ".list.";
    const int H = P->bufs[feat.buf].H, W = P->bufs[feat.buf].W, ch = a.cls_hidden;
    const int hbuf = new_buf(H, W, 64 + ch), bxb = new_buf(H, W, 64), clb = new_buf(H, W, ch);
    // The level's two entry convs (box: feat -> 64, class: feat -> ch; yolov9.py:205-206) read the same map.  As ONE 64 + ch channel GEMM
    // the input is read once - but 64 + 256 = 320 channels do not tile by 256, so the whole launch falls back to five 64-wide channel
    // tiles that each pull the activations again.  With ch a multiple of 256 the class conv alone takes the eight-wave 256-wide
    // kernel and the 64-channel box conv a launch of its own (cc_conv_bench, B = 64: 3x3 256 -> 320 at 80x80 857 us against 535 + 206,
    // split weights 1495 against 935 + 399; profiles/r04c_head_split.txt).  Same K order per channel: the same bits either way.
    // CLEARCAM_HEAD_SPLIT=0 keeps the single launch.
    static const bool head_split_on = [] { const char* e = getenv("CLEARCAM_HEAD_SPLIT"); return !(e && atoi(e) == 0); }();
    if (head_split_on && Y->dtype != F32 && ch % 256 == 0) {
      conv({{feat, 0}}, pconv({hb + "0.conv"}, {1}), slice(whole(hbuf), 0, 64), 1, 1);
      conv({{feat, 0}}, pconv({hc + "0.conv"}, {1}), slice(whole(hbuf), 64, ch), 1, 1);
    } else
    conv({{feat, 0}}, pconv({hb + "0.conv", hc + "0.conv"}, {1, 1}), whole(hbuf), 1, 1);
    conv({{slice(whole(hbuf), 0, 64), 0}}, pconv({hb + "1.conv"}, {4}), whole(bxb), 1, 1);
    conv({{slice(whole(hbuf), 64, ch), 0}}, pconv({hc + "1.conv"}, {1}), whole(clb), 1, 1);
    const PackedConv &c2 = pconv({hb + "2"}, {4}), &c3 = pconv({hc + "2"}, {1});
    if (fused) {
      CC_CHECK(c2.cin == 64 && c2.cout == 64 && c2.k == 1 && c3.cin == ch && c3.cout == 80 && c3.k == 1, "fused DDetect tail: unexpected conv shapes");
      HeadTailP& q = head_tail.tail;
      q.bx[l] = (const void*)(intptr_t)bxb; q.cl[l] = (const void*)(intptr_t)clb;
      q.w2[l] = c2.w; q.w3[l] = c3.w; q.b2[l] = c2.bias; q.b3[l] = c3.bias; q.kw2 = c2.kw; q.kw3 = c3.kw;
      q.split = c2.split; q.os2[l] = c2.oscale; q.os3[l] = c3.oscale;
      q.H[l] = H; q.W[l] = W;
      head_acc.push_back(rd(whole(bxb))); head_acc.push_back(rd(whole(clb)));
    } else {
      const int raw = new_buf(H, W, 144, true);
      conv({{whole(bxb), 0}}, c2, slice(whole(raw), 0, 64), 1, 0);
      conv({{whole(clb), 0}}, c3, slice(whole(raw), 64, 80), 1, 0);
      P->taps["raw" + std::to_string(l)] = raw;
      head_dec.dec.raw[l] = (const float*)(intptr_t)raw; head_dec.dec.H[l] = H; head_dec.dec.W[l] = W;
      head_acc.push_back(rd(whole(raw)));
    }
    P->A += H * W;
  }
  void head_finish() {
    CC_CHECK(head_levels == 3, "DDetect has three levels");
    head_acc.push_back(Op::Access{-2, 0, 1, true});
    if (fuse_head_tail()) {
      HeadTailP& q = head_tail.tail;
      q.B = P->B; q.A = P->A; q.ch = a.cls_hidden; q.dfl_w = Y->dfl_w; q.conf = 0.25f;
      push(head_tail, head_acc);
    } else {
      head_dec.dec.B = P->B; head_dec.dec.A = P->A; head_dec.dec.dfl_w = Y->dfl_w; head_dec.dec.conf = 0.25f;
      push(head_dec, head_acc);
    }
    Op nms{}; nms.kind = 3;
    nms.nms.B = P->B; nms.nms.A = P->A; nms.nms.iou_thr = 0.45f;
    // scale_boxes (:406-416): python-float arithmetic, then f32 tensor ops
    const double gain = std::min((double)P->Hn / P->H, (double)P->Wn / P->W);
    nms.nms.gain = (float)gain;
    nms.nms.pad_x = (float)((P->Wn - P->W * gain) / 2); nms.nms.pad_y = (float)((P->Hn - P->H * gain) / 2);
    nms.nms.src_w = (float)P->W; nms.nms.src_h = (float)P->H;
    push(nms, {Op::Access{-2, 0, 1, false}, Op::Access{-3, 0, 1, true}});
  }

  void build_e() {   // detection/yolov9.py:328-371
    const std::string M = "model.list.";
    const int cp = Y->cin_pad();
    P->in_buf = new_buf(P->Hn, P->Wn, cp);
    P->taps["input"] = P->in_buf;
    auto stem = [&](const std::string& n, View in, int cout, int cpad) {
      const Buf& b = P->bufs[in.buf];
      const int o = new_buf(b.H / 2, b.W / 2, cout);
      if (in.buf == P->in_buf && fuse_stem(cout)) stem_fused(n, pconv({n + ".conv"}, {1}, cpad), whole(o));
      else conv({{in, 0}}, pconv({n + ".conv"}, {1}, cpad), whole(o), 2, 1);
      return whole(o);
    };
    const View y1 = stem(M + "1", whole(P->in_buf), 64, cp), y2 = stem(M + "2", y1, 128, 0);
    const View y3 = elan4(M + "3", {{y2, 0}}, 32, 256), y4 = down(M + "4", y3, 256);
    const View y5 = elan4(M + "5", {{y4, 0}}, 64, 512), y6 = down(M + "6", y5, 512);
    const View y7 = elan4(M + "7", {{y6, 0}}, 128, 1024), y8 = down(M + "8", y7, 1024);
    const View y9 = elan4(M + "9", {{y8, 0}}, 128, 1024);
    const View c10 = cblinear(M + "10", y1), c11 = cblinear(M + "11", y3), c12 = cblinear(M + "12", y5),
               c13 = cblinear(M + "13", y7), c14 = cblinear(M + "14", y9);
    // split offsets: [64 | 128 | 256 | 512 | 1024]
    auto part = [&](View c, int idx) { static const int off[5] = {0, 64, 192, 448, 960}; return slice(c, off[idx], 64 << idx); };
    const View y15 = stem(M + "15", whole(P->in_buf), 64, cp);
    const View y16 = cbfuse({part(c10, 0), part(c11, 0), part(c12, 0), part(c13, 0), part(c14, 0)}, y15);
    const View y17 = stem(M + "17", y16, 128, 0);
    const View y18 = cbfuse({part(c11, 1), part(c12, 1), part(c13, 1), part(c14, 1)}, y17);
    const View y19 = elan4(M + "19", {{y18, 0}}, 32, 256), y20 = down(M + "20", y19, 256);
    const View y21 = cbfuse({part(c12, 2), part(c13, 2), part(c14, 2)}, y20);
    const View y22 = elan4(M + "22", {{y21, 0}}, 64, 512), y23 = down(M + "23", y22, 512);
    const View y24 = cbfuse({part(c13, 3), part(c14, 3)}, y23);
    const View y25 = elan4(M + "25", {{y24, 0}}, 128, 1024), y26 = down(M + "26", y25, 1024);
    const View y27 = cbfuse({part(c14, 4)}, y26);
    const View y28 = elan4(M + "28", {{y27, 0}}, 128, 1024);
    const View y29 = sppelan(M + "29", y28, 256, 512);
    const View y32 = elan4(M + "32", {{y29, 1}, {y25, 0}}, 128, 512);
    const View y35 = elan4(M + "35", {{y32, 1}, {y22, 0}}, 64, 256);
    head_level(M + "42.", 0, y35);
    const View y36 = down(M + "36", y35, 256);
    const View y38 = elan4(M + "38", {{y36, 0}, {y32, 0}}, 128, 512);
    head_level(M + "42.", 1, y38);
    const View y39 = down(M + "39", y38, 512);
    const View y41 = elan4(M + "41", {{y39, 0}, {y29, 0}}, 256, 512);
    head_level(M + "42.", 2, y41);
    P->taps["p3"] = y35.buf; P->taps["p4"] = y38.buf; P->taps["p5"] = y41.buf;
    head_finish();
  }

  void build() {
    if (!strcmp(a.size, "e")) { build_e(); return; }
    const std::string M = "model.list.";
    const int cp = Y->cin_pad();
    P->in_buf = new_buf(P->Hn, P->Wn, cp);
    P->taps["input"] = P->in_buf;
    const int b0 = new_buf(P->Hn / 2, P->Wn / 2, a.stem);
    if (getenv("CLEARCAM_TAP_STEM")) P->taps["stem"] = b0;       // tests: keep the first conv's output readable (costs arena)
    if (fuse_stem(a.stem)) stem_fused(M + "0", pconv({M + "0.conv"}, {1}, cp), whole(b0));
    else conv({{whole(P->in_buf), 0}}, pconv({M + "0.conv"}, {1}, cp), whole(b0), 2, 1);
    const int b1 = new_buf(P->Hn / 4, P->Wn / 4, 2 * a.stem);
    conv({{whole(b0), 0}}, pconv({M + "1.conv"}, {1}), whole(b1), 2, 1);
    const View y2 = a.elan1 ? elan1(M + "2", whole(b1), a.b2_hidden, a.b2_out) : elan4(M + "2", {{whole(b1), 0}}, a.b2_hidden, a.b2_out);
    const View y3 = down(M + "3", y2, a.d3_out);
    const View y4 = elan4(M + "4", {{y3, 0}}, a.e4_hidden, a.b4_out);
    const View y5 = down(M + "5", y4, a.d5_out);
    const View y6 = elan4(M + "6", {{y5, 0}}, a.e6_hidden, a.p4);
    const View y7 = down(M + "7", y6, a.d7_out);
    const View y8 = elan4(M + "8", {{y7, 0}}, a.e8_hidden, a.p5);
    const View y9 = sppelan(M + "9", y8, a.spp_hidden, a.p5);
    const View y12 = elan4(M + "12", {{y9, 1}, {y6, 0}}, a.e6_hidden, a.p4);
    const View y15 = elan4(M + "15", {{y12, 1}, {y4, 0}}, a.e4_hidden, a.p3);
    head_level(M + "22.", 0, y15);                               // DDetect (:157-220), each level as soon as its map exists
    const View y16 = down(M + "16", y15, a.d16_out);
    const View y18 = elan4(M + "18", {{y16, 0}, {y12, 0}}, a.e6_hidden, a.p4);
    head_level(M + "22.", 1, y18);
    const View y19 = down(M + "19", y18, a.d19_out);
    const View y21 = elan4(M + "21", {{y19, 0}, {y9, 0}}, a.e8_hidden, a.p5);
    head_level(M + "22.", 2, y21);
    P->taps["p3"] = y15.buf; P->taps["p4"] = y18.buf; P->taps["p5"] = y21.buf;
    if (getenv("CLEARCAM_TAP_BLOCKS")) {                         // development: every block's output readable ("b<block>": the WHOLE buffer the
      const std::pair<int, View> ys[] = {{2, y2}, {3, y3}, {4, y4}, {5, y5}, {6, y6}, {7, y7}, {8, y8}, {9, y9}, {12, y12}, {16, y16}, {19, y19}};   // view lives in)
      for (auto& kv : ys) {
        P->taps["b" + std::to_string(kv.first)] = kv.second.buf;
        fprintf(stderr, "[clearcam] tap b%d: channels [%d, %d) of a %d-channel buffer\n", kv.first, kv.second.coff, kv.second.coff + kv.second.C, P->bufs[kv.second.buf].C);
      }
      P->taps["b1"] = b1;
    }
    head_finish();
  }

  // Arena packing: a buffer lives from the first launch that touches it to the last; buffers whose lifetimes do not
  // overlap share memory (first-fit over buffers sorted by first use).  The letterboxed input and every tensor a
  // parity tap can ask for stay live to the end.  YOLOv9-C, B=64, 640x640, bf16: 12 GB of tensors -> ~3 GB of arena.
  // CLEARCAM_ARENA_REUSE=0 gives every buffer its own range (debugging).
  void pack_arena() {
    const char* e = getenv("CLEARCAM_ARENA_REUSE");
    if (e && atoi(e) == 0) return;
    const int nb = (int)P->bufs.size(), nops = (int)P->ops.size();
    std::vector<int> first(nb, nops + 1), last(nb, -2);
    auto touch = [&](const void* id, int t) {
      const intptr_t i = (intptr_t)id;
      if (i < 0 || i >= nb) return;
      first[i] = std::min(first[i], t); last[i] = std::max(last[i], t);
    };
    for (int t = 0; t < nops; ++t) {
      const Op& op = P->ops[t];
      if (op.kind == 0) { touch(op.conv.s0.ptr, t); touch(op.conv.s1.ptr, t); touch(op.conv.out, t); touch(op.conv.res, t); }
      else if (op.kind == 1) { touch(op.pool.in, t); touch(op.pool.out, t); }
      else if (op.kind == 2) { for (int l = 0; l < 3; ++l) touch(op.dec.raw[l], t); }
      else if (op.kind == 4) { for (int k = 0; k < op.fuse.n; ++k) touch(op.fuse.in[k], t); touch(op.fuse.out, t); }
      else if (op.kind == 5) touch(op.stem.out, -1);           // runs before the graph, whatever its position in the list
      else if (op.kind == 6) { touch(op.csp.x, t); touch(op.csp.out, t); }
      else if (op.kind == 7) { for (int l = 0; l < 3; ++l) { touch(op.tail.bx[l], t); touch(op.tail.cl[l], t); } }
    }
    // A launch on a side lane may run as late as its join: the first later launch of another lane that conflicts with that lane's
    // work from there on.  What it touches stays live until then (trunk launches never run later than their place in the list).
    auto same_tensor_conflict = [](const Op& x, const Op& y) {
      for (const Op::Access& p : x.acc) for (const Op::Access& q : y.acc)
        if ((p.write || q.write) && p.buf == q.buf && p.coff < q.coff + q.C && q.coff < p.coff + p.C) return true;
      return false;
    };
    for (int t = 0; t < nops; ++t) {
      const Op& op = P->ops[t];
      if (op.lane == 0) continue;
      int join = nops;
      for (int u = t + 1; u < nops && join == nops; ++u) {
        if (P->ops[u].lane == op.lane) continue;
        for (int v = t; v < u; ++v) if (P->ops[v].lane == op.lane && same_tensor_conflict(P->ops[v], P->ops[u])) { join = u; break; }
      }
      for (const Op::Access& x : op.acc) if (x.buf >= 0) last[x.buf] = std::max(last[x.buf], join);
    }
    first[P->in_buf] = -1;                                     // written by the letterbox kernel before the first op
    for (auto& kv : P->taps) last[kv.second] = nops + 1;       // cc_yolo_get_tensor reads these after the run
    for (int i = 0; i < nb; ++i) if (last[i] < first[i]) { first[i] = -1; last[i] = nops + 1; }   // never touched: keep apart
    auto bytes_of = [&](int i) {
      const Buf& b = P->bufs[i];
      const size_t n = (size_t)P->B * b.H * b.W * b.C * (b.f32 ? 4 : dtype_size(Y->dtype));
      return (n + 255) & ~(size_t)255;
    };
    std::vector<int> order(nb);
    for (int i = 0; i < nb; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return first[x] < first[y]; });
    std::vector<int> placed;
    size_t top = 0;
    for (int i : order) {
      const size_t need = bytes_of(i);
      // candidate offsets: 0 and the end of every placed buffer that is alive at the same time
      std::vector<std::pair<size_t, size_t>> busy;             // [off, end) of time-overlapping buffers
      for (int j : placed) if (!(last[j] < first[i] || last[i] < first[j])) busy.emplace_back(P->bufs[j].off, P->bufs[j].off + bytes_of(j));
      std::sort(busy.begin(), busy.end());
      size_t off = 0;
      for (auto& b : busy) { if (off + need <= b.first) break; off = std::max(off, b.second); }
      P->bufs[i].off = off;
      placed.push_back(i);
      top = std::max(top, off + need);
    }
    if (getenv("CLEARCAM_VERBOSE"))
      fprintf(stderr, "[clearcam] plan B=%d %dx%d: %d tensors, %.2f GB unpacked -> %.2f GB arena\n", P->B, P->Hn, P->Wn, nb,
              (double)P->arena_bytes / 1e9, (double)top / 1e9);
    P->arena_bytes = top;
  }

  void resolve() {
    pack_arena();
    CC_HIP(hipMalloc((void**)&P->arena, P->arena_bytes));
    CC_HIP(hipMemset(P->arena, 0, P->arena_bytes));
    CC_HIP(hipMalloc((void**)&P->det, (size_t)P->B * P->A * 6 * 4));
    CC_HIP(hipMalloc((void**)&P->out_dev, (size_t)P->B * CC_MAX_DET * 6 * 4));
    CC_HIP(hipMalloc((void**)&P->nonfinite, 256)); CC_HIP(hipMemset(P->nonfinite, 0, 256));
    auto ptr = [&](const void* id) -> char* { const intptr_t i = (intptr_t)id; return i < 0 ? nullptr : P->arena + P->bufs[i].off; };
    for (Op& op : P->ops) {
      if (op.kind == 0) {
        op.conv.s0.ptr = ptr(op.conv.s0.ptr); op.conv.s1.ptr = ptr(op.conv.s1.ptr);
        if (!op.conv.s1.ptr) op.conv.s1.ptr = op.conv.s0.ptr;
        op.conv.out = ptr(op.conv.out); op.conv.res = ptr(op.conv.res);
      } else if (op.kind == 1) { op.pool.in = ptr(op.pool.in); op.pool.out = ptr(op.pool.out); }
      else if (op.kind == 2) { for (int l = 0; l < 3; ++l) op.dec.raw[l] = (const float*)ptr(op.dec.raw[l]); op.dec.det = P->det; op.dec.nonfinite = P->nonfinite; }
      else if (op.kind == 4) { for (int k = 0; k < op.fuse.n; ++k) op.fuse.in[k] = ptr(op.fuse.in[k]); op.fuse.out = ptr(op.fuse.out); }
      else if (op.kind == 5) op.stem.out = ptr(op.stem.out);
      else if (op.kind == 6) { op.csp.x = ptr(op.csp.x); op.csp.out = ptr(op.csp.out); }
      else if (op.kind == 7) { for (int l = 0; l < 3; ++l) { op.tail.bx[l] = ptr(op.tail.bx[l]); op.tail.cl[l] = ptr(op.tail.cl[l]); } op.tail.det = P->det; op.tail.nonfinite = P->nonfinite; }
      else { op.nms.det = P->det; op.nms.out = P->out_dev; }
    }
  }
};

// tinygrad interpolate index tables in float32; mirrors oracle interp_axis_tables.
#pragma clang fp contract(off)
void axis_tables(int n_in, int n_out, std::vector<int>& lo, std::vector<int>& hi, std::vector<float>& fr) {
  lo.resize(n_out); hi.resize(n_out); fr.resize(n_out);
  const float scale = (float)((double)n_in / (double)n_out);
  for (int i = 0; i < n_out; ++i) {
    volatile float t = (float)i + 0.5f;
    volatile float u = scale * t;
    volatile float idx = u - 0.5f;
    float v = idx;
    if (v < 0.f) v = 0.f;
    if (v > (float)(n_in - 1)) v = (float)(n_in - 1);
    const float f = floorf(v);
    lo[i] = (int)f; hi[i] = (int)ceilf(v);
    volatile float d = v - f;
    fr[i] = d;
  }
}

static int round_half_even(double x) { return (int)std::nearbyint(x); }

template <class T> static T* to_device(const std::vector<T>& v) {
  T* d = nullptr;
  CC_HIP(hipMalloc((void**)&d, v.size() * sizeof(T) + 16));
  CC_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

// One launch of the plan.  Kind 5 (fused letterbox + first conv) reads the caller's frames: inside the captured graph it is skipped
// (run_stems launches it right before the graph); the profilers replay it on the frames of the last call.
static void launch_op(int dtype, const Plan* P, const Op& op, hipStream_t s, bool with_stem) {
  switch (op.kind) {
    case 0: launch_conv(dtype, op.conv, s); break;
    case 1: launch_pool(dtype, op.pool, s); break;
    case 2: launch_decode(op.dec, s); break;
    case 3: if (P->ragged) launch_topk_nms_ragged(op.nms, P->desc_dev, s); else launch_topk_nms(op.nms, s); break;
    case 4: launch_fuse(dtype, op.fuse, s); break;
    case 5: if (with_stem) { StemP q = op.stem; q.pre.frames = P->last_frames; launch_stem_fused(dtype, q, s); } break;
    case 6: launch_csp_fused(dtype, op.csp, s); break;
    case 7: launch_head_tail(dtype, op.tail, s); break;
    default: throw cc::Error(-22, "unknown op kind");
  }
}

static void run_ops(cc_yolo* Y, Plan* P, hipStream_t s) {
  for (const Op& op : P->ops) launch_op(Y->dtype, P, op, s, false);
}

// Two launches conflict when one writes what the other touches: overlapping channel ranges of one tensor, or overlapping arena bytes
// of two tensors that share memory (pack_arena).
static bool ops_conflict(const cc_yolo* Y, const Plan* P, const Op& x, const Op& y) {
  auto bytes = [&](int i) { const Buf& b = P->bufs[i]; return (size_t)P->B * b.H * b.W * b.C * (b.f32 ? 4 : dtype_size(Y->dtype)); };
  for (const Op::Access& p : x.acc)
    for (const Op::Access& q : y.acc) {
      if (!(p.write || q.write)) continue;
      if (p.buf < 0 || q.buf < 0) { if (p.buf == q.buf) return true; continue; }
      if (p.buf == q.buf) { if (p.coff < q.coff + q.C && q.coff < p.coff + p.C) return true; continue; }
      const size_t po = P->bufs[p.buf].off, qo = P->bufs[q.buf].off;
      if (po < qo + bytes(q.buf) && qo < po + bytes(p.buf)) return true;
    }
  return false;
}

// The plan under capture with its lanes as streams: lane 0 is the capturing stream, every other lane a side stream that joins the
// capture by waiting for an event of it.  A launch waits for the LAST conflicting launch of each other lane (stream order covers the
// earlier ones); all lanes are joined back before the capture ends.  Events recorded under capture are graph edges, not nodes.
static void run_ops_lanes(cc_yolo* Y, Plan* P, hipStream_t s) {
  const int nops = (int)P->ops.size();
  int nl = 1;
  for (const Op& op : P->ops) nl = std::max(nl, op.lane + 1);
  if (nl == 1) { run_ops(Y, P, s); return; }
  while ((int)Y->side.size() < nl - 1) Y->side.push_back(pool_stream_get(Y->device));
  auto stream_of = [&](int lane) { return lane == 0 ? s : Y->side[lane - 1]; };
  std::vector<hipEvent_t>& ev = P->lane_ev;             // owned by the plan: they outlive the capture
  ev.assign(nops + 1, nullptr);
  {
    std::vector<char> joined(nl, 0); joined[0] = 1;
    std::vector<std::vector<int>> seen(nl, std::vector<int>(nl, -1));   // seen[l][m]: last launch of lane m that lane l has waited for
    std::vector<int> tail(nl, -1);                                       // last launch of each lane
    for (int i = 0; i < nops; ++i) {
      const Op& op = P->ops[i];
      if (op.kind == 5) continue;                                        // runs before the graph
      const int l = op.lane; hipStream_t st = stream_of(l);
      std::vector<int> need(nl, -1);
      for (int j = 0; j < i; ++j) { const Op& o = P->ops[j]; if (o.kind != 5 && o.lane != l && ops_conflict(Y, P, op, o)) need[o.lane] = j; }
      bool waited = false;
      for (int m = 0; m < nl; ++m) if (need[m] > seen[l][m]) {
        CC_HIP(hipStreamWaitEvent(st, ev[need[m]], 0)); seen[l][m] = need[m]; waited = true;
      }
      if (!joined[l]) {
        if (!waited) {                                                   // no producer on another lane: fork from the trunk's current point
          if (!ev[nops]) CC_HIP(hipEventCreateWithFlags(&ev[nops], hipEventDisableTiming));
          CC_HIP(hipEventRecord(ev[nops], s)); CC_HIP(hipStreamWaitEvent(st, ev[nops], 0));
        }
        joined[l] = 1;
      }
      launch_op(Y->dtype, P, op, st, false);
      CC_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
      CC_HIP(hipEventRecord(ev[i], st));
      tail[l] = i;
    }
    for (int m = 1; m < nl; ++m) if (joined[m] && tail[m] > seen[0][m]) CC_HIP(hipStreamWaitEvent(s, ev[tail[m]], 0));
  }
}

// The fused letterbox + first conv launches read the caller's frames, whose address changes from call to call, so they
// stay outside the captured graph and run right before it.
static void run_stems(cc_yolo* Y, Plan* P, const void* frames, hipStream_t s) {
  for (Op& op : P->ops) if (op.kind == 5) {
    op.stem.pre.frames = frames;
    if (P->ragged) launch_stem_fused_ragged(Y->dtype, op.stem, P->desc_dev, P->packed_bytes, P->stem_big, s);
    else launch_stem_fused(Y->dtype, op.stem, s);
  }
}

// letterbox geometry, detection/yolov9.py:390-403 (python round = half-to-even)
static void letterbox_geometry(int H, int W, int res, int& nh, int& nw, int& pad_y, int& pad_x) {
  const double r = std::min((double)res / H, (double)res / W);
  nw = round_half_even(W * r); nh = round_half_even(H * r);
  const double dw = ((res - nw) % 32) / 2.0, dh = ((res - nh) % 32) / 2.0;
  pad_x = round_half_even(dw - 0.1); pad_y = round_half_even(dh - 0.1);
}
static const char* kNot32 = "letterboxed frame is not a multiple of 32 (the reference graph cannot run this shape either)";

// ragged: H x W IS the network shape; the key carries the flag and NOT the source sizes, so a camera that changes resolution keeps its graph
static Plan* get_plan(cc_yolo* Y, int B, int H, int W, int frame_f32, int slot = 0, bool ragged = false) {
  std::vector<int> key{B, H, W, frame_f32, slot};
  if (ragged) key.push_back(1);
  if (Plan* hit = Y->plans.find(key)) return hit;
  std::unique_ptr<Plan> P(new Plan());
  P->B = B; P->H = H; P->W = W; P->frame_f32 = frame_f32; P->ragged = ragged;
  if (ragged) { P->nh = H; P->nw = W; P->pad_x = P->pad_y = 0; }
  else letterbox_geometry(H, W, Y->res, P->nh, P->nw, P->pad_y, P->pad_x);
  P->Hn = P->nh + 2 * P->pad_y; P->Wn = P->nw + 2 * P->pad_x;
  CC_CHECK(P->Hn % 32 == 0 && P->Wn % 32 == 0 && P->Hn > 0 && P->Wn > 0, kNot32);
  std::vector<int> lo, hi; std::vector<float> fr;
  axis_tables(W, P->nw, lo, hi, fr); P->xlo = to_device(lo); P->xhi = to_device(hi); P->xfr = to_device(fr);
  axis_tables(H, P->nh, lo, hi, fr); P->ylo = to_device(lo); P->yhi = to_device(hi); P->yfr = to_device(fr);
  Builder bld(Y, P.get());
  bld.build();
  bld.resolve();
  if (ragged) {                                          // the staging buffer for host frames grows with the calls (stage_frames)
    CC_HIP(hipMalloc((void**)&P->desc_dev, (size_t)B * sizeof(FrameDesc)));
    CC_HIP(hipMemset(P->desc_dev, 0, (size_t)B * sizeof(FrameDesc)));
    CC_HIP(hipHostMalloc((void**)&P->desc_host, (size_t)B * sizeof(FrameDesc)));
    CC_HIP(hipEventCreateWithFlags(&P->desc_up, hipEventDisableTiming));
  } else {
    P->frames_bytes = (size_t)B * H * W * 3 * (frame_f32 ? 4 : 1);
    CC_HIP(hipMalloc(&P->frames_dev, P->frames_bytes));
  }
  // capture the launch list once; replay afterwards (the TinyJit role, helpers.py:214-221)
  hipGraph_t graph = nullptr;
  CC_HIP(hipStreamBeginCapture(Y->stream, hipStreamCaptureModeThreadLocal));
  try { run_ops_lanes(Y, P.get(), Y->stream); } catch (...) { hipStreamEndCapture(Y->stream, &graph); if (graph) hipGraphDestroy(graph); throw; }
  CC_HIP(hipStreamEndCapture(Y->stream, &graph));
  CC_HIP(hipGraphInstantiate(&P->exec, graph, nullptr, nullptr, 0));
  CC_HIP(hipGraphDestroy(graph));
  ++Y->plans_built;
  // a plan that cc_yolo_get_tensor / cc_yolo_profile still point at must not dangle when it is evicted
  return Y->plans.insert(key, std::move(P), Y->stream, [&](Plan* gone) {
    for (hipStream_t t : Y->slot_stream) hipStreamSynchronize(t);        // the evicted plan may be running on a slot's stream
    if (Y->last == gone) Y->last = nullptr;
  });
}

}  // namespace cc

namespace cc {

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

// Slots of a handle (batches in flight) must not share a hardware queue: the runtime maps streams onto a small pool of queues
// (GPU_MAX_HW_QUEUES, 4 unless the environment says otherwise, handed out least-used first), packets of one queue run in order, and
// two slots on one queue do not overlap at all.  So a new slot's stream is PROBED against the streams it has to run beside and
// replaced until it overlaps with all of them; rejected streams stay alive until the end so that the runtime moves on to another
// queue.  (Stream priority classes have queue pools of their own and would separate three slots by construction, but strict
// priority only fills gaps: 10.7 ms per B = 64 detect step against 10.1 with three equal slots.)
thread_local LaunchNote g_launch_note = {"", 0, 1};
thread_local bool g_note_launches = false;
static std::mutex g_pool_mu;
static std::map<int, std::deque<hipStream_t>> g_pool;
hipStream_t pool_stream_get(int device, bool fresh) {
  if (!fresh) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto& q = g_pool[device];
    if (!q.empty()) { hipStream_t s = q.front(); q.pop_front(); return s; }
  }
  hipStream_t s = nullptr;
  CC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return s;
}
hipStream_t pool_stream_get(int device) { return pool_stream_get(device, false); }
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

}  // namespace cc

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
namespace cc { void set_error(const std::string& m) { g_err = m; } }

#define CC_API_BEGIN try {
#define CC_API_END                                                         \
  return 0; }                                                              \
  catch (const cc::Error& e) { cc::set_error(e.what()); return e.code; }   \
  catch (const std::exception& e) { cc::set_error(e.what()); return -1; }

extern "C" {

const char* cc_last_error(void) { return g_err.c_str(); }
int cc_version(void) { return 100; }
int cc_device_count(int* n) { CC_API_BEGIN CC_HIP(hipGetDeviceCount(n)); CC_API_END }

static void input_step(cc_yolo* h, Plan* P, hipStream_t s, const void* fdev);   // letterbox (below)
static void detect_on_plan(cc_yolo* h, Plan* P, const void* frames, size_t bytes, int frames_on_device, float* out, int out_on_device, void* stream);
static int next_slot(cc_yolo* h);
static void submit_on_plan(cc_yolo* h, Plan* P, int slot, const void* frames, size_t bytes, int frames_on_device, float* out, int out_on_device,
                           void* stream, long long* ticket);

// dtype "f16c": the float32 weights of the 1x1 convs in h->host are replaced by f16-representable values chosen by the GPTQ recursion
// (calibrate.hip) on the second moments of each conv's own input - measured on an f32 twin of the handle running the calibration frames
// launch by launch (the inputs of conv i are in the arena right before launch i) - before the usual finalize packs them.  Convs that share
// an input and were packed together (RepNCSP's cv1 | cv2) share H.  Left to controlled rounding: 3x3 convs, grouped convs, DDetect.
static void calibrate_1x1(cc_yolo* h) {
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
    if (op.kind == 0 && c.ks == 1 && c.stride == 1 && c.pad == 0 && c.s0.shift >= 0 && c.s1.shift >= 0) {
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

int cc_yolo_create(cc_yolo** h, const char* size, int res, int dtype, int device) {
  CC_API_BEGIN
  CC_CHECK(h && size, "null argument");
  CC_CHECK(dtype >= 0 && dtype <= 5, "dtype must be 0 (f32), 1 (f16), 2 (bf16), 3 (f16 storage with split f16 weights), 4 (... in the backbone only) or 5 (f16, calibrated 1x1 weights)");
  CC_CHECK(res > 0 && res % 32 == 0, "res must be a positive multiple of 32");
  const Arch* a = nullptr;
  for (const Arch& x : kArch) if (!strcmp(x.size, size)) a = &x;
  CC_CHECK(a, std::string("unknown model size '") + size + "' (t, s, m, c, e)");
  int n = 0; CC_HIP(hipGetDeviceCount(&n));
  CC_CHECK(n > 0 && device >= 0 && device < n, "no such HIP device");
  CC_HIP(hipSetDevice(device));
  std::unique_ptr<cc_yolo> y(new cc_yolo());
  y->arch = a; y->res = res; y->dtype = storage_dtype(dtype); y->wsplit = dtype == F16S || dtype == F16H || dtype == F16C; y->device = device;
  if (dtype == F16H) {
    // development switches (tools/dev/hybrid_eval.py, test_split_boundaries): the last block whose every conv / whose 1x1 convs carry the low plane
    const char *ea = getenv("CLEARCAM_SPLIT_ALL_LAST"), *e1 = getenv("CLEARCAM_SPLIT_1X1_LAST");
    const bool e = !strcmp(size, "e");                               // "e": block 1 is the first conv, block 29 the SPPELAN
    y->split_all_last = ea ? atoi(ea) : (e ? 1 : 0);
    y->split_1x1_last = e1 ? atoi(e1) : (e ? 29 : 9);
  }
  if (dtype == F16C) {                                   // two planes in the stem conv only; the 1x1 convs are calibrated at finalize
    y->calibrated = true;
    y->split_all_last = !strcmp(size, "e") ? 1 : 0;
    y->split_1x1_last = -1;
  }
  y->stream = pool_stream_get(device);
  CC_HIP(hipEventCreate(&y->ev0)); CC_HIP(hipEventCreate(&y->ev1));
  CC_HIP(hipHostMalloc((void**)&y->nonfinite_host, 64, hipHostMallocDefault)); y->nonfinite_host[0] = y->nonfinite_host[1] = 0;
  *h = y.release();
  CC_API_END
}

int cc_yolo_load(cc_yolo* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  CC_API_BEGIN
  CC_CHECK(h && name && data && shape && ndim >= 0 && ndim <= 4, "bad argument");
  CC_CHECK(!h->finalized, "cc_yolo_load after cc_yolo_finalize");
  HostTensor t; size_t n = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
  t.data.assign(data, data + n);
  h->host[name] = std::move(t);
  CC_API_END
}

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

int cc_yolo_finalize(cc_yolo* h) {
  CC_API_BEGIN
  CC_CHECK(h, "null handle");
  CC_HIP(hipSetDevice(h->device));
  const std::string dfl = std::string("model.list.") + (!strcmp(h->arch->size, "e") ? "42" : "22") + ".dfl.conv.weight";
  auto d = h->host.find(dfl);
  CC_CHECK(d != h->host.end() && d->second.data.size() == 16, "missing parameter " + dfl);
  CC_HIP(hipMalloc((void**)&h->dfl_w, 64));
  CC_HIP(hipMemcpy(h->dfl_w, d->second.data.data(), 64, hipMemcpyHostToDevice));
  if (h->calibrated) calibrate_1x1(h);
  // dry-run build at B=1, res x res: packs every conv and proves the parameter set is complete
  Plan P; P.B = 1; P.H = P.W = P.Hn = P.Wn = h->res; P.nh = P.nw = h->res; P.pad_x = P.pad_y = 0;
  Builder(h, &P).build();
  h->finalized = true;
  h->host.clear();
  std::vector<unsigned char>().swap(h->calib_frames);
  CC_API_END
}

// One batch through plan P on stream s: the letterbox (or the fused letterbox + first conv launches, which read the caller's frames)
// and then the captured graph.
static void input_step(cc_yolo* h, Plan* P, hipStream_t s, const void* fdev) {
  PreP pp{};
  pp.frames = fdev; pp.frame_f32 = P->frame_f32; pp.B = P->B; pp.H = P->H; pp.W = P->W;
  pp.nh = P->nh; pp.nw = P->nw; pp.pad_y = P->pad_y; pp.pad_x = P->pad_x; pp.Hn = P->Hn; pp.Wn = P->Wn;
  pp.xlo = P->xlo; pp.xhi = P->xhi; pp.xfr = P->xfr; pp.ylo = P->ylo; pp.yhi = P->yhi; pp.yfr = P->yfr;
  pp.out = P->arena + P->bufs[P->in_buf].off; pp.out_c = P->bufs[P->in_buf].C;
  pp.flip = 1; pp.div = 255.0f; pp.sub = 0.0f; pp.pad_val = 0.0f;          // [..., ::-1] and / 255.0 (detection/yolov9.py:377-379)
  if (P->fused_stem) run_stems(h, P, fdev, s);
  else if (P->ragged) launch_preprocess_ragged(h->dtype, pp, P->desc_dev, P->packed_bytes, s);
  else launch_preprocess(h->dtype, pp, s);
  P->last_frames = fdev;
}
// Host frames go through the plan's staging buffer.  A uniform plan's is allocated with the plan; a ragged plan's grows to the largest
// packed buffer seen (hipFree waits for the device, so no batch in flight still reads the old one).
static const void* stage_frames(Plan* P, const void* frames, size_t bytes, hipStream_t s) {
  if (P->frames_bytes < bytes) {
    if (P->frames_dev) { CC_HIP(hipFree(P->frames_dev)); P->frames_dev = nullptr; P->frames_bytes = 0; }
    CC_HIP(hipMalloc(&P->frames_dev, bytes));
    P->frames_bytes = bytes;
  }
  CC_HIP(hipMemcpyAsync(P->frames_dev, frames, bytes, hipMemcpyHostToDevice, s));
  return P->frames_dev;
}
// ragged plan: this call's records go up on the plan's stream, ahead of the stem launches and the graph that read them
static void upload_desc(Plan* P, hipStream_t s) {
  if (!P->ragged) return;
  CC_HIP(hipMemcpyAsync(P->desc_dev, P->desc_host, (size_t)P->B * sizeof(FrameDesc), hipMemcpyHostToDevice, s));
  CC_HIP(hipEventRecord(P->desc_up, s));
  P->desc_pending = true;
}
static void enqueue_step(cc_yolo* h, Plan* P, hipStream_t s, const void* fdev) {
  input_step(h, P, s, fdev);
  if (getenv("CLEARCAM_EAGER_DEBUG")) {                      // development: launch by launch with a sync and a trace line after each
    int i = 0;
    for (const Op& op : P->ops) {
      launch_op(h->dtype, P, op, s, false);
      const hipError_t e = hipStreamSynchronize(s);
      fprintf(stderr, "[clearcam] op %d kind %d: %s\n", i, op.kind, hipGetErrorString(e)); fflush(stderr);
      ++i;
    }
  } else
  CC_HIP(hipGraphLaunch(P->exec, s));
}

int cc_yolo_detect(cc_yolo* h, const void* frames, int B, int H, int W, int frame_f32, int frames_on_device,
                   float* out, int out_on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && frames && out, "null argument");
  CC_CHECK(h->finalized, "cc_yolo_detect before cc_yolo_finalize");
  CC_CHECK(B > 0 && H > 0 && W > 0, "bad frame shape");
  CC_HIP(hipSetDevice(h->device));
  Plan* P = get_plan(h, B, H, W, frame_f32 ? 1 : 0);
  detect_on_plan(h, P, frames, P->frames_bytes, frames_on_device, out, out_on_device, stream);
  CC_API_END
}

// cc_yolo_detect / cc_yolo_detect_ragged from the plan on: `bytes` of frames (uniform: B*H*W*3 elements; ragged: the packed buffer)
static void detect_on_plan(cc_yolo* h, Plan* P, const void* frames, size_t bytes, int frames_on_device, float* out, int out_on_device, void* stream) {
  const int B = P->B;
  hipStream_t s = h->stream;
  if (stream) {   // order our stream after the caller's
    hipEvent_t e; CC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    CC_HIP(hipEventRecord(e, (hipStream_t)stream)); CC_HIP(hipStreamWaitEvent(s, e, 0)); CC_HIP(hipEventDestroy(e));
  }
  const void* fdev = frames_on_device ? frames : stage_frames(P, frames, bytes, s);
  upload_desc(P, s);
  // the plan's non-finite counter sums over the plan's life (device-output / submitted batches are read by cc_yolo_nonfinite): a host-output
  // call answers for ITS OWN batch only - the counter is snapshotted before the step and the difference is what this call reports
  if (!out_on_device) CC_HIP(hipMemcpyAsync(h->nonfinite_host + 1, P->nonfinite, 4, hipMemcpyDeviceToHost, s));
  CC_HIP(hipEventRecord(h->ev0, s));
  enqueue_step(h, P, s, fdev);
  CC_HIP(hipEventRecord(h->ev1, s));
  const size_t ob = (size_t)B * CC_MAX_DET * 6 * 4;
  if (out_on_device) {
    CC_HIP(hipMemcpyAsync(out, P->out_dev, ob, hipMemcpyDeviceToDevice, s));
    if (stream) {
      hipEvent_t e; CC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      CC_HIP(hipEventRecord(e, s)); CC_HIP(hipStreamWaitEvent((hipStream_t)stream, e, 0)); CC_HIP(hipEventDestroy(e));
    }
  } else {
    CC_HIP(hipMemcpyAsync(out, P->out_dev, ob, hipMemcpyDeviceToHost, s));
    CC_HIP(hipMemcpyAsync(h->nonfinite_host, P->nonfinite, 4, hipMemcpyDeviceToHost, s));
    CC_HIP(hipStreamSynchronize(s));
    h->last = P;
    if (h->nonfinite_host[0] != h->nonfinite_host[1]) {     // the rows are in `out` (garbage where the logits were); say why
      const int n = h->nonfinite_host[0] - h->nonfinite_host[1];
      // this batch's anchors have been reported: take them out of the running count (earlier device-output batches stay in it)
      CC_HIP(hipMemcpyAsync(P->nonfinite, h->nonfinite_host + 1, 4, hipMemcpyHostToDevice, s)); CC_HIP(hipStreamSynchronize(s));
      h->nonfinite_host[0] = h->nonfinite_host[1];
      throw cc::Error(-34, std::to_string(n) + " anchors with non-finite logits: activations left the storage type's range (f16 saturates at 65504) - "
                           "run this checkpoint with dtype bf16 or f32");
    }
  }
  h->last = P;
}

// taps and profilers read what the last call left behind: every stream of the handle has to be idle
static void sync_all(cc_yolo* h) {
  CC_HIP(hipStreamSynchronize(h->stream));
  for (hipStream_t t : h->slot_stream) CC_HIP(hipStreamSynchronize(t));
}

int cc_yolo_set_in_flight(cc_yolo* h, int n) {
  CC_API_BEGIN
  CC_CHECK(h && n >= 1 && n <= 8, "in-flight depth must be 1..8");
  CC_HIP(hipSetDevice(h->device));
  if (n == (int)h->slot_stream.size() + 1 && !h->slot_done.empty()) return 0;   // same depth: plans, slots and outstanding tickets stay valid
  sync_all(h);
  h->plans.clear();                                     // plans are built for one depth (lanes on or off) and belong to a slot
  h->last = nullptr;
  while ((int)h->slot_stream.size() > n - 1) { pool_stream_put(h->device, h->slot_stream.back()); h->slot_stream.pop_back(); }
  grow_slot_streams(h->device, h->stream, h->slot_stream, n - 1);      // probed: kernels on any two of them really run side by side
  while ((int)h->slot_done.size() > n) { hipEventDestroy(h->slot_done.back()); h->slot_done.pop_back(); }
  while ((int)h->slot_done.size() < n) { hipEvent_t e; CC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->slot_done.push_back(e); }
  h->submitted = 0;
  CC_API_END
}

int cc_yolo_submit(cc_yolo* h, const void* frames, int B, int H, int W, int frame_f32, int frames_on_device, float* out, int out_on_device,
                   void* stream, long long* ticket) {
  CC_API_BEGIN
  CC_CHECK(h && frames && out && ticket, "null argument");
  CC_CHECK(h->finalized, "cc_yolo_submit before cc_yolo_finalize");
  CC_CHECK(B > 0 && H > 0 && W > 0, "bad frame shape");
  CC_HIP(hipSetDevice(h->device));
  const int slot = next_slot(h);
  Plan* P = get_plan(h, B, H, W, frame_f32 ? 1 : 0, slot);
  submit_on_plan(h, P, slot, frames, P->frames_bytes, frames_on_device, out, out_on_device, stream, ticket);
  CC_API_END
}

// the slot the next submission runs on (round robin over the in-flight depth)
static int next_slot(cc_yolo* h) {
  if (h->slot_done.empty()) { hipEvent_t e; CC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->slot_done.push_back(e); }
  const int depth = (int)h->slot_stream.size() + 1;
  return (int)(h->submitted % depth);
}
// cc_yolo_submit / cc_yolo_submit_ragged from the plan on (`bytes` as detect_on_plan)
static void submit_on_plan(cc_yolo* h, Plan* P, int slot, const void* frames, size_t bytes, int frames_on_device, float* out, int out_on_device,
                           void* stream, long long* ticket) {
  const int B = P->B;
  hipStream_t s = h->stream_of_slot(slot);
  if (stream) {   // the frames are ready on the caller's stream; the caller's stream is NOT made to wait for the result (cc_yolo_wait does that)
    hipEvent_t e; CC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    CC_HIP(hipEventRecord(e, (hipStream_t)stream)); CC_HIP(hipStreamWaitEvent(s, e, 0)); CC_HIP(hipEventDestroy(e));
  }
  // host frames / rows (pinned, or the copies are not asynchronous): upload, detect and download are one in-order chain on the slot's
  // stream, and the chains of the slots overlap - the upload of one batch runs under the convs of another
  const void* fdev = frames_on_device ? frames : stage_frames(P, frames, bytes, s);
  upload_desc(P, s);
  enqueue_step(h, P, s, fdev);
  CC_HIP(hipMemcpyAsync(out, P->out_dev, (size_t)B * CC_MAX_DET * 6 * 4, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  CC_HIP(hipEventRecord(h->slot_done[slot], s));
  h->last = P;
  *ticket = h->submitted++;
}

int cc_yolo_wait(cc_yolo* h, long long ticket, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h, "null handle");
  const int depth = (int)h->slot_stream.size() + 1;
  CC_CHECK(ticket >= 0 && ticket < h->submitted, "no such submission");
  // a slot's stream runs its submissions in order: once a LATER submission of the same slot has been recorded, the slot's event
  // stands for that one, which finishes after this one - waiting for it is still correct (only later than necessary)
  CC_HIP(hipSetDevice(h->device));
  hipEvent_t e = h->slot_done[(int)(ticket % depth)];
  if (stream) CC_HIP(hipStreamWaitEvent((hipStream_t)stream, e, 0));
  else CC_HIP(hipEventSynchronize(e));
  CC_API_END
}

int cc_letterbox_geometry(int H, int W, int res, int* nh, int* nw, int* pad_y, int* pad_x) {
  CC_API_BEGIN
  CC_CHECK(H > 0 && W > 0 && res > 0 && nh && nw && pad_y && pad_x, "bad argument");
  letterbox_geometry(H, W, res, *nh, *nw, *pad_y, *pad_x);
  CC_API_END
}

// The frame's tables for one axis, from the handle's cache (built and uploaded the first time a size is seen).
static cc_yolo::AxisTab& axis_tab(cc_yolo* h, int n_in, int n_out) {
  auto it = h->axis_tabs.find({n_in, n_out});
  if (it == h->axis_tabs.end()) {
    std::vector<int> lo, hi; std::vector<float> fr;
    axis_tables(n_in, n_out, lo, hi, fr);
    char* d = nullptr;
    CC_HIP(hipMalloc((void**)&d, (size_t)n_out * 12 + 16));
    CC_HIP(hipMemcpy(d, lo.data(), (size_t)n_out * 4, hipMemcpyHostToDevice));
    CC_HIP(hipMemcpy(d + (size_t)n_out * 4, hi.data(), (size_t)n_out * 4, hipMemcpyHostToDevice));
    CC_HIP(hipMemcpy(d + (size_t)n_out * 8, fr.data(), (size_t)n_out * 4, hipMemcpyHostToDevice));
    it = h->axis_tabs.emplace(std::make_pair(n_in, n_out), cc_yolo::AxisTab{(int*)d, (int*)(d + (size_t)n_out * 4), (float*)(d + (size_t)n_out * 8), 0}).first;
  }
  it->second.used = ++h->axis_tick;
  return it->second;
}
constexpr size_t kMaxAxisTabs = 256;

// Checks a ragged call, finds (or builds) its plan and fills the plan's pinned records; *bytes = size of the packed buffer.
static Plan* ragged_prepare(cc_yolo* h, const void* pixels, const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B,
                            int frame_f32, int slot, size_t* bytes) {
  CC_CHECK(pixels && offsets && heights && widths && B > 0, "null argument / empty batch");
  const size_t es = frame_f32 ? 4 : 1;
  struct Geo { int nh, nw, pad_y, pad_x; };
  std::vector<Geo> geo(B);
  int Hn = 0, Wn = 0;
  size_t end = 0;
  for (int b = 0; b < B; ++b) {
    const std::string who = "frame " + std::to_string(b) + " (" + std::to_string(heights[b]) + "x" + std::to_string(widths[b]) + ")";
    if (heights[b] <= 0 || widths[b] <= 0 || offsets[b] < 0) throw cc::Error(-22, who + ": bad shape or offset");
    if (frame_f32 && offsets[b] % 4 != 0) throw cc::Error(-22, who + ": float32 frames must start at a multiple of 4 bytes");
    Geo& g = geo[b];
    letterbox_geometry(heights[b], widths[b], h->res, g.nh, g.nw, g.pad_y, g.pad_x);
    const int hn = g.nh + 2 * g.pad_y, wn = g.nw + 2 * g.pad_x;
    if (!(hn % 32 == 0 && wn % 32 == 0 && hn > 0 && wn > 0 && g.nh > 0 && g.nw > 0)) throw cc::Error(-22, who + ": " + kNot32);
    if (b == 0) { Hn = hn; Wn = wn; }
    else if (hn != Hn || wn != Wn)
      throw cc::Error(-22, who + " letterboxes to " + std::to_string(hn) + "x" + std::to_string(wn) + " but frame 0 (" + std::to_string(heights[0]) + "x" +
                               std::to_string(widths[0]) + ") to " + std::to_string(Hn) + "x" + std::to_string(Wn) +
                               ": the frames of one ragged batch must share one network shape (group them with cc_letterbox_geometry)");
    end = std::max(end, (size_t)offsets[b] + (size_t)heights[b] * widths[b] * 3 * es);
  }
  Plan* P = get_plan(h, B, Hn, Wn, frame_f32 ? 1 : 0, slot, true);
  // the pinned records may still be the source of the previous upload on this plan (see Plan): wait for that copy, not for the batch
  if (P->desc_pending) { CC_HIP(hipEventSynchronize(P->desc_up)); P->desc_pending = false; }
  if (h->axis_tabs.size() > kMaxAxisTabs) {             // bounded: drop the least recently used half once nothing in flight can read them
    sync_all(h);
    std::vector<std::pair<unsigned long long, std::pair<int, int>>> byage;
    for (auto& kv : h->axis_tabs) byage.emplace_back(kv.second.used, kv.first);
    std::sort(byage.begin(), byage.end());
    for (size_t i = 0; i < byage.size() / 2; ++i) { hipFree(h->axis_tabs[byage[i].second].lo); h->axis_tabs.erase(byage[i].second); }
  }
  bool big = false;
  for (int b = 0; b < B; ++b) {
    const Geo& g = geo[b];
    const int H = heights[b], W = widths[b];
    FrameDesc d{};
    d.off = offsets[b]; d.H = H; d.W = W; d.nh = g.nh; d.nw = g.nw; d.pad_y = g.pad_y; d.pad_x = g.pad_x;
    const cc_yolo::AxisTab &tx = axis_tab(h, W, g.nw), &ty = axis_tab(h, H, g.nh);
    d.xlo = tx.lo; d.xhi = tx.hi; d.xfr = tx.fr; d.ylo = ty.lo; d.yhi = ty.hi; d.yfr = ty.fr;
    // scale_boxes exactly as the uniform plan's NMS launch gets it (Builder::head_finish): double arithmetic, then one cast to float
    const double gain = std::min((double)Hn / H, (double)Wn / W);
    d.gain = (float)gain;
    d.fpad_x = (float)((Wn - W * gain) / 2); d.fpad_y = (float)((Hn - H * gain) / 2);
    d.src_w = (float)W; d.src_h = (float)H;
    P->desc_host[b] = d;
    big = big || stem_needs_big(H, W, g.nh, g.nw, frame_f32);
  }
  P->stem_big = big; P->packed_bytes = end;
  *bytes = end;
  return P;
}

int cc_yolo_detect_ragged(cc_yolo* h, const void* pixels, const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B,
                          int frame_f32, int pixels_on_device, float* out, int out_on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && out, "null argument");
  CC_CHECK(h->finalized, "cc_yolo_detect_ragged before cc_yolo_finalize");
  CC_HIP(hipSetDevice(h->device));
  size_t bytes = 0;
  Plan* P = ragged_prepare(h, pixels, offsets, heights, widths, B, frame_f32, 0, &bytes);
  detect_on_plan(h, P, pixels, bytes, pixels_on_device, out, out_on_device, stream);
  CC_API_END
}

int cc_yolo_submit_ragged(cc_yolo* h, const void* pixels, const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B,
                          int frame_f32, int pixels_on_device, float* out, int out_on_device, void* stream, long long* ticket) {
  CC_API_BEGIN
  CC_CHECK(h && out && ticket, "null argument");
  CC_CHECK(h->finalized, "cc_yolo_submit_ragged before cc_yolo_finalize");
  CC_HIP(hipSetDevice(h->device));
  const int slot = next_slot(h);
  size_t bytes = 0;
  Plan* P = ragged_prepare(h, pixels, offsets, heights, widths, B, frame_f32, slot, &bytes);
  submit_on_plan(h, P, slot, pixels, bytes, pixels_on_device, out, out_on_device, stream, ticket);
  CC_API_END
}

int cc_yolo_plans_built(cc_yolo* h, int* n) {
  CC_API_BEGIN
  CC_CHECK(h && n, "null argument");
  *n = h->plans_built;
  CC_API_END
}

// frames [b0, b0 + nb) of a tap; nb < 0: every frame
static int get_tensor_frames(cc_yolo* h, const char* name, int b0, int nb, float* out, int64_t* shape, int* ndim) {
  CC_API_BEGIN
  CC_CHECK(h && name && shape && ndim, "null argument");
  CC_CHECK(h->last, "no detect call yet");
  Plan* P = h->last;
  if (nb < 0) { b0 = 0; nb = P->B; }
  CC_CHECK(b0 >= 0 && nb >= 1 && b0 < P->B && nb <= P->B - b0, "frame range outside [0, B)");
  CC_HIP(hipSetDevice(h->device));
  sync_all(h);
  if (!strcmp(name, "decoded")) {
    shape[0] = nb; shape[1] = P->A; shape[2] = 6; *ndim = 3;
    if (out) CC_HIP(hipMemcpy(out, P->det + (size_t)b0 * P->A * 6, (size_t)nb * P->A * 24, hipMemcpyDeviceToHost));
    return 0;
  }
  auto it = P->taps.find(name);
  CC_CHECK(it != P->taps.end(), std::string("unknown tensor '") + name + "'");
  const Buf& b = P->bufs[it->second];
  if (!strcmp(name, "input") && P->fused_stem) {             // the fused stem never writes the network input: build it for the tap
    CC_CHECK(P->last_frames, "no frames to letterbox");
    PreP pp{};
    for (const Op& op : P->ops) if (op.kind == 5) { pp = op.stem.pre; break; }
    pp.frames = P->last_frames; pp.out = P->arena + b.off; pp.out_c = b.C;
    if (P->ragged) launch_preprocess_ragged(h->dtype, pp, P->desc_dev, P->packed_bytes, h->stream);   // the records of the last call are still there
    else launch_preprocess(h->dtype, pp, h->stream);
    CC_HIP(hipStreamSynchronize(h->stream));
  }
  const int C = !strcmp(name, "input") ? 3 : b.C;
  shape[0] = nb; shape[1] = b.H; shape[2] = b.W; shape[3] = C; *ndim = 4;
  if (!out) return 0;
  const size_t frame = (size_t)b.H * b.W * b.C;
  const size_t n = (size_t)nb * frame;
  const size_t es = b.f32 ? 4 : dtype_size(h->dtype);
  std::vector<char> tmp(n * es);
  CC_HIP(hipMemcpy(tmp.data(), P->arena + b.off + (size_t)b0 * frame * es, n * es, hipMemcpyDeviceToHost));
  const size_t px = (size_t)nb * b.H * b.W;
  for (size_t i = 0; i < px; ++i)
    for (int c = 0; c < C; ++c) {
      const size_t j = i * b.C + c;
      float v;
      if (b.f32 || h->dtype == F32) v = ((const float*)tmp.data())[j];
      else if (h->dtype == F16) v = (float)((const f16_t*)tmp.data())[j];
      else v = bf16_bits_to_f32(((const uint16_t*)tmp.data())[j]);
      out[i * C + c] = v;
    }
  CC_API_END
}

int cc_yolo_get_tensor(cc_yolo* h, const char* name, float* out, int64_t* shape, int* ndim) {
  return get_tensor_frames(h, name, 0, -1, out, shape, ndim);
}

int cc_yolo_get_tensor_frames(cc_yolo* h, const char* name, int b0, int nb, float* out, int64_t* shape, int* ndim) {
  if (nb < 0) nb = 0;                                        // a negative count is a bad range here, not "every frame"
  return get_tensor_frames(h, name, b0, nb, out, shape, ndim);
}

int cc_yolo_nonfinite(cc_yolo* h, int* count) {
  CC_API_BEGIN
  CC_CHECK(h && count, "null argument");
  CC_HIP(hipSetDevice(h->device));
  sync_all(h);
  int total = 0;
  for (auto& kv : h->plans.slots) {
    int n = 0; CC_HIP(hipMemcpy(&n, kv.second.plan->nonfinite, 4, hipMemcpyDeviceToHost));
    if (n) CC_HIP(hipMemset(kv.second.plan->nonfinite, 0, 4));
    total += n;
  }
  *count = total;
  CC_API_END
}

int cc_yolo_last_gpu_ms(cc_yolo* h, float* ms) {
  CC_API_BEGIN
  CC_CHECK(h && ms && h->last, "no detect call yet");
  CC_HIP(hipEventSynchronize(h->ev1));
  CC_HIP(hipEventElapsedTime(ms, h->ev0, h->ev1));
  CC_API_END
}

int cc_yolo_profile(cc_yolo* h, int iters, float* ms, double* alg_macs_per_step, int* n_conv_launches) {
  CC_API_BEGIN
  CC_CHECK(h && ms && h->last && iters > 0, "bad argument / no detect call yet");
  Plan* P = h->last;
  CC_CHECK(!P->ragged, "cc_yolo_profile: the last call was a ragged batch - profile the uniform plan of the same network shape");
  CC_HIP(hipSetDevice(h->device));
  sync_all(h);
  hipStream_t s = h->stream;
  const size_t n = P->ops.size();
  std::vector<hipEvent_t> ev(2 * n);
  for (auto& e : ev) CC_HIP(hipEventCreate(&e));
  double acc[5] = {0, 0, 0, 0, 0}, macs = 0; int nconv = 0;
  std::vector<cc::LaunchNote> notes(n, cc::LaunchNote{"", 0, 1});
  if (getenv("CLEARCAM_PROFILE_CSV")) {
    // the launch notes (kernel taken, tiles, slots: an occupancy query per launch) come from an UNTIMED pass of their own, so that
    // no host work sits between the two events of a timed launch (pass 0 carried it and was summed into conv_ms / pool_ms)
    for (size_t i = 0; i < n; ++i) {
      cc::g_note_launches = true;
      cc::g_launch_note = cc::LaunchNote{"", 0, 1};
      launch_op(h->dtype, P, P->ops[i], s, true);
      notes[i] = cc::g_launch_note;
      cc::g_note_launches = false;
    }
    CC_HIP(hipStreamSynchronize(s));
  }
  for (int it = 0; it < iters; ++it) {
    for (size_t i = 0; i < n; ++i) {
      const Op& op = P->ops[i];
      CC_HIP(hipEventRecord(ev[2 * i], s));
      launch_op(h->dtype, P, op, s, true);
      CC_HIP(hipEventRecord(ev[2 * i + 1], s));
    }
    CC_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
      float t = 0; CC_HIP(hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]));
      const int kd = P->ops[i].kind;
      // CBFuse counts with the pools; the fused letterbox + stem has its own slot; a fused RepNCSP is conv work; the fused DDetect tail
      // (last 1x1 convs + decode) is timed in the decode slot, its 0.35 % of the FLOPs stay out of the conv roofline
      acc[kd == 4 ? 1 : (kd == 5 ? 4 : (kd == 6 ? 0 : (kd == 7 ? 2 : kd)))] += t;
    }
  }
  for (const Op& op : P->ops) if (op.kind == 0 || op.kind == 6) { macs += op.alg_macs; ++nconv; }
  if (const char* path = getenv("CLEARCAM_PROFILE_CSV")) {   // per-launch table for tuning
    FILE* f = fopen(path, "w");
    if (f) {
      fprintf(f, "op,kind,ms,M,Cout,Ktot,ks,stride,Cin,alg_gmac,tflops,gbytes_min,gbs,weight_planes,kernel,tiles,slots,rounds,last_round_fill,bound,roof_ms\n");
      // tiles / slots: units of work of the launch and how many the chip takes at once (resident blocks x CUs; the grid of a persistent kernel);
      // rounds = ceil(tiles / slots), last_round_fill = share of the slots the last round uses; bound / roof_ms = the larger of
      // FLOPs / 2.5 PFLOP/s and minimum bytes / 8 TB/s
      auto tail = [&](size_t i, double macs, double bytes) {
        const cc::LaunchNote& ln = notes[i];
        const long rounds = ln.tiles ? (ln.tiles + ln.slots - 1) / ln.slots : 0;
        const double fill = rounds ? (double)(ln.tiles - (rounds - 1) * ln.slots) / (double)ln.slots : 0.0;
        const double tm = 2 * macs / 2.5e15 * 1e3, tb = bytes / 8e12 * 1e3;
        fprintf(f, ",%s,%ld,%ld,%ld,%.3f,%s,%.4f\n", ln.kernel, ln.tiles, ln.slots, rounds, fill, tm > tb ? "mfma" : "hbm", tm > tb ? tm : tb);
      };
      for (size_t i = 0; i < n; ++i) {
        const Op& op = P->ops[i];
        float t = 0; hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]);
        if (op.kind == 0) {
          const ConvP& c = op.conv; const double M = (double)c.B * c.Ho * c.Wo;
          const double es = dtype_size(h->dtype);
          const bool avg = c.s0.shift < 0;                 // reads the 2x2 average of its source (conv_adown.hip)
          const double in0 = avg ? (double)(c.Hin + 1) * (c.Win + 1) : (double)(c.Hin >> c.s0.shift) * (c.Win >> c.s0.shift);
          const double bytes = (double)c.B * in0 * c.s0.C * es + (double)c.B * (c.Hin >> c.s1.shift) * (c.Win >> c.s1.shift) * c.s1.C * es
                             + M * c.Cout * (c.out_f32 ? 4 : es) + (c.res ? M * c.Cout * es : 0) + (double)c.Cout * c.Ktot * es;
          fprintf(f, "%zu,%s,%.4f,%.0f,%d,%d,%d,%d,%d,%.4f,%.1f,%.4f,%.0f,%d", i, avg ? "conv_avg" : "conv", t, M, c.Cout, c.Ktot, c.ks, c.stride, c.Cin,
                  op.alg_macs / 1e9, 2 * op.alg_macs / (t * 1e-3) / 1e12, bytes / 1e9, bytes / (t * 1e-3) / 1e9, 1 + c.split);
          tail(i, op.alg_macs, bytes);
        } else if (op.kind == 1) {
          const PoolP& q = op.pool; const double es = dtype_size(h->dtype);
          const double bytes = ((double)q.B * q.H * q.W + (double)q.B * q.Ho * q.Wo) * q.C * es;
          fprintf(f, "%zu,pool%d_k%d_s%d,%.4f,%.0f,%d,0,%d,%d,%d,0,0,%.4f,%.0f,0", i, q.mode, q.k, q.stride, t, (double)q.B * q.Ho * q.Wo, q.C, q.k, q.stride, q.C,
                  bytes / 1e9, bytes / (t * 1e-3) / 1e9);
          tail(i, 0.0, bytes);
        } else if (op.kind == 5) {
          const StemP& q = op.stem; const double M = (double)q.pre.B * q.Ho * q.Wo, es = dtype_size(h->dtype);
          const double bytes = (double)q.pre.B * q.pre.H * q.pre.W * 3 * (q.pre.frame_f32 ? 4 : 1) + M * q.Cout * es;
          fprintf(f, "%zu,stem_fused,%.4f,%.0f,%d,27,3,2,3,%.4f,%.1f,%.4f,%.0f,%d", i, t, M, q.Cout, op.alg_macs / 1e9, 2 * op.alg_macs / (t * 1e-3) / 1e12,
                  bytes / 1e9, bytes / (t * 1e-3) / 1e9, q.w_lo ? 2 : 1);
          tail(i, op.alg_macs, bytes);
        } else if (op.kind == 6) {
          const CspP& q = op.csp; const double M = (double)q.B * q.H * q.W, es = dtype_size(h->dtype);
          const double bytes = M * 4 * q.hid * es + (double)(8 + 18) * q.hid * q.hid * es;     // x in, out out, the four weight matrices
          fprintf(f, "%zu,csp_fused,%.4f,%.0f,%d,%d,3,1,%d,%.4f,%.1f,%.4f,%.0f,%d", i, t, M, 2 * q.hid, (8 + 18) * q.hid, 2 * q.hid, op.alg_macs / 1e9,
                  2 * op.alg_macs / (t * 1e-3) / 1e12, bytes / 1e9, bytes / (t * 1e-3) / 1e9, q.split ? 2 : 1);
          tail(i, op.alg_macs, bytes);
        } else fprintf(f, "%zu,%s,%.4f,0,0,0,0,0,0,0,0,0,0,0,,0,0,0,0,,0\n", i, op.kind == 2 ? "decode" : (op.kind == 4 ? "cbfuse" : (op.kind == 7 ? "head_tail" : "topk_nms")), t);
      }
      fclose(f);
    }
  }
  for (auto& e : ev) hipEventDestroy(e);
  for (int k = 0; k < 5; ++k) ms[k] = (float)(acc[k] / iters);
  if (alg_macs_per_step) *alg_macs_per_step = macs;
  if (n_conv_launches) *n_conv_launches = nconv;
  CC_API_END
}

int cc_yolo_profile_graph(cc_yolo* h, int iters, int which, float* ms_per_replay) {
  CC_API_BEGIN
  CC_CHECK(h && ms_per_replay && h->last && iters > 0 && which >= 0 && which <= 2, "bad argument / no detect call yet");
  Plan* P = h->last;
  CC_CHECK(!P->ragged, "cc_yolo_profile_graph: the last call was a ragged batch - profile the uniform plan of the same network shape");
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  sync_all(h);
  hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
  CC_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  try {
    for (const Op& op : P->ops) {
      const bool conv = op.kind == 0 || op.kind == 6;
      if (which == 0 ? !conv : (which == 1 ? conv : false)) continue;
      launch_op(h->dtype, P, op, s, true);
    }
  } catch (...) { hipStreamEndCapture(s, &graph); if (graph) hipGraphDestroy(graph); throw; }
  CC_HIP(hipStreamEndCapture(s, &graph));
  CC_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  CC_HIP(hipGraphDestroy(graph));
  for (int i = 0; i < 2; ++i) CC_HIP(hipGraphLaunch(exec, s));          // warm-up
  CC_HIP(hipEventRecord(h->ev0, s));
  for (int i = 0; i < iters; ++i) CC_HIP(hipGraphLaunch(exec, s));
  CC_HIP(hipEventRecord(h->ev1, s));
  CC_HIP(hipEventSynchronize(h->ev1));
  float t = 0; CC_HIP(hipEventElapsedTime(&t, h->ev0, h->ev1));
  CC_HIP(hipGraphExecDestroy(exec));
  *ms_per_replay = t / iters;
  CC_API_END
}

void cc_yolo_destroy(cc_yolo* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (hipStream_t t : h->slot_stream) hipStreamSynchronize(t);
  h->plans.clear();
  for (auto& kv : h->axis_tabs) hipFree(kv.second.lo);
  for (auto& kv : h->packed) { hipFree(kv.second.w); hipFree(kv.second.bias); }
  if (h->dfl_w) hipFree(h->dfl_w);
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->nonfinite_host) hipHostFree(h->nonfinite_host);
  for (hipStream_t t : h->side) pool_stream_put(h->device, t);              // parked, never destroyed (kernels.h)
  for (hipStream_t t : h->slot_stream) pool_stream_put(h->device, t);
  for (hipEvent_t e : h->slot_done) hipEventDestroy(e);
  pool_stream_put(h->device, h->stream);
  delete h;
}

int cc_conv2d_nhwc(int dtype, const void* x_dev, int B, int H, int W, int Cin, const float* w_oihw, const float* bias,
                   int Cout, int k, int stride, int groups, int act, void* out_dev, int force_direct, void* stream) {
  CC_API_BEGIN
  CC_CHECK(x_dev && w_oihw && out_dev && groups >= 1 && Cin % groups == 0 && Cout % groups == 0, "bad argument");
  HostTensor w, b;
  w.shape = {Cout, Cin / groups, k, k};
  w.data.assign(w_oihw, w_oihw + (size_t)Cout * (Cin / groups) * k * k);
  if (bias) { b.shape = {Cout}; b.data.assign(bias, bias + Cout); }
  const int split = dtype == F16S;                       // dtype 3: f16 storage, split weights
  dtype = storage_dtype(dtype);
  PackedConv pc = pack_convs(dtype, {&w}, {bias ? &b : nullptr}, {groups}, 0, split);
  ConvP c{};
  c.s0 = Src{x_dev, H, W, Cin, 0, Cin, 0}; c.s1 = Src{x_dev, 1, 1, 0, 0, 0, 0};
  c.B = B; c.Hin = H; c.Win = W; c.Cin = Cin; c.ks = k; c.stride = stride; c.pad = k / 2;
  c.Ho = (H + 2 * c.pad - k) / stride + 1; c.Wo = (W + 2 * c.pad - k) / stride + 1; c.Cout = Cout; c.Ktot = k * k * Cin * (1 + split); c.Kw = pc.kw;
  c.split = pc.split; c.oscale = pc.oscale;
  c.w = pc.w; c.bias = pc.bias; c.out = out_dev; c.out_cstride = Cout; c.out_coff = 0; c.out_f32 = 0; c.res = nullptr; c.act = act;
  c.variant = force_direct;                              // ConvVariant (conv_select.h): 0 auto, 1 direct, 2 generic MFMA, ...
  launch_conv(dtype, c, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  hipFree(pc.w); hipFree(pc.bias);
  CC_API_END
}

// Diagnostic: average device time of one attention launch over random 16-bit data (kernel tuning; abl as AttnP::abl).
int cc_attn_bench(int dtype, int B, int L, int H, int causal, int abl, int iters, float* ms) {
  CC_API_BEGIN
  CC_CHECK(ms && iters > 0 && (dtype == F16 || dtype == BF16) && B > 0 && L > 0 && H > 0, "bad argument");
  const int D = H * 64;
  const size_t nq = (size_t)B * L * 3 * D, no = (size_t)B * L * D;
  std::vector<float> hx(std::min<size_t>(nq, (size_t)1 << 22));
  uint32_t st = 777u;
  for (auto& v : hx) { st = st * 1664525u + 1013904223u; v = ((st >> 8) & 0xffff) / 65536.0f - 0.5f; }
  std::vector<char> h16(hx.size() * 2);
  convert_f32_to(dtype, hx.data(), h16.data(), hx.size());
  char *qkv = nullptr, *ctx = nullptr;
  CC_HIP(hipMalloc((void**)&qkv, nq * 2 + 256)); CC_HIP(hipMalloc((void**)&ctx, no * 2 + 256));
  for (size_t off = 0; off < nq * 2; off += h16.size()) CC_HIP(hipMemcpy(qkv + off, h16.data(), std::min(h16.size(), nq * 2 - off), hipMemcpyHostToDevice));
  AttnP a{}; a.qkv = qkv; a.ctx = ctx; a.B = B; a.L = L; a.H = H; a.D = D; a.causal = causal; a.scale = 0.125f; a.abl = abl;
  hipStream_t s; CC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipEvent_t e0, e1; CC_HIP(hipEventCreate(&e0)); CC_HIP(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) launch_attention(dtype, a, s);
  CC_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) launch_attention(dtype, a, s);
  CC_HIP(hipEventRecord(e1, s));
  CC_HIP(hipStreamSynchronize(s));
  float t = 0; CC_HIP(hipEventElapsedTime(&t, e0, e1));
  *ms = t / iters;
  hipEventDestroy(e0); hipEventDestroy(e1); hipStreamDestroy(s);
  hipFree(qkv); hipFree(ctx);
  CC_API_END
}

int cc_round_weights(int dtype, const float* w, int64_t cout, int64_t cin, int64_t k, float* out) {
  CC_API_BEGIN
  CC_CHECK(w && out && cout >= 0 && cin >= 0 && k >= 1 && (dtype == F16 || dtype == BF16), "bad argument (dtype 1 = f16 or 2 = bf16)");
  const std::vector<float> q = round_controlled(dtype, w, (size_t)cout, (size_t)cin, (size_t)k);
  memcpy(out, q.data(), q.size() * sizeof(float));
  CC_API_END
}

int cc_dev_set(const char* key, int value) {
  CC_API_BEGIN
  CC_CHECK(key, "null key");
  if (std::string(key) == "phase_flags") cc::g_phase_flags_override = value;
  else if (std::string(key) == "stream") cc::g_stream_override = value;
  else if (std::string(key) == "stream_abl") cc::g_stream_abl = value;
  else if (std::string(key) == "stream_flags") cc::g_stream_flags_override = value;
  else if (std::string(key) == "tile64_abl") cc::g_tile64_abl = value;
  else if (std::string(key) == "tile64_w") cc::g_tile64_w_override = value;
  else throw cc::Error(-22, std::string("cc_dev_set: unknown key ") + key);
  CC_API_END
}

// Diagnostic: average device time of ONE conv launch (random bf16/f16 data resident in HBM, weights packed once), hipEvents
// on a private stream around `iters` back-to-back launches after 3 warm-up launches.  variant as ConvP::variant.
int cc_conv_bench(int dtype, int B, int H, int W, int Cin, int Cout, int k, int stride, int act, int variant, int iters, float* ms) {
  CC_API_BEGIN
  CC_CHECK(ms && iters > 0 && (dtype == F16 || dtype == BF16 || dtype == F16S), "bad argument");
  const int split = dtype == F16S;
  dtype = storage_dtype(dtype);
  HostTensor w, b;
  w.shape = {Cout, Cin, k, k};
  w.data.resize((size_t)Cout * Cin * k * k);
  uint32_t st = 12345u;
  auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 65536.0f - 0.5f; };
  const float sc = 2.0f / sqrtf((float)Cin * k * k);
  for (auto& v : w.data) v = rnd() * sc;
  b.shape = {Cout}; b.data.assign(Cout, 0.01f);
  PackedConv pc = pack_convs(dtype, {&w}, {&b}, {1}, 0, split);
  const int pad = k / 2, Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const size_t nin = (size_t)B * H * W * Cin, nout = (size_t)B * Ho * Wo * Cout;
  std::vector<float> hx(std::min<size_t>(nin, (size_t)1 << 24));
  for (auto& v : hx) v = rnd() * 2.0f;
  std::vector<char> hx16(hx.size() * 2);
  convert_f32_to(dtype, hx.data(), hx16.data(), hx.size());
  char *x = nullptr, *out = nullptr;
  CC_HIP(hipMalloc((void**)&x, nin * 2 + 256)); CC_HIP(hipMalloc((void**)&out, nout * 2 + 256));
  for (size_t off = 0; off < nin * 2; off += hx16.size()) CC_HIP(hipMemcpy(x + off, hx16.data(), std::min(hx16.size(), nin * 2 - off), hipMemcpyHostToDevice));
  ConvP c{};
  c.s0 = Src{x, H, W, Cin, 0, Cin, 0}; c.s1 = Src{x, 1, 1, 0, 0, 0, 0};
  c.B = B; c.Hin = H; c.Win = W; c.Cin = Cin; c.ks = k; c.stride = stride; c.pad = pad; c.Ho = Ho; c.Wo = Wo; c.Cout = Cout;
  c.Ktot = k * k * Cin * (1 + split); c.Kw = pc.kw; c.split = pc.split; c.oscale = pc.oscale; c.w = pc.w; c.bias = pc.bias; c.out = out; c.out_cstride = Cout; c.act = act; c.variant = variant;
  hipStream_t s; CC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipEvent_t e0, e1; CC_HIP(hipEventCreate(&e0)); CC_HIP(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) launch_conv(dtype, c, s);
  CC_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) launch_conv(dtype, c, s);
  CC_HIP(hipEventRecord(e1, s));
  CC_HIP(hipStreamSynchronize(s));
  float t = 0; CC_HIP(hipEventElapsedTime(&t, e0, e1));
  *ms = t / iters;
  if (const char* e = getenv("CLEARCAM_BENCH_DUMP")) {   // dev: the 256 slack bytes behind the output (a kernel's timing ablation may leave cycle counts there)
    unsigned long long v[32] = {};
    (void)e;
    CC_HIP(hipMemcpy(v, out + nout * 2, sizeof(v), hipMemcpyDeviceToHost));
    for (int i = 0; i < 32; ++i) fprintf(stderr, "%llu%c", v[i], (i & 3) == 3 ? '\n' : ' ');
  }
  hipEventDestroy(e0); hipEventDestroy(e1); hipStreamDestroy(s);
  hipFree(x); hipFree(out); hipFree(pc.w); hipFree(pc.bias);
  CC_API_END
}

}  // extern "C"
