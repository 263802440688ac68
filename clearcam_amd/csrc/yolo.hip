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
#include <cmath>
#include <cstring>
#include "conv_select.h"
#include "yolo_plan.h"

using namespace cc;

namespace cc {

// detection/yolov9.py:461-464 (SIZES) by role; same table as clearcam_amd/arch.py.
static const Arch kArch[] = {
    {"t", 16, true, 32, 32, false, 64, 16, 64, 64, 96, 24, 96, 128, 32, 128, 64, 48, 64, 80, 3},
    {"s", 32, true, 64, 64, false, 128, 32, 128, 128, 192, 48, 192, 256, 64, 256, 128, 96, 128, 128, 3},
    {"m", 32, false, 32, 128, false, 240, 60, 240, 240, 360, 90, 360, 480, 120, 480, 240, 184, 240, 240, 1},
    {"c", 64, false, 32, 256, true, 256, 64, 256, 512, 512, 128, 512, 512, 128, 512, 256, 256, 512, 256, 1},
    // "e" (yolov9.py:328-371) has its own 43-block builder; only adown / cls_hidden / rep_n are read from this row
    {"e", 64, false, 32, 256, true, 0, 0, 256, 0, 0, 0, 512, 0, 0, 512, 256, 0, 0, 256, 2},
};

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
PackedConv pack_convs(int dt, const std::vector<const HostTensor*>& ws, const std::vector<const HostTensor*>& bs,
                      const std::vector<int>& groups, int cin_pad, int split) {
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

// The environment switches that shape a plan (docs/env_switches.md; each is described where the Builder uses it), read once per plan
// build: the plan-level twin of conv_switches().  The three CSP development switches are honoured only under CLEARCAM_DEV=1.
struct PlanSwitches {
  static int num(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
  static bool set(const char* name) { return getenv(name) != nullptr; }
  const int lanes = num("CLEARCAM_LANES", 0), fuse_csp = num("CLEARCAM_FUSE_CSP", 2);
  const bool fuse_stem = num("CLEARCAM_FUSE_STEM", 1) != 0, fuse_adown = num("CLEARCAM_FUSE_ADOWN", 0) != 0, fuse_head = num("CLEARCAM_FUSE_HEAD", 1) != 0;
  const bool head_split = num("CLEARCAM_HEAD_SPLIT", 1) != 0, arena_reuse = num("CLEARCAM_ARENA_REUSE", 1) != 0;
  const bool tap_csp = set("CLEARCAM_TAP_CSP"), tap_stem = set("CLEARCAM_TAP_STEM"), tap_blocks = set("CLEARCAM_TAP_BLOCKS"), verbose = set("CLEARCAM_VERBOSE");
  const bool dev = num("CLEARCAM_DEV", 0) != 0;
  const bool csp_only_set = dev && set("CLEARCAM_CSP_ONLY");            // fuse just the RepNCSP with index csp_only (csp_debug.py)
  const int csp_only = dev ? num("CLEARCAM_CSP_ONLY", 0) : 0, csp_dbg = dev ? num("CLEARCAM_CSP_DBG", 0) : 0, csp_stream = dev ? num("CLEARCAM_CSP_STREAM", 0) : 0;
};

struct Builder {
  cc_yolo* Y; Plan* P; const Arch& a; const PlanSwitches sw;
  Builder(cc_yolo* y, Plan* p) : Y(y), P(p), a(*y->arch) {}

  int cur_lane = 0;
  // Which independent chains leave the trunk (CLEARCAM_LANES, sw.lanes, read per plan): bit 1 = each DDetect level on its own lane (2-4), bit 2 =
  // the three levels share lane 2, bit 0 = ADown's pooled half on lane 1.  OFF by default.  Measured with nothing else on the GPU:
  // DDetect lanes B = 64: 11.39 -> 11.24 ms, B = 16: 3.75 -> 3.67 (P3's 3x3 convs fill the CUs the neck's 40x40 / 20x20 launches
  // leave idle); a graph with branches costs ~50 us per replay (B = 8: 2.35 -> 2.39 ms, one frame 1.30 -> 1.35); ADown's halves gain
  // nothing (both open with a bandwidth-bound pool); profiles/r03o_lanes_ab*.txt.  But the runtime replays the branches on
  // internal streams that share its few hardware queues with every other stream of the process, and inside a camera pipeline
  // (upload, download and caller streams) a branch that lands behind another stream's barrier costs far more than the lanes gain
  // (64 x 1080p cameras, frames resident: 6.1 k frames/s with lanes against 8.5-9 k without, profiles/r03s_*).  Batches in flight
  // (cc_yolo_submit, slots on probed queues) are the robust way to fill those CUs.  Outputs are bit-identical either way.
  struct Lane {                                            // scope guard: launches pushed inside run on lane `l`
    Builder& b; int saved;
    Lane(Builder& b_, int l) : b(b_), saved(b_.cur_lane) {
      const int m = b.sw.lanes;
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
    Op op{}; op.kind = Conv; ConvP& c = op.conv;
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
    return sw.fuse_stem && Y->cin_pad() == 8 && stem_fused_supported(Y->dtype, cout);
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
    Op op{}; op.kind = Stem; StemP& q = op.stem;
    const Buf& ob = P->bufs[out.buf];
    CC_CHECK(pc.k == 3 && pc.cin == 8 && ob.H == P->Hn / 2 && ob.W == P->Wn / 2 && out.C == pc.cout, "fused stem: shape mismatch");
    q.pre = plan_prep(P);                                                      // as cc_yolo_detect's preprocess launch; frames set per call (run_stems)
    q.w = stem_weights(name, pc); q.bias = pc.bias; q.Cout = pc.cout;
    q.w_lo = pc.split ? stem_weights(name, pc, 1) : nullptr; q.oscale = pc.oscale;
    q.out = (void*)(intptr_t)out.buf; q.out_cstride = ob.C; q.out_coff = out.coff; q.Ho = ob.H; q.Wo = ob.W;
    op.alg_macs = (double)P->B * ob.H * ob.W * pc.macs_px;
    push(op, {wr(out)});
    P->fused_stem = true;
  }

  void pool(View in, View out, int k, int stride, int pad, int mode) {
    Op op{}; op.kind = Pool; PoolP& q = op.pool;
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
  // Round 6: at hidden width 64 the layer-at-a-time path has caught up wherever conv_tile64.hip takes the block's two 3x3 64 -> 64 convs (one round of its
  // 8 x 32 tiles: B >= 11 at 80x80, unsplit 3x3 weights) - whole step, B = 64, f16h, twice each: 6582 / 6582 frames/s against 6531 / 6452 fused
  // (profiles/r06x_fuse_csp.txt).  Level 2 (default) therefore fuses hidden 64 only below that; 3 = always (the round-2..5 behaviour).  Both forms
  // produce the same bits (test_fused_csp_equals_unfused), so the choice may depend on the batch.
  bool fuse_csp(View in, int hid, int index, const std::string& r) {
    const int level = sw.fuse_csp;
    if (level == 0 || (level == 1 && hid != 32)) return false;
    if (level == 2 && hid == 64 && !pconv({r + ".m.list.0.cv1.conv"}, {1}).split) {
      const Buf& ib = P->bufs[in.buf];
      if (conv_tile64_takes(P->B, ib.H, ib.W)) return false;
    }
    if (sw.csp_only_set && sw.csp_only != index) return false;      // development: fuse just this block (csp_debug.py)
    if (!(a.rep_n == 1 && csp_fused_supported(Y->dtype, hid, Y->wsplit) && in.C == 2 * hid && in.coff % 8 == 0 && P->bufs[in.buf].C % 8 == 0)) return false;
    // the fused kernel knows three split patterns: none, all four convs ("f16s"), the two 1x1 launches only ("f16h" in the backbone)
    const int s12 = pconv({r + ".cv1.conv", r + ".cv2.conv"}, {1, 1}).split, s3 = pconv({r + ".cv3.conv"}, {1}).split;
    const int sr = pconv({r + ".m.list.0.cv1.conv"}, {1}).split, sb = pconv({r + ".m.list.0.cv2.conv"}, {1}).split;
    return s12 == s3 && sr == sb && (sr == s12 || (s12 && !sr));
  }
  void csp_fused(const std::string& r, View in, View out, int hid) {
    Op op{}; op.kind = Csp; CspP& q = op.csp;
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
    q.dbg = sw.csp_dbg; q.stream = sw.csp_stream;                   // development (PlanSwitches)
    op.alg_macs = (double)P->B * ib.H * ib.W * (c12.macs_px + cr.macs_px + cb.macs_px + c3.macs_px);
    push(op, {rd(in), wr(out)});
  }

  // RepNCSP (:92-105) + trailing 3x3 Conv (:112,115): in -> out
  int n_csp = 0;
  void csp_branch(const std::string& p, View in, View out, int hid) {
    const int H = P->bufs[in.buf].H, W = P->bufs[in.buf].W;
    const std::string r = p + ".list.0";
    const bool tap = sw.tap_csp;                                     // tests: keep the block's tensors readable (costs arena)
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
    if (sw.tap_csp) P->taps["cat" + std::to_string(n_csp / 2)] = cat;     // tests: [y0 | y1 | y2 | y3] of the n-th RepNCSPELAN4
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
    if (!sw.fuse_adown || Y->wsplit) return false;
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
    Op op{}; op.kind = Fuse; FuseP& f = op.fuse;
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
    return sw.fuse_head && head_tail_supported(Y->dtype, a.cls_hidden, Y->wsplit);
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
    if (head_levels++ == 0) { head_dec = Op{}; head_dec.kind = Decode; head_tail = Op{}; head_tail.kind = HeadTail; head_acc.clear(); P->A = 0; }
    const std::string hb = H22 + "cv2.list." + std::to_string(l) + ".list.", hc = H22 + "cv3.list." + std::to_string(l) + ".list.";
    const int H = P->bufs[feat.buf].H, W = P->bufs[feat.buf].W, ch = a.cls_hidden;
    const int hbuf = new_buf(H, W, 64 + ch), bxb = new_buf(H, W, 64), clb = new_buf(H, W, ch);
    // The level's two entry convs (box: feat -> 64, class: feat -> ch; yolov9.py:205-206) read the same map.  As ONE 64 + ch channel GEMM
    // the input is read once - but 64 + 256 = 320 channels do not tile by 256, so the whole launch falls back to five 64-wide channel
    // tiles that each pull the activations again.  With ch a multiple of 256 the class conv alone takes the eight-wave 256-wide
    // kernel and the 64-channel box conv a launch of its own (cc_conv_bench, B = 64: 3x3 256 -> 320 at 80x80 857 us against 535 + 206,
    // split weights 1495 against 935 + 399; profiles/r04c_head_split.txt).  Same K order per channel: the same bits either way.
    // CLEARCAM_HEAD_SPLIT=0 keeps the single launch.
    if (sw.head_split && Y->dtype != F32 && ch % 256 == 0) {
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
    Op nms{}; nms.kind = Nms;
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
    if (sw.tap_stem) P->taps["stem"] = b0;       // tests: keep the first conv's output readable (costs arena)
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
    if (sw.tap_blocks) {                         // development: every block's output readable ("b<block>": the WHOLE buffer the
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
    if (!sw.arena_reuse) return;
    const int nb = (int)P->bufs.size(), nops = (int)P->ops.size();
    std::vector<int> first(nb, nops + 1), last(nb, -2);
    for (int t = 0; t < nops; ++t) {                           // every tensor a launch touches is in its access list (push)
      const Op& op = P->ops[t];
      const int when = op.kind == Stem ? -1 : t;               // the fused stem runs before the graph, whatever its position in the list
      for (const Op::Access& x : op.acc) if (x.buf >= 0) { first[x.buf] = std::min(first[x.buf], when); last[x.buf] = std::max(last[x.buf], when); }
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
    if (sw.verbose)
      fprintf(stderr, "[clearcam] plan B=%d %dx%d: %d tensors, %.2f GB unpacked -> %.2f GB arena\n", P->B, P->Hn, P->Wn, nb,
              (double)P->arena_bytes / 1e9, (double)top / 1e9);
    P->arena_bytes = top;
  }

  // Buffer ids become arena addresses.  The typed pointer fields below are the ONE place that still knows which fields of an op are
  // tensors; lifetimes (pack_arena) and conflicts (ops_conflict) go by Op::acc.
  void resolve() {
    pack_arena();
    CC_HIP(hipMalloc((void**)&P->arena, P->arena_bytes));
    CC_HIP(hipMemset(P->arena, 0, P->arena_bytes));
    CC_HIP(hipMalloc((void**)&P->det, (size_t)P->B * P->A * 6 * 4));
    CC_HIP(hipMalloc((void**)&P->out_dev, (size_t)P->B * CC_MAX_DET * 6 * 4));
    CC_HIP(hipMalloc((void**)&P->nonfinite, 256)); CC_HIP(hipMemset(P->nonfinite, 0, 256));
    auto ptr = [&](const void* id) -> char* { const intptr_t i = (intptr_t)id; return i < 0 ? nullptr : P->arena + P->bufs[i].off; };
    for (Op& op : P->ops) {
      if (op.kind == Conv) {
        op.conv.s0.ptr = ptr(op.conv.s0.ptr); op.conv.s1.ptr = ptr(op.conv.s1.ptr);
        if (!op.conv.s1.ptr) op.conv.s1.ptr = op.conv.s0.ptr;
        op.conv.out = ptr(op.conv.out); op.conv.res = ptr(op.conv.res);
      } else if (op.kind == Pool) { op.pool.in = ptr(op.pool.in); op.pool.out = ptr(op.pool.out); }
      else if (op.kind == Decode) { for (int l = 0; l < 3; ++l) op.dec.raw[l] = (const float*)ptr(op.dec.raw[l]); op.dec.det = P->det; op.dec.nonfinite = P->nonfinite; }
      else if (op.kind == Fuse) { for (int k = 0; k < op.fuse.n; ++k) op.fuse.in[k] = ptr(op.fuse.in[k]); op.fuse.out = ptr(op.fuse.out); }
      else if (op.kind == Stem) op.stem.out = ptr(op.stem.out);
      else if (op.kind == Csp) { op.csp.x = ptr(op.csp.x); op.csp.out = ptr(op.csp.out); }
      else if (op.kind == HeadTail) { for (int l = 0; l < 3; ++l) { op.tail.bx[l] = ptr(op.tail.bx[l]); op.tail.cl[l] = ptr(op.tail.cl[l]); } op.tail.det = P->det; op.tail.nonfinite = P->nonfinite; }
      else { op.nms.det = P->det; op.nms.out = P->out_dev; }
    }
  }
};

void build_plan(cc_yolo* Y, Plan* P) { Builder bld(Y, P); bld.build(); bld.resolve(); }

}  // namespace cc

extern "C" {

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

int cc_round_weights(int dtype, const float* w, int64_t cout, int64_t cin, int64_t k, float* out) {
  CC_API_BEGIN
  CC_CHECK(w && out && cout >= 0 && cin >= 0 && k >= 1 && (dtype == F16 || dtype == BF16), "bad argument (dtype 1 = f16 or 2 = bf16)");
  const std::vector<float> q = round_controlled(dtype, w, (size_t)cout, (size_t)cin, (size_t)k);
  memcpy(out, q.data(), q.size() * sizeof(float));
  CC_API_END
}

}  // extern "C"
