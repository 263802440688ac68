// Development entries that run ONE launch of a multi-stage kernel that keeps its intermediates on chip, outside any plan, on inputs the
// caller crafts: cc_dev_csp / cc_dev_csp_choice (launch_csp_fused: csp_fused_kernel resident or streamed, csp_tile_kernel, and the
// selection rule choose_csp) and cc_dev_stem (launch_stem_fused / launch_stem_fused_ragged: letterbox + first conv from frames).  Each
// validates every argument before the first HIP call - whatever a launcher would refuse is refused here, with its text behind
// cc_last_error, so the refusals can be tested without a device - packs the weights with the detector's own packers (pack_convs,
// stem_pack_weights), builds geometry, axis tables and frame records with the functions the plans use (yolo_run.hip), calls the
// production launcher once, synchronises the stream and frees what it packed.
#include <memory>
#include "conv_select.h"
#include "yolo_plan.h"

using namespace cc;

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
constexpr long kMaxElems = 1L << 30;                     // elements of one buffer: every index the kernels form stays inside int / 32-bit byte offsets

// device memory of one call, freed on every way out
struct Owner {
  std::vector<void*> mem;
  ~Owner() { for (void* p : mem) if (p) hipFree(p); }
  void* alloc(size_t bytes) { void* p = nullptr; CC_HIP(hipMalloc(&p, bytes)); mem.push_back(p); return p; }
  template <class T> T* upload(const std::vector<T>& v) {
    T* d = (T*)alloc(v.size() * sizeof(T) + 16);
    CC_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  PackedConv keep(PackedConv pc) { mem.push_back(pc.w); mem.push_back(pc.bias); return pc; }
};

// ---- RepNCSP -------------------------------------------------------------------------------------------------------------------------
enum { V_AUTO = 0, V_FUSED = 1, V_STREAM = 2, V_TILE = 3, V_LAYERS = 4 };

// What both CSP entries check (no pointer, no HIP call); returns the tile mode the launch runs under and sets `stream`.
int csp_check(int dtype, int split, int hid, int B, int H, int W, int variant, int dbg, int& stream) {
  CC_CHECK(dtype == F16 || dtype == BF16, "storage dtype must be 1 (f16) or 2 (bf16)");
  CC_CHECK(split >= 0 && split <= 2, "split is 0 (one plane), 1 (two planes everywhere) or 2 (two planes in the 1x1 convs)");
  CC_CHECK(hid == 32 || hid == 64, "hidden width must be 32 or 64");
  CC_CHECK(csp_fused_supported(dtype, hid, split), "split weights need f16 storage");
  CC_CHECK(B > 0 && H > 0 && W > 0, "bad shape");
  CC_CHECK(variant >= V_AUTO && variant <= V_LAYERS && dbg >= 0 && dbg <= 3, "variant is 0 .. 4, dbg 0 .. 3");
  CC_CHECK((long)B * ((H + 7) / 8) * ((W + 15) / 16) < (1L << 22), "too many tiles");
  stream = variant == V_STREAM;
  const int mode = variant == V_AUTO ? csp_tile_mode() : variant == V_TILE ? 2 : 0;
  if (variant == V_TILE) {
    CC_CHECK(!dbg, "csp_tile_kernel has no dbg dumps");
    CC_CHECK(choose_csp(dtype, hid, split, B, H, W, 0, 0, 2) == CSP_TILE, "csp_tile_kernel: hidden width 32, one weight plane or two in the 1x1 convs");
  }
  return mode;
}

// the tile mode of one launch: cc_dev_set("csp_tile") for its duration, the previous value back afterwards
struct TileMode {
  int saved;
  explicit TileMode(int mode) : saved(g_csp_tile_override.exchange(mode)) {}
  ~TileMode() { g_csp_tile_override = saved; }
};

HostTensor host_tensor(const float* p, std::vector<int64_t> shape) {
  HostTensor t; t.shape = std::move(shape);
  size_t n = 1; for (int64_t d : t.shape) n *= (size_t)d;
  t.data.assign(p, p + n);
  return t;
}

// one launch of the layer-at-a-time path (Builder::conv): 3x3 or 1x1, stride 1, bias + SiLU, optional 16-bit residual
ConvP layer(const PackedConv& pc, int B, int H, int W, const void* in, int in_cs, int in_coff, void* out, int out_cs, int out_coff,
            const void* res = nullptr, int res_cs = 0, int res_coff = 0) {
  ConvP c{};
  c.s0 = Src{in, H, W, in_cs, in_coff, pc.cin, 0}; c.s1 = Src{in, 1, 1, 0, 0, 0, 0};
  c.B = B; c.Hin = H; c.Win = W; c.Cin = pc.cin; c.Ho = H; c.Wo = W; c.Cout = pc.cout; c.ks = pc.k; c.stride = 1; c.pad = pc.k / 2;
  c.Ktot = c.ks * c.ks * c.Cin * (pc.split ? 2 : 1); c.Kw = pc.kw; c.split = pc.split; c.oscale = pc.oscale;
  c.w = pc.w; c.bias = pc.bias; c.out = out; c.out_cstride = out_cs; c.out_coff = out_coff; c.act = 1;
  c.res = res; c.res_cstride = res_cs; c.res_coff = res_coff;
  return c;
}

}  // namespace

extern "C" {

int cc_dev_csp_choice(int dtype, int split, int hid, int B, int H, int W, int variant, int dbg, int* choice) {
  CC_API_BEGIN
  CC_CHECK(choice, "null argument");
  int stream = 0;
  const int mode = csp_check(dtype, split, hid, B, H, W, variant, dbg, stream);
  *choice = variant == V_LAYERS ? CC_DEV_CSP_LAYERS : (int)choose_csp(dtype, hid, split, B, H, W, stream, dbg, mode);
  CC_API_END
}

int cc_dev_csp(int dtype, int split, int hid, const void* x_dev, int x_cstride, int x_coff, void* out_dev, int out_cstride, int out_coff,
               int B, int H, int W, const float* const* w, const float* const* bias, int variant, int dbg, int* choice, void* stream) {
  CC_API_BEGIN
  int strm = 0;
  const int mode = csp_check(dtype, split, hid, B, H, W, variant, dbg, strm);
  CC_CHECK(x_dev && out_dev && w && bias, "null argument");
  for (int i = 0; i < 5; ++i) CC_CHECK(w[i] && bias[i], "five convs with biases: cv1, cv2, m.0.cv1 (folded 3x3), m.0.cv2, cv3");
  const int C2 = 2 * hid;
  CC_CHECK(aligned16(x_dev) && aligned16(out_dev) && x_cstride % 8 == 0 && x_coff % 8 == 0 && out_cstride % 8 == 0 && out_coff % 8 == 0,
           "views must be 16-byte aligned: pointers, channel strides and offsets whole 16-byte chunks");
  CC_CHECK(x_coff >= 0 && x_coff + C2 <= x_cstride && out_coff >= 0 && out_coff + C2 <= out_cstride, "bad channel view");
  CC_CHECK((long)B * H * W * x_cstride < kMaxElems && (long)B * H * W * out_cstride < kMaxElems, "tensor too large");
  hipStream_t s = (hipStream_t)stream;
  Owner own;
  const HostTensor w1 = host_tensor(w[0], {hid, C2, 1, 1}), w2 = host_tensor(w[1], {hid, C2, 1, 1}), wr = host_tensor(w[2], {hid, hid, 3, 3}),
                   wb = host_tensor(w[3], {hid, hid, 3, 3}), w3 = host_tensor(w[4], {C2, C2, 1, 1});
  const HostTensor b1 = host_tensor(bias[0], {hid}), b2 = host_tensor(bias[1], {hid}), br = host_tensor(bias[2], {hid}), bb = host_tensor(bias[3], {hid}),
                   b3 = host_tensor(bias[4], {C2});
  // as Builder::csp_fused finds them packed: cv1 | cv2 together, two planes in the 1x1 convs for split 1 / 2, in the 3x3 convs for split 1
  const int s1 = split != 0, s3 = split == 1;
  const PackedConv c12 = own.keep(pack_convs(dtype, {&w1, &w2}, {&b1, &b2}, {1, 1}, 0, s1)), cr = own.keep(pack_convs(dtype, {&wr}, {&br}, {1}, 0, s3)),
                   cb = own.keep(pack_convs(dtype, {&wb}, {&bb}, {1}, 0, s3)), c3 = own.keep(pack_convs(dtype, {&w3}, {&b3}, {1}, 0, s1));
  CC_CHECK(c12.cin == C2 && c12.cout == C2 && cr.cin == hid && cr.cout == hid && cb.cin == hid && cb.cout == hid && c3.cin == C2 && c3.cout == C2,
           "unexpected weight layout");
  if (variant == V_LAYERS) {
    // The four launches the kernel replaces (Builder::csp_branch), on the same packed weights: [a | b], t, u in place over a, out.
    // dbg 1 .. 3 stop where the fused kernel's dumps do and leave [a | b], t or [u | b] in the output view.
    const size_t px = (size_t)B * H * W, es = dtype_size(dtype);
    const bool ab_out = dbg == 1 || dbg == 3;
    void* ab = ab_out ? out_dev : own.alloc(px * C2 * es + 256);
    const int ab_cs = ab_out ? out_cstride : C2, ab_co = ab_out ? out_coff : 0;
    void* t = dbg == 2 ? out_dev : own.alloc(px * hid * es + 256);
    const int t_cs = dbg == 2 ? out_cstride : hid, t_co = dbg == 2 ? out_coff : 0;
    launch_conv(dtype, layer(c12, B, H, W, x_dev, x_cstride, x_coff, ab, ab_cs, ab_co), s);
    if (dbg != 1) launch_conv(dtype, layer(cr, B, H, W, ab, ab_cs, ab_co, t, t_cs, t_co), s);
    if (dbg == 0 || dbg == 3) launch_conv(dtype, layer(cb, B, H, W, t, t_cs, t_co, ab, ab_cs, ab_co, ab, ab_cs, ab_co), s);
    if (dbg == 0) launch_conv(dtype, layer(c3, B, H, W, ab, ab_cs, ab_co, out_dev, out_cstride, out_coff), s);
    CC_HIP(hipStreamSynchronize(s));
    if (choice) *choice = CC_DEV_CSP_LAYERS;
    return 0;
  }
  CspP q{};
  q.x = x_dev; q.x_cstride = x_cstride; q.x_coff = x_coff; q.out = out_dev; q.out_cstride = out_cstride; q.out_coff = out_coff;
  q.w12 = c12.w; q.kw12 = c12.kw; q.b12 = c12.bias; q.wr = cr.w; q.kwr = cr.kw; q.br = cr.bias;
  q.wb = cb.w; q.kwb = cb.kw; q.bb = cb.bias; q.w3 = c3.w; q.kw3 = c3.kw; q.b3 = c3.bias;
  q.B = B; q.H = H; q.W = W; q.hid = hid;
  q.split = !c12.split ? 0 : (cr.split ? 1 : 2); q.os12 = c12.oscale; q.osr = cr.oscale; q.osb = cb.oscale; q.os3 = c3.oscale;
  q.dbg = dbg; q.stream = strm;
  CspKernel ran = CSP_FUSED_RESIDENT;
  {
    std::unique_ptr<TileMode> forced;
    if (variant != V_AUTO) forced.reset(new TileMode(mode));
    launch_csp_fused(dtype, q, s, &ran);
  }
  CC_HIP(hipStreamSynchronize(s));
  if (choice) *choice = (int)ran;
  CC_API_END
}

int cc_dev_stem(int dtype, int split, const void* frames_dev, int frame_f32, const int64_t* offsets, const int32_t* heights, const int32_t* widths,
                int B, int res, int ragged, const float* w_oihw, const float* bias, int Cout, void* out_dev, int out_cstride, int out_coff,
                int* info, void* stream) {
  CC_API_BEGIN
  CC_CHECK(dtype == F16 || dtype == BF16, "storage dtype must be 1 (f16) or 2 (bf16)");
  CC_CHECK(split == 0 || (split == 1 && dtype == F16), "split weights (two f16 planes) need f16 storage");
  CC_CHECK(stem_fused_supported(dtype, Cout), "fused stem: Cout must be 16, 32 or 64");
  CC_CHECK(frames_dev && offsets && heights && widths && w_oihw && bias && out_dev, "null argument");
  CC_CHECK(B > 0 && res > 0, "empty batch / bad resolution");
  CC_CHECK(aligned16(out_dev) && out_cstride % 8 == 0 && out_coff % 8 == 0 && out_coff >= 0 && out_coff + Cout <= out_cstride, "bad output view");
  CC_CHECK(!frame_f32 || (reinterpret_cast<uintptr_t>(frames_dev) & 3u) == 0, "float32 frames must be 4-byte aligned");
  // geometry exactly as the plans compute and check it: one network shape, a multiple of 32
  std::vector<LetterboxGeo> geo;
  int Hn = 0, Wn = 0;
  size_t end = 0;
  ragged_geometry(offsets, heights, widths, B, frame_f32, res, geo, Hn, Wn, end);
  const size_t es = frame_f32 ? 4 : 1;
  if (!ragged)
    for (int b = 1; b < B; ++b)
      CC_CHECK(heights[b] == heights[0] && widths[b] == widths[0] && offsets[b] == offsets[0] + (int64_t)b * heights[0] * widths[0] * 3 * (int64_t)es,
               "the uniform launch takes frames of one size, one behind the other");
  const int Ho = Hn / 2, Wo = Wn / 2;
  CC_CHECK((long)B * Ho * Wo * out_cstride < kMaxElems && end < (size_t)1 << 31, "tensor too large");
  bool big = false;
  for (int b = 0; b < B; ++b) big = big || stem_needs_big(heights[b], widths[b], geo[b].nh, geo[b].nw, frame_f32);
  if (info) { info[0] = Hn; info[1] = Wn; info[2] = big ? 1 : 0; }

  hipStream_t s = (hipStream_t)stream;
  Owner own;
  const HostTensor w = host_tensor(w_oihw, {Cout, 3, 3, 3}), bt = host_tensor(bias, {Cout});
  const PackedConv pc = own.keep(pack_convs(dtype, {&w}, {&bt}, {1}, 8, split));          // the stem conv's 3 channels padded to 8 (cc_yolo::cin_pad)
  CC_CHECK(pc.k == 3 && pc.cin == 8 && pc.cout == Cout, "unexpected weight layout");
  auto stem_plane = [&](int plane) {                                                      // Builder::stem_weights
    void* f = own.alloc((size_t)Cout * 32 * dtype_size(dtype) + 256);
    stem_pack_weights(dtype, pc.w, pc.kw, pc.split ? 16 : 8, plane ? 8 : 0, Cout, f, s);
    return f;
  };
  StemP q{};
  q.w = stem_plane(0); q.bias = pc.bias; q.Cout = Cout;
  q.w_lo = pc.split ? stem_plane(1) : nullptr; q.oscale = pc.oscale;
  q.out = out_dev; q.out_cstride = out_cstride; q.out_coff = out_coff; q.Ho = Ho; q.Wo = Wo;
  // the letterbox as a plan holds it (plan_prep); a ragged plan's own geometry is the network shape (get_plan), the records carry the frames'
  Plan P;
  P.B = B; P.frame_f32 = frame_f32 ? 1 : 0; P.Hn = Hn; P.Wn = Wn;
  std::vector<int> lo, hi; std::vector<float> fr;
  struct Tab { const int* lo; const int* hi; const float* fr; };
  auto tables = [&](int n_in, int n_out) { axis_tables(n_in, n_out, lo, hi, fr); return Tab{own.upload(lo), own.upload(hi), own.upload(fr)}; };
  if (!ragged) {
    P.H = heights[0]; P.W = widths[0]; P.nh = geo[0].nh; P.nw = geo[0].nw; P.pad_y = geo[0].pad_y; P.pad_x = geo[0].pad_x;
    const Tab tx = tables(P.W, P.nw), ty = tables(P.H, P.nh);
    q.pre = plan_prep(&P);
    q.pre.xlo = tx.lo; q.pre.xhi = tx.hi; q.pre.xfr = tx.fr; q.pre.ylo = ty.lo; q.pre.yhi = ty.hi; q.pre.yfr = ty.fr;
    q.pre.frames = reinterpret_cast<const unsigned char*>(frames_dev) + offsets[0];
    launch_stem_fused(dtype, q, s);
  } else {
    P.H = Hn; P.W = Wn; P.nh = Hn; P.nw = Wn; P.pad_y = P.pad_x = 0; P.ragged = true;
    std::vector<FrameDesc> desc((size_t)B);
    for (int b = 0; b < B; ++b) {
      const Tab tx = tables(widths[b], geo[b].nw), ty = tables(heights[b], geo[b].nh);
      desc[b] = frame_record(offsets[b], heights[b], widths[b], geo[b], Hn, Wn, tx.lo, tx.hi, tx.fr, ty.lo, ty.hi, ty.fr);
    }
    q.pre = plan_prep(&P);
    q.pre.frames = frames_dev;
    launch_stem_fused_ragged(dtype, q, own.upload(desc), end, big, s);
  }
  CC_HIP(hipStreamSynchronize(s));
  CC_API_END
}

}  // extern "C"
