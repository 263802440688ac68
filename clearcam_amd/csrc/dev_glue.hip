// Development entries that run ONE launch of a kernel that sits between the convs, outside any plan, on inputs the caller crafts:
// cc_dev_pool / cc_dev_pool_choice (launch_pool and its selection rule), cc_dev_fuse (launch_fuse, CBFuse) and cc_dev_conv_src (one conv
// over two Src views - Concat, nearest-x2 upsample or the 2x2 average folded into the loader - weights packed by the detector's own
// pack_convs; cc_dev_conv_det is its sibling for the detector's launches: groups densified as the detector does it and a residual that
// may be the output buffer; cc_dev_conv_det_choice stops at the selector).  Each validates its arguments and launches nothing on bad
// input, goes through the production launcher and synchronises the stream.  Whatever a launcher refuses is refused before the first HIP call, so the refusals can be tested without a device.
// cc_dev_affine and cc_dev_face_pre are in face.hip, beside the kernels they launch.
#include "conv_select.h"
#include "yolo_plan.h"

using namespace cc;

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
constexpr long kMaxElems = 1L << 30;                     // elements of one buffer: every index the kernels form stays inside int / 32-bit byte offsets

PoolP pool_args(int dtype, const void* in_dev, int in_cstride, int in_coff, void* out_dev, int out_cstride, int out_coff, int B, int H, int W,
                int C, int Ho, int Wo, int k, int stride, int pad, int mode) {
  CC_CHECK(dtype == F32 || dtype == F16 || dtype == BF16, "dtype must be 0 (f32), 1 (f16) or 2 (bf16)");
  CC_CHECK(in_dev && out_dev, "null argument");
  CC_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0, "bad shape");
  CC_CHECK(mode >= 0 && mode <= 2 && k > 0 && k <= 16 && stride > 0 && pad >= 0 && pad < k, "bad window");
  CC_CHECK(in_coff >= 0 && in_coff + C <= in_cstride && out_coff >= 0 && out_coff + C <= out_cstride, "bad channel view");
  CC_CHECK((long)B * H * W * in_cstride < kMaxElems && (long)B * Ho * Wo * out_cstride < kMaxElems, "tensor too large");
  // every window holds at least one input position (mode 0: all of them - the average counts what it pads)
  const int Hp = mode == 2 ? H - 1 : H, Wp = mode == 2 ? W - 1 : W;        // mode 2: the max stage walks the averaged map
  CC_CHECK(Hp > 0 && Wp > 0, "avg-max pool: the input needs two rows and two columns");
  if (mode == 0) CC_CHECK(pad == 0 && (Ho - 1) * stride + k <= H && (Wo - 1) * stride + k <= W, "avg pool: windows must lie inside the input (pad 0)");
  else CC_CHECK((Ho - 1) * stride - pad < Hp && (Wo - 1) * stride - pad < Wp, "Ho / Wo beyond the padded input");
  PoolP p{};
  p.in = in_dev; p.in_cstride = in_cstride; p.in_coff = in_coff; p.out = out_dev; p.out_cstride = out_cstride; p.out_coff = out_coff;
  p.B = B; p.H = H; p.W = W; p.C = C; p.Ho = Ho; p.Wo = Wo; p.k = k; p.stride = stride; p.pad = pad; p.mode = mode;
  return p;
}

Src src_view(const cc_src_desc& s) { return Src{s.ptr, s.H, s.W, s.cstride, s.coff, s.C, s.shift}; }

// What the two conv entries share.  `det` = cc_dev_conv_det: groups (densified by pack_convs), a residual that may be the output buffer,
// eight ints of choice.  launch = false: everything up to the selector, no HIP call (cc_dev_conv_det_choice).
int dev_conv(bool det, bool launch, const cc_conv_desc* d, const cc_src_desc* s0, const cc_src_desc* s1, const float* w_oihw, const float* bias,
             const void* res_dev, void* out_dev, int* choice, void* stream) {
  PackedConv pc;                                         // pack_convs hands its device memory to the caller
  auto release = [&]() { if (pc.w) hipFree(pc.w); if (pc.bias) hipFree(pc.bias); pc.w = nullptr; pc.bias = nullptr; };
  try {
    CC_CHECK(d && s0 && out_dev && (w_oihw || !launch), "null argument");
    CC_CHECK(d->dtype == F32 || d->dtype == F16 || d->dtype == BF16 || d->dtype == F16S, "dtype must be 0 (f32), 1 (f16), 2 (bf16) or 3 (f16s)");
    const int split = d->dtype == F16S, dt = storage_dtype(d->dtype);
    CC_CHECK(d->B > 0 && d->H > 0 && d->W > 0 && d->k > 0 && d->k <= 7 && d->stride > 0 && d->Cin > 0 && d->Cout > 0, "bad shape");
    if (!det) CC_CHECK(d->groups == 1 && d->act >= 0 && d->act <= 2 && !d->res_f32 && !d->res_cstride && !d->res_coff, "one group, act 0 .. 2, no residual");
    else {
      CC_CHECK(d->groups >= 1 && d->Cin % d->groups == 0 && d->Cout % d->groups == 0, "groups must divide Cin and Cout");
      CC_CHECK(d->act >= 0 && d->act <= (launch ? 2 : 4), "act 0 .. 2");     // pack_convs carries no PReLU slopes; the selector may be asked about any act
      CC_CHECK(res_dev || (!d->res_f32 && !d->res_cstride && !d->res_coff), "a residual view without a residual pointer");
    }
    ConvP c{};
    c.s0 = src_view(*s0);
    c.s1 = s1 ? src_view(*s1) : Src{s0->ptr, 1, 1, 0, 0, 0, 0};
    c.B = d->B; c.Hin = d->H; c.Win = d->W; c.Cin = d->Cin; c.Cout = d->Cout; c.ks = d->k; c.stride = d->stride; c.pad = d->pad < 0 ? d->k / 2 : d->pad;
    c.Ho = d->Ho > 0 ? d->Ho : (c.Hin + 2 * c.pad - c.ks) / c.stride + 1; c.Wo = d->Wo > 0 ? d->Wo : (c.Win + 2 * c.pad - c.ks) / c.stride + 1;
    CC_CHECK(c.s0.C > 0 && c.s1.C >= 0 && c.s0.C + c.s1.C == c.Cin, "Cin must be the channels of the two sources");
    for (const Src* s : {&c.s0, &c.s1}) {
      if (s->C == 0) continue;
      CC_CHECK(s->ptr && s->H > 0 && s->W > 0 && s->coff >= 0 && s->coff + s->C <= s->cstride && (long)c.B * s->H * s->W * s->cstride < kMaxElems, "bad source view");
      CC_CHECK(s->shift >= -1 && s->shift <= 4, "shift must be -1 (2x2 average), 0 or a nearest-upsample exponent");
      // the logical input H x W must lie inside what the source holds: (H - 1) >> shift rows up, H + 1 rows under the 2x2 average
      if (s->shift >= 0) CC_CHECK(((c.Hin - 1) >> s->shift) < s->H && ((c.Win - 1) >> s->shift) < s->W, "a source is smaller than the input over 2^shift");
      else CC_CHECK(s == &c.s0 && c.Hin == s->H - 1 && c.Win == s->W - 1, "the 2x2 average: first source only, input = (H - 1) x (W - 1) of it");
    }
    c.out = out_dev; c.out_cstride = d->out_cstride > 0 ? d->out_cstride : d->Cout; c.out_coff = d->out_coff; c.out_f32 = d->out_f32 ? 1 : 0;
    c.act = d->act; c.variant = d->variant; c.split = split;
    c.Ktot = c.ks * c.ks * c.Cin * (1 + split);
    c.Kw = (c.Ktot + 63) / 64 * 64;                      // as pack_convs lays the rows out (checked below)
    CC_CHECK(c.Ho > 0 && c.Wo > 0 && c.out_coff >= 0 && c.out_coff + c.Cout <= c.out_cstride && (long)c.B * c.Ho * c.Wo * c.out_cstride < kMaxElems, "bad output view");
    // the loaders read zeros past the bottom / right edge, never before the top / left one: every window must start inside pad
    CC_CHECK(c.pad >= 0 && c.pad < c.ks && (c.Ho - 1) * c.stride - c.pad < c.Hin && (c.Wo - 1) * c.stride - c.pad < c.Win, "Ho / Wo beyond the padded input");
    const bool adown = c.s0.shift < 0;
    if (res_dev) {
      c.res = res_dev; c.res_f32 = d->res_f32 ? 1 : 0; c.res_cstride = d->res_cstride > 0 ? d->res_cstride : d->Cout; c.res_coff = d->res_coff;
      CC_CHECK(c.res_coff >= 0 && c.res_coff + c.Cout <= c.res_cstride && (long)c.B * c.Ho * c.Wo * c.res_cstride < kMaxElems, "bad residual view");
      CC_CHECK(!adown, "the averaging loader takes no residual");
      // in place (RepNBottleneck's x + cv2(cv1(x))): every element is read and written by the same thread only when the two views are one
      CC_CHECK(res_dev != out_dev || (c.res_f32 == c.out_f32 && c.res_cstride == c.out_cstride && c.res_coff == c.out_coff),
               "a residual that is the output buffer must be the output's own view");
    }
    if (adown) CC_CHECK(d->groups == 1 && conv_adown_supported(dt, c), "fused average + stride-2 conv: unsupported shape");
    ConvChoice ch;
    if (!adown) ch = choose_conv(dt, c);                 // pure: an unknown variant or a forced kernel the shape is not eligible for stops here
    const int nch = det ? 8 : 6;
    auto report = [&]() {
      if (!choice) return;
      const int adn[8] = {CC_DEV_CONV_ADOWN, 0, 128, adown ? conv_adown_bn(c) : 0, 0, 0, 0, 0};
      const int got[8] = {(int)ch.kernel, ch.sched, ch.bm, ch.bn, ch.simple ? 1 : 0, ch.two ? 1 : 0, ch.cprw, ch.ns};
      for (int i = 0; i < nch; ++i) choice[i] = adown ? adn[i] : got[i];
    };
    if (!launch) { report(); return 0; }
    HostTensor w, b;
    const size_t wn = (size_t)d->Cout * (d->Cin / d->groups) * d->k * d->k;
    w.shape = {d->Cout, d->Cin / d->groups, d->k, d->k};
    w.data.assign(w_oihw, w_oihw + wn);
    if (bias) { b.shape = {d->Cout}; b.data.assign(bias, bias + d->Cout); }
    pc = pack_convs(dt, {&w}, {bias ? &b : nullptr}, {d->groups}, 0, split);
    CC_CHECK(pc.kw == c.Kw && pc.cin == c.Cin, "unexpected weight layout");
    c.w = pc.w; c.bias = pc.bias; c.oscale = pc.oscale;
    if (adown) launch_conv_adown(dt, c, (hipStream_t)stream);
    else launch_conv_chosen(dt, c, (hipStream_t)stream, &ch);
    CC_HIP(hipStreamSynchronize((hipStream_t)stream));
    report();
    release();
    return 0;
  } catch (const cc::Error& e) { release(); cc::set_error(e.what()); return e.code; }
  catch (const std::exception& e) { release(); cc::set_error(e.what()); return -1; }
}

}  // namespace

extern "C" {

int cc_dev_pool_choice(int dtype, const void* in_dev, int in_cstride, int in_coff, void* out_dev, int out_cstride, int out_coff, int B, int H,
                       int W, int C, int Ho, int Wo, int k, int stride, int pad, int mode, int* kernel) {
  CC_API_BEGIN
  CC_CHECK(kernel, "null argument");
  const PoolP p = pool_args(dtype, in_dev, in_cstride, in_coff, out_dev, out_cstride, out_coff, B, H, W, C, Ho, Wo, k, stride, pad, mode);
  *kernel = (int)choose_pool(dtype, p);
  CC_API_END
}

int cc_dev_pool(int dtype, const void* in_dev, int in_cstride, int in_coff, void* out_dev, int out_cstride, int out_coff, int B, int H, int W,
                int C, int Ho, int Wo, int k, int stride, int pad, int mode, int* kernel, void* stream) {
  CC_API_BEGIN
  const PoolP p = pool_args(dtype, in_dev, in_cstride, in_coff, out_dev, out_cstride, out_coff, B, H, W, C, Ho, Wo, k, stride, pad, mode);
  PoolKernel ran = POOL_SCALAR;
  launch_pool(dtype, p, (hipStream_t)stream, &ran);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  if (kernel) *kernel = (int)ran;
  CC_API_END
}

int cc_dev_fuse(int dtype, int n, const void* const* in_dev, const int* H, const int* W, const int* cstride, const int* coff, const int* shift,
                void* out_dev, int out_cstride, int out_coff, int B, int Ho, int Wo, int C, void* stream) {
  CC_API_BEGIN
  CC_CHECK(dtype == F32 || dtype == F16 || dtype == BF16, "dtype must be 0 (f32), 1 (f16) or 2 (bf16)");
  CC_CHECK(in_dev && H && W && cstride && coff && shift && out_dev, "null argument");
  CC_CHECK(n >= 1 && n <= 6, "CBFuse takes 1 .. 6 inputs");
  CC_CHECK(B > 0 && Ho > 0 && Wo > 0 && C > 0, "bad shape");
  CC_CHECK(out_coff >= 0 && out_coff + C <= out_cstride && aligned16(out_dev) && (long)B * Ho * Wo * out_cstride < kMaxElems, "bad output view");
  FuseP p{};
  p.n = n; p.out = out_dev; p.out_cstride = out_cstride; p.out_coff = out_coff; p.B = B; p.Ho = Ho; p.Wo = Wo; p.C = C;
  for (int i = 0; i < n; ++i) {
    CC_CHECK(in_dev[i] && aligned16(in_dev[i]), "inputs must be non-null and 16-byte aligned (uint4 loads)");
    CC_CHECK(shift[i] >= 0 && shift[i] <= 8 && H[i] > 0 && W[i] > 0 && ((Ho - 1) >> shift[i]) < H[i] && ((Wo - 1) >> shift[i]) < W[i],
             "an input is smaller than the output map over 2^shift");
    CC_CHECK(coff[i] >= 0 && coff[i] + C <= cstride[i] && (long)B * H[i] * W[i] * cstride[i] < kMaxElems, "bad input view");
    p.in[i] = in_dev[i]; p.H[i] = H[i]; p.W[i] = W[i]; p.cstride[i] = cstride[i]; p.coff[i] = coff[i]; p.shift[i] = shift[i];
  }
  launch_fuse(dtype, p, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  CC_API_END
}

int cc_dev_conv_src(const cc_conv_desc* d, const cc_src_desc* s0, const cc_src_desc* s1, const float* w_oihw, const float* bias, void* out_dev,
                    int* choice, void* stream) {
  return dev_conv(false, true, d, s0, s1, w_oihw, bias, nullptr, out_dev, choice, stream);
}

int cc_dev_conv_det(const cc_conv_desc* d, const cc_src_desc* s0, const cc_src_desc* s1, const float* w_oihw, const float* bias,
                    const void* res_dev, void* out_dev, int* choice, void* stream) {
  return dev_conv(true, true, d, s0, s1, w_oihw, bias, res_dev, out_dev, choice, stream);
}

int cc_dev_conv_det_choice(const cc_conv_desc* d, const cc_src_desc* s0, const cc_src_desc* s1, const void* res_dev, void* out_dev, int* choice) {
  return dev_conv(true, false, d, s0, s1, nullptr, nullptr, res_dev, out_dev, choice, nullptr);
}

}  // extern "C"
