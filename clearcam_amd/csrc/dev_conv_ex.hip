// Development entry cc_conv2d_ex: ONE conv launch with any ConvP the CLIP, AdaFace and BlazeFace plans build (every activation, PReLU
// slopes, a 16-bit or f32 residual that may alias the output, f32 output, channel-slice views, asymmetric padding through Ho / Wo),
// weights packed by the face nets' own pack_conv.  Reports the ConvChoice the launch ran with: four ints (kernel, sched, bm, bn), as its
// callers have always sized the buffer; cc_conv2d_ex_route is the same launch reporting the eight ints of cc_dev_conv_det.
// A translation unit of its own because net_common.h and yolo_plan.h (dev_bench.hip) each define the host tensor type.
#include "conv_select.h"
#include "net_common.h"
#include "../../include/clearcam_hip.h"

using namespace cc;

namespace {

// nchoice: ints of `choice` the caller's buffer holds (4 or 8)
int conv2d_ex(const cc_conv_desc* d, const void* x_dev, const float* w_oihw, const float* bias, const float* slope,
              const void* res_dev, void* out_dev, int* choice, int nchoice, void* stream) {
  std::vector<void*> owner;
  auto release = [&]() { for (void* q : owner) hipFree(q); owner.clear(); };
  try {
    CC_CHECK(d && x_dev && w_oihw && out_dev, "null argument");
    CC_CHECK(d->dtype == F32 || d->dtype == F16 || d->dtype == BF16, "dtype must be 0 (f32), 1 (f16) or 2 (bf16)");
    CC_CHECK(d->B > 0 && d->H > 0 && d->W > 0 && d->k > 0 && d->stride > 0, "bad shape");
    CC_CHECK(d->groups >= 1 && d->Cin > 0 && d->Cout > 0 && d->Cin % d->groups == 0 && d->Cout % d->groups == 0, "bad channel counts");
    CC_CHECK(d->act >= 0 && d->act <= 4, "act must be 0..4");
    CC_CHECK(d->act != 3 || slope, "act 3 (PReLU) needs slope[Cout]");
    HostTensor w;
    w.shape = {d->Cout, d->Cin / d->groups, d->k, d->k};
    w.data.assign(w_oihw, w_oihw + (size_t)d->Cout * (d->Cin / d->groups) * d->k * d->k);
    PConv pc = pack_conv(d->dtype, owner, w, d->groups, {}, bias ? std::vector<float>(bias, bias + d->Cout) : std::vector<float>());
    if (slope) pc.slope = upload_f32(owner, std::vector<float>(slope, slope + d->Cout));
    const int ocs = d->out_cstride > 0 ? d->out_cstride : d->Cout;
    ConvP c = conv_params(pc, x_dev, d->B, d->H, d->W, d->stride, out_dev, ocs, d->out_f32 ? 1 : 0, d->act, res_dev,
                          d->res_cstride > 0 ? d->res_cstride : d->Cout, d->pad, d->Ho, d->Wo);
    c.out_coff = d->out_coff; c.res_coff = res_dev ? d->res_coff : 0; c.res_f32 = res_dev && d->res_f32 ? 1 : 0;
    c.variant = d->variant;
    CC_CHECK(c.Ho > 0 && c.Wo > 0 && c.out_coff >= 0 && c.out_coff + c.Cout <= c.out_cstride, "bad output view");
    CC_CHECK(!c.res || (c.res_coff >= 0 && c.res_coff + c.Cout <= c.res_cstride), "bad residual view");
    // the loaders read zeros past the bottom / right edge, never before the top / left one: every window must start inside pad
    CC_CHECK(c.pad >= 0 && c.pad < c.ks && (c.Ho - 1) * c.stride - c.pad < c.Hin && (c.Wo - 1) * c.stride - c.pad < c.Win, "Ho / Wo beyond the padded input");
    ConvChoice ch;
    launch_conv_chosen(d->dtype, c, (hipStream_t)stream, &ch);
    CC_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (choice) {                                        // the order cc_dev_conv_det reports them in
      const int got[8] = {(int)ch.kernel, ch.sched, ch.bm, ch.bn, ch.simple ? 1 : 0, ch.two ? 1 : 0, ch.cprw, ch.ns};
      for (int i = 0; i < nchoice; ++i) choice[i] = got[i];
    }
    release();
    return 0;
  } catch (const cc::Error& e) { release(); cc::set_error(e.what()); return e.code; }
  catch (const std::exception& e) { release(); cc::set_error(e.what()); return -1; }
}

}  // namespace

extern "C" {

int cc_conv2d_ex(const cc_conv_desc* d, const void* x_dev, const float* w_oihw, const float* bias, const float* slope,
                 const void* res_dev, void* out_dev, int* choice, void* stream) {
  return conv2d_ex(d, x_dev, w_oihw, bias, slope, res_dev, out_dev, choice, 4, stream);
}

int cc_conv2d_ex_route(const cc_conv_desc* d, const void* x_dev, const float* w_oihw, const float* bias, const float* slope,
                       const void* res_dev, void* out_dev, int* choice, void* stream) {
  return conv2d_ex(d, x_dev, w_oihw, bias, slope, res_dev, out_dev, choice, 8, stream);
}

int cc_route_log_take(int* records, int cap, int* n) {
  CC_API_BEGIN
  CC_CHECK(n && cap >= 0 && (records || cap == 0), "bad argument");
  *n = route_log_take(records, cap);
  CC_API_END
}

}  // extern "C"
