// Development entry points that time or run ONE launch outside any plan: a single conv (cc_conv2d_nhwc, cc_conv_bench), a single attention
// launch (cc_attn_bench) and the kernel-selection overrides (cc_dev_set).
#include <cmath>
#include "conv_select.h"
#include "yolo_plan.h"

using namespace cc;

extern "C" {

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

int cc_dev_set(const char* key, int value) {
  CC_API_BEGIN
  CC_CHECK(key, "null key");
  if (std::string(key) == "phase_flags") cc::g_phase_flags_override = value;
  else if (std::string(key) == "stream") cc::g_stream_override = value;
  else if (std::string(key) == "stream_abl") cc::g_stream_abl = value;
  else if (std::string(key) == "stream_flags") cc::g_stream_flags_override = value;
  else if (std::string(key) == "tile64_abl") cc::g_tile64_abl = value;
  else if (std::string(key) == "tile64_w") cc::g_tile64_w_override = value;
  else if (std::string(key) == "index_slab_rows") cc::g_index_slab_rows = value;
  else if (std::string(key) == "index_i8_pass") cc::g_index_i8_pass = value;
  else if (std::string(key) == "index_i8_mfma") cc::g_index_i8_mfma = value;
  else if (std::string(key) == "pool_rows") cc::g_pool_rows_override = value;
  else if (std::string(key) == "csp_tile") cc::g_csp_tile_override = value;
  else if (std::string(key) == "route_log") cc::g_route_log = value ? 1 : 0;
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
