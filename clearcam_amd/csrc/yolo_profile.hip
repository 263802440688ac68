// Detector runtime, taps and profilers: what the last call left in the plan's arena (cc_yolo_get_tensor*), the non-finite counter, and
// the per-launch / per-graph timings behind bench.py's roofline table (cc_yolo_profile, cc_yolo_profile_graph).
#include <cstring>
#include "yolo_plan.h"

using namespace cc;

// the `kind` column of the CLEARCAM_PROFILE_CSV table (bench.py and tools/ parse it)
static std::string op_kind_name(const Op& op) {
  switch (op.kind) {
    case Conv: return op.conv.s0.shift < 0 ? "conv_avg" : "conv";
    case Pool: return "pool" + std::to_string(op.pool.mode) + "_k" + std::to_string(op.pool.k) + "_s" + std::to_string(op.pool.stride);
    case Decode: return "decode";      case Nms: return "topk_nms";     case Fuse: return "cbfuse";
    case Stem: return "stem_fused";    case Csp: return "csp_fused";    case HeadTail: return "head_tail";
  }
  return "";
}
// The slot of cc_yolo_profile's ms[5] (conv, pool, decode, nms, stem) a launch is timed in.  CBFuse counts with the pools; the fused
// letterbox + stem has its own slot; a fused RepNCSP is conv work; the fused DDetect tail (last 1x1 convs + decode) is timed in the
// decode slot, its 0.35 % of the FLOPs stay out of the conv roofline
static int profile_slot(OpKind k) {
  switch (k) {
    case Conv: case Csp: return 0;
    case Pool: case Fuse: return 1;
    case Decode: case HeadTail: return 2;
    case Nms: return 3;
    case Stem: return 4;
  }
  return 0;
}

extern "C" {

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
    PreP pp = plan_prep(P);
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
      acc[profile_slot(P->ops[i].kind)] += t;
    }
  }
  for (const Op& op : P->ops) if (op.kind == Conv || op.kind == Csp) { macs += op.alg_macs; ++nconv; }
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
        const std::string kind = op_kind_name(op);
        if (op.kind == Conv) {
          const ConvP& c = op.conv; const double M = (double)c.B * c.Ho * c.Wo;
          const double es = dtype_size(h->dtype);
          const bool avg = c.s0.shift < 0;                 // reads the 2x2 average of its source (conv_adown.hip)
          const double in0 = avg ? (double)(c.Hin + 1) * (c.Win + 1) : (double)(c.Hin >> c.s0.shift) * (c.Win >> c.s0.shift);
          const double bytes = (double)c.B * in0 * c.s0.C * es + (double)c.B * (c.Hin >> c.s1.shift) * (c.Win >> c.s1.shift) * c.s1.C * es
                             + M * c.Cout * (c.out_f32 ? 4 : es) + (c.res ? M * c.Cout * es : 0) + (double)c.Cout * c.Ktot * es;
          fprintf(f, "%zu,%s,%.4f,%.0f,%d,%d,%d,%d,%d,%.4f,%.1f,%.4f,%.0f,%d", i, kind.c_str(), t, M, c.Cout, c.Ktot, c.ks, c.stride, c.Cin,
                  op.alg_macs / 1e9, 2 * op.alg_macs / (t * 1e-3) / 1e12, bytes / 1e9, bytes / (t * 1e-3) / 1e9, 1 + c.split);
          tail(i, op.alg_macs, bytes);
        } else if (op.kind == Pool) {
          const PoolP& q = op.pool; const double es = dtype_size(h->dtype);
          const double bytes = ((double)q.B * q.H * q.W + (double)q.B * q.Ho * q.Wo) * q.C * es;
          fprintf(f, "%zu,%s,%.4f,%.0f,%d,0,%d,%d,%d,0,0,%.4f,%.0f,0", i, kind.c_str(), t, (double)q.B * q.Ho * q.Wo, q.C, q.k, q.stride, q.C,
                  bytes / 1e9, bytes / (t * 1e-3) / 1e9);
          tail(i, 0.0, bytes);
        } else if (op.kind == Stem) {
          const StemP& q = op.stem; const double M = (double)q.pre.B * q.Ho * q.Wo, es = dtype_size(h->dtype);
          const double bytes = (double)q.pre.B * q.pre.H * q.pre.W * 3 * (q.pre.frame_f32 ? 4 : 1) + M * q.Cout * es;
          fprintf(f, "%zu,%s,%.4f,%.0f,%d,27,3,2,3,%.4f,%.1f,%.4f,%.0f,%d", i, kind.c_str(), t, M, q.Cout, op.alg_macs / 1e9, 2 * op.alg_macs / (t * 1e-3) / 1e12,
                  bytes / 1e9, bytes / (t * 1e-3) / 1e9, q.w_lo ? 2 : 1);
          tail(i, op.alg_macs, bytes);
        } else if (op.kind == Csp) {
          const CspP& q = op.csp; const double M = (double)q.B * q.H * q.W, es = dtype_size(h->dtype);
          const double bytes = M * 4 * q.hid * es + (double)(8 + 18) * q.hid * q.hid * es;     // x in, out out, the four weight matrices
          fprintf(f, "%zu,%s,%.4f,%.0f,%d,%d,3,1,%d,%.4f,%.1f,%.4f,%.0f,%d", i, kind.c_str(), t, M, 2 * q.hid, (8 + 18) * q.hid, 2 * q.hid, op.alg_macs / 1e9,
                  2 * op.alg_macs / (t * 1e-3) / 1e12, bytes / 1e9, bytes / (t * 1e-3) / 1e9, q.split ? 2 : 1);
          tail(i, op.alg_macs, bytes);
        } else fprintf(f, "%zu,%s,%.4f,0,0,0,0,0,0,0,0,0,0,0,,0,0,0,0,,0\n", i, kind.c_str(), t);
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
      const bool conv = op.kind == Conv || op.kind == Csp;
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

}  // extern "C"
