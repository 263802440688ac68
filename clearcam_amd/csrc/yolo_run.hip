// Detector runtime, plan execution: the plan of a shape (letterbox geometry, op list from yolo.hip's builder, captured hipGraph), one
// batch through it (cc_yolo_detect), batches in flight (cc_yolo_submit / cc_yolo_wait) and ragged batches of mixed source sizes.
#include <algorithm>
#include <cmath>
#include "yolo_plan.h"

using namespace cc;

namespace cc {

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

// letterbox geometry, detection/yolov9.py:390-403 (python round = half-to-even)
void letterbox_geometry(int H, int W, int res, int& nh, int& nw, int& pad_y, int& pad_x) {
  const double r = std::min((double)res / H, (double)res / W);
  nw = round_half_even(W * r); nh = round_half_even(H * r);
  const double dw = ((res - nw) % 32) / 2.0, dh = ((res - nh) % 32) / 2.0;
  pad_x = round_half_even(dw - 0.1); pad_y = round_half_even(dh - 0.1);
}
const char* const kNot32 = "letterboxed frame is not a multiple of 32 (the reference graph cannot run this shape either)";

// The letterbox of plan P as a launch's PreP; the caller adds its own frames / out fields.
PreP plan_prep(const Plan* P) {
  PreP pp{};
  pp.frame_f32 = P->frame_f32; pp.B = P->B; pp.H = P->H; pp.W = P->W;
  pp.nh = P->nh; pp.nw = P->nw; pp.pad_y = P->pad_y; pp.pad_x = P->pad_x; pp.Hn = P->Hn; pp.Wn = P->Wn;
  pp.xlo = P->xlo; pp.xhi = P->xhi; pp.xfr = P->xfr; pp.ylo = P->ylo; pp.yhi = P->yhi; pp.yfr = P->yfr;
  pp.flip = 1; pp.div = 255.0f; pp.sub = 0.0f; pp.pad_val = 0.0f;          // [..., ::-1] and / 255.0 (detection/yolov9.py:377-379)
  return pp;
}

// One launch of the plan.  A Stem op (fused letterbox + first conv) reads the caller's frames: inside the captured graph it is skipped
// (run_stems launches it right before the graph); the profilers replay it on the frames of the last call.
void launch_op(int dtype, const Plan* P, const Op& op, hipStream_t s, bool with_stem) {
  switch (op.kind) {
    case Conv: launch_conv(dtype, op.conv, s); break;
    case Pool: launch_pool(dtype, op.pool, s); break;
    case Decode: launch_decode(op.dec, s); break;
    case Nms: if (P->ragged) launch_topk_nms_ragged(op.nms, P->desc_dev, s); else launch_topk_nms(op.nms, s); break;
    case Fuse: launch_fuse(dtype, op.fuse, s); break;
    case Stem: if (with_stem) { StemP q = op.stem; q.pre.frames = P->last_frames; launch_stem_fused(dtype, q, s); } break;
    case Csp: launch_csp_fused(dtype, op.csp, s); break;
    case HeadTail: launch_head_tail(dtype, op.tail, s); break;
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
      if (op.kind == Stem) continue;                                     // runs before the graph
      const int l = op.lane; hipStream_t st = stream_of(l);
      std::vector<int> need(nl, -1);
      for (int j = 0; j < i; ++j) { const Op& o = P->ops[j]; if (o.kind != Stem && o.lane != l && ops_conflict(Y, P, op, o)) need[o.lane] = j; }
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
  for (Op& op : P->ops) if (op.kind == Stem) {
    op.stem.pre.frames = frames;
    if (P->ragged) launch_stem_fused_ragged(Y->dtype, op.stem, P->desc_dev, P->packed_bytes, P->stem_big, s);
    else launch_stem_fused(Y->dtype, op.stem, s);
  }
}

// ragged: H x W IS the network shape; the key carries the flag and NOT the source sizes, so a camera that changes resolution keeps its graph
Plan* get_plan(cc_yolo* Y, int B, int H, int W, int frame_f32, int slot, bool ragged) {
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
  build_plan(Y, P.get());
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

// One batch through plan P on stream s: the letterbox (or the fused letterbox + first conv launches, which read the caller's frames)
// and then the captured graph.
void input_step(cc_yolo* h, Plan* P, hipStream_t s, const void* fdev) {
  PreP pp = plan_prep(P);
  pp.frames = fdev; pp.out = P->arena + P->bufs[P->in_buf].off; pp.out_c = P->bufs[P->in_buf].C;
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
      fprintf(stderr, "[clearcam] op %d kind %d: %s\n", i, (int)op.kind, hipGetErrorString(e)); fflush(stderr);
      ++i;
    }
  } else
  CC_HIP(hipGraphLaunch(P->exec, s));
}

// cc_yolo_detect / cc_yolo_detect_ragged from the plan on: `bytes` of frames (uniform: B*H*W*3 elements; ragged: the packed buffer)
static void detect_on_plan(cc_yolo* h, Plan* P, const void* frames, size_t bytes, int frames_on_device, float* out, int out_on_device, void* stream) {
  const int B = P->B;
  hipStream_t s = h->stream;
  if (stream) order_after(s, (hipStream_t)stream);   // order our stream after the caller's
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
    if (stream) order_after((hipStream_t)stream, s);
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
  // the frames are ready on the caller's stream; the caller's stream is NOT made to wait for the result (cc_yolo_wait does that)
  if (stream) order_after(s, (hipStream_t)stream);
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

// taps and profilers read what the last call left behind: every stream of the handle has to be idle
void sync_all(cc_yolo* h) {
  CC_HIP(hipStreamSynchronize(h->stream));
  for (hipStream_t t : h->slot_stream) CC_HIP(hipStreamSynchronize(t));
}

// The checks of a ragged batch, no HIP call: every frame's letterbox geometry, the ONE network shape Hn x Wn they must share (a multiple of
// 32) and `end`, the size of the packed buffer (the last byte any frame reaches).
void ragged_geometry(const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B, int frame_f32, int res,
                     std::vector<LetterboxGeo>& geo, int& Hn, int& Wn, size_t& end) {
  const size_t es = frame_f32 ? 4 : 1;
  geo.assign(B, LetterboxGeo{});
  Hn = Wn = 0; end = 0;
  for (int b = 0; b < B; ++b) {
    const std::string who = "frame " + std::to_string(b) + " (" + std::to_string(heights[b]) + "x" + std::to_string(widths[b]) + ")";
    if (heights[b] <= 0 || widths[b] <= 0 || offsets[b] < 0) throw cc::Error(-22, who + ": bad shape or offset");
    if (frame_f32 && offsets[b] % 4 != 0) throw cc::Error(-22, who + ": float32 frames must start at a multiple of 4 bytes");
    LetterboxGeo& g = geo[b];
    letterbox_geometry(heights[b], widths[b], res, g.nh, g.nw, g.pad_y, g.pad_x);
    const int hn = g.nh + 2 * g.pad_y, wn = g.nw + 2 * g.pad_x;
    if (!(hn % 32 == 0 && wn % 32 == 0 && hn > 0 && wn > 0 && g.nh > 0 && g.nw > 0)) throw cc::Error(-22, who + ": " + kNot32);
    if (b == 0) { Hn = hn; Wn = wn; }
    else if (hn != Hn || wn != Wn)
      throw cc::Error(-22, who + " letterboxes to " + std::to_string(hn) + "x" + std::to_string(wn) + " but frame 0 (" + std::to_string(heights[0]) + "x" +
                               std::to_string(widths[0]) + ") to " + std::to_string(Hn) + "x" + std::to_string(Wn) +
                               ": the frames of one ragged batch must share one network shape (group them with cc_letterbox_geometry)");
    end = std::max(end, (size_t)offsets[b] + (size_t)heights[b] * widths[b] * 3 * es);
  }
}

// One frame's record of a ragged batch: its place in the packed buffer, its geometry, its six axis tables (device) and scale_boxes.
FrameDesc frame_record(long long off, int H, int W, const LetterboxGeo& g, int Hn, int Wn, const int* xlo, const int* xhi, const float* xfr,
                       const int* ylo, const int* yhi, const float* yfr) {
  FrameDesc d{};
  d.off = off; d.H = H; d.W = W; d.nh = g.nh; d.nw = g.nw; d.pad_y = g.pad_y; d.pad_x = g.pad_x;
  d.xlo = xlo; d.xhi = xhi; d.xfr = xfr; d.ylo = ylo; d.yhi = yhi; d.yfr = yfr;
  // scale_boxes exactly as the uniform plan's NMS launch gets it (Builder::head_finish): double arithmetic, then one cast to float
  const double gain = std::min((double)Hn / H, (double)Wn / W);
  d.gain = (float)gain;
  d.fpad_x = (float)((Wn - W * gain) / 2); d.fpad_y = (float)((Hn - H * gain) / 2);
  d.src_w = (float)W; d.src_h = (float)H;
  return d;
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
  std::vector<LetterboxGeo> geo;
  int Hn = 0, Wn = 0;
  size_t end = 0;
  ragged_geometry(offsets, heights, widths, B, frame_f32, h->res, geo, Hn, Wn, end);
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
    const LetterboxGeo& g = geo[b];
    const int H = heights[b], W = widths[b];
    const cc_yolo::AxisTab &tx = axis_tab(h, W, g.nw), &ty = axis_tab(h, H, g.nh);
    const FrameDesc d = frame_record(offsets[b], H, W, g, Hn, Wn, tx.lo, tx.hi, tx.fr, ty.lo, ty.hi, ty.fr);
    P->desc_host[b] = d;
    big = big || stem_needs_big(H, W, g.nh, g.nw, frame_f32);
  }
  P->stem_big = big; P->packed_bytes = end;
  *bytes = end;
  return P;
}

}  // namespace cc

extern "C" {

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

int cc_yolo_set_in_flight(cc_yolo* h, int n) {
  CC_API_BEGIN
  CC_CHECK(h && n >= 1 && n <= 8, "in-flight depth must be 1..8");
  CC_HIP(hipSetDevice(h->device));
  if (n == (int)h->slot_stream.size() + 1 && !h->slot_done.empty()) return 0;   // same depth: plans, slots and outstanding tickets stay valid
  sync_all(h);
  h->plans.clear();                                     // plans are built for one depth (lanes on or off) and belong to a slot
  h->last = nullptr;
  resize_slots(h->device, h->stream, h->slot_stream, h->slot_done, n);
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

}  // extern "C"
