// The detector's internal types, shared by its translation units: yolo.hip (model -> op list), yolo_run.hip (plan execution and the
// detect / submit entry points), calibrate.hip ("f16c"), yolo_profile.hip (taps and profilers), dev_bench.hip (single-launch benches).
#pragma once
#include "kernels.h"
#include "../../include/clearcam_hip.h"

namespace cc {

struct Arch {
  const char* size; int stem; bool elan1; int b2_hidden, b2_out; bool adown; int d3_out, e4_hidden, p3, b4_out,
      d5_out, e6_hidden, p4, d7_out, e8_hidden, p5, spp_hidden, d16_out, d19_out, cls_hidden, rep_n;
};

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };
struct PackedConv { void* w = nullptr; float* bias = nullptr; int cin = 0, cout = 0, k = 0, kw = 0; double macs_px = 0; int split = 0; float oscale = 1.0f; };

struct Buf { int H, W, C; bool f32; size_t off; };
struct View { int buf; int coff; int C; };
struct In { View v; int shift; };

// What a launch of the plan is.  The numbers are part of the record: CLEARCAM_EAGER_DEBUG prints them.
//   Stem: letterbox + first conv (launched before the graph: it reads the caller's frames); Csp: fused RepNCSP;
//   HeadTail: fused DDetect tail (last 1x1 convs of both branches + decode)
enum OpKind : int { Conv = 0, Pool = 1, Decode = 2, Nms = 3, Fuse = 4, Stem = 5, Csp = 6, HeadTail = 7 };

struct Op {
  OpKind kind;
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

struct cc_yolo {
  const cc::Arch* arch = nullptr;
  int res = 640, dtype = cc::BF16, device = 0;              // dtype: STORAGE type of activations and weights
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
  std::map<std::string, cc::HostTensor> host;
  std::map<std::string, cc::PackedConv> packed;
  float* dfl_w = nullptr;
  bool finalized = false;
  cc::PlanCache<std::vector<int>, cc::Plan> plans;
  cc::Plan* last = nullptr;
  int plans_built = 0;                                 // plans built (arena + graph capture) over the handle's life: cc_yolo_plans_built
  // Axis tables of the ragged entry points, one device allocation (lo | hi | fr) per distinct (n_in, n_out), least recently used dropped
  // beyond kMaxAxisTabs (ragged_prepare): a site has a handful of camera models, so a frame's tables are almost always already there.
  struct AxisTab { int* lo; int* hi; float* fr; unsigned long long used; };
  std::map<std::pair<int, int>, AxisTab> axis_tabs;
  unsigned long long axis_tick = 0;
  int cin_pad() const { return dtype == cc::F32 ? 4 : 8; }
};

namespace cc {

// ---- yolo.hip ----
// Pack a list of OIHW convs over the same input into one [sum Cout][k*k*cin_pad] matrix (+ bias); device memory, owned by the caller.
PackedConv pack_convs(int dt, const std::vector<const HostTensor*>& ws, const std::vector<const HostTensor*>& bs,
                      const std::vector<int>& groups, int cin_pad, int split = 0);
// The op list of P (geometry and axis tables set) from the handle's weights, its arena packed and allocated, every pointer patched.
void build_plan(cc_yolo* Y, Plan* P);
// ---- yolo_run.hip ----
// letterbox geometry, detection/yolov9.py:390-403
struct LetterboxGeo { int nh, nw, pad_y, pad_x; };
void letterbox_geometry(int H, int W, int res, int& nh, int& nw, int& pad_y, int& pad_x);
extern const char* const kNot32;                         // the error text of a frame that does not letterbox to a multiple of 32
// a ragged batch's checks and per-frame records (cc_yolo_detect_ragged, cc_dev_stem); neither makes a HIP call
void ragged_geometry(const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B, int frame_f32, int res,
                     std::vector<LetterboxGeo>& geo, int& Hn, int& Wn, size_t& end);
FrameDesc frame_record(long long off, int H, int W, const LetterboxGeo& g, int Hn, int Wn, const int* xlo, const int* xhi, const float* xfr,
                       const int* ylo, const int* yhi, const float* yfr);
PreP plan_prep(const Plan* P);
void launch_op(int dtype, const Plan* P, const Op& op, hipStream_t s, bool with_stem);
Plan* get_plan(cc_yolo* Y, int B, int H, int W, int frame_f32, int slot = 0, bool ragged = false);
void input_step(cc_yolo* h, Plan* P, hipStream_t s, const void* fdev);
void sync_all(cc_yolo* h);
// ---- calibrate.hip ----
void calibrate_1x1(cc_yolo* h);

}  // namespace cc
