// Kernel launchers (one translation unit per family).  All launches are asynchronous on `stream`.
#pragma once
#include <atomic>
#include <vector>
#include "common.h"

namespace cc {

// Per-launch note for the profiler's table (cc_yolo_profile -> CLEARCAM_PROFILE_CSV): which kernel a conv took, how many tiles of work it
// had and how many tiles the chip takes per round (resident blocks x CUs; the grid for persistent kernels).  Filled only while
// g_note_launches is set - the occupancy query is not free.
struct LaunchNote { const char* kernel; long tiles; long slots; };
extern thread_local LaunchNote g_launch_note;   // per thread: cc_yolo_profile sets the switch and reads the note on the thread that launches
extern thread_local bool g_note_launches;
template <class K> inline void note_launch(const char* name, K kernel, long tiles, int threads, size_t lds, long persistent_grid = 0) {
  if (!g_note_launches) return;
  long slots = persistent_grid;
  if (!slots) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(kernel), threads, lds) != hipSuccess) nb = 1;
    slots = (long)nb * cu_count();
  }
  g_launch_note = LaunchNote{name, tiles, slots > 0 ? slots : 1};
}

// ---- convolution / GEMM (conv_mfma.hip, conv_direct.hip) --------------------------------------
// True when the MFMA implicit-GEMM kernel can run this problem (16-byte channel alignment etc.).
bool conv_mfma_supported(int dt, const ConvP& p);
void launch_conv_mfma(int dt, const ConvP& p, hipStream_t stream);
// Generic direct convolution: any channel counts; slow path for shapes the MFMA kernel rejects.
void launch_conv_direct(int dt, const ConvP& p, hipStream_t stream);
// Picks the MFMA kernel when supported, else the direct kernel.
void launch_conv(int dt, const ConvP& p, hipStream_t stream);
// 3x3 stride-2 conv over the 2x2 stride-1 average of its source (ConvP::s0.shift == -1; Hin x Win = the averaged map): conv_adown.hip
bool conv_adown_supported(int dt, const ConvP& p);
int conv_adown_bn(const ConvP& p);                       // channel tile of the launch: 64 where that pads Cout less than 128 does
void launch_conv_adown(int dt, const ConvP& p, hipStream_t stream);

// ---- fused RepNCSP block (csp_fused.hip) ----------------------------------------------------------
// detection/yolov9.py:92-105 with n = 1: cv1 | cv2 (1x1), RepConvN 3x3, 3x3 + shortcut, cv3 (1x1) in one launch; 16-bit
// storage, hidden width 32 or 64.  Weights are the packed [Cout][Kw] matrices of the four convs it replaces.
struct CspP {
  const void* x; int x_cstride, x_coff;          // input view: 2*hid channels of a (B,H,W,x_cstride) tensor
  void* out; int out_cstride, out_coff;          // output view: 2*hid channels
  const void* w12; int kw12; const float* b12;   // cv1 | cv2: [2*hid][kw12]
  const void* wr; int kwr; const float* br;      // m.0.cv1 (RepConvN): [hid][kwr], k = tap*hid + c
  const void* wb; int kwb; const float* bb;      // m.0.cv2: [hid][kwb]
  const void* w3; int kw3; const float* b3;      // cv3: [2*hid][kw3], k = [m-branch | cv2]
  int B, H, W, hid;
  int split; float os12, osr, osb, os3;          // split weights (ConvP::split): 0 none, 1 all four convs, 2 the 1x1 convs (cv1 | cv2, cv3) only; rows [tap: hi | lo], the four exact 2^-e output scales
  int tx, tiles; float inv_tiles, inv_tx;        // filled by the launcher: 8x16 tiles per row / per image
  int dbg;                                       // development: 1..3 = stop after that stage and write its intermediate to `out`
  int stream;                                    // 1: take the weight-streaming one-tile-per-block variant even where the weights fit in LDS
};
bool csp_fused_supported(int dt, int hid, int split = 0);
// The kernel a fused RepNCSP launch takes.  choose_csp is pure (no HIP call): csp_tile.hip from 256 of its 16 x 32 tiles on (tile_mode 1),
// at every size (2) or never (0), and only where it can run (hidden width 32, split 0 / 2, no dbg, no stream); else csp_fused_kernel,
// weights resident at hidden width 32 with one plane, streamed otherwise.
enum CspKernel : int { CSP_FUSED_RESIDENT = 0, CSP_FUSED_STREAMED = 1, CSP_TILE = 2 };
CspKernel choose_csp(int dt, int hid, int split, int B, int H, int W, int stream, int dbg, int tile_mode);
// cc_dev_set("csp_tile"): the tile mode, as CLEARCAM_CSP_TILE (0 / 1 / 2); -1 = the environment / default.  csp_tile_mode() is what a launch reads.
extern std::atomic<int> g_csp_tile_override;
int csp_tile_mode();
void launch_csp_fused(int dt, const CspP& p, hipStream_t stream, CspKernel* chosen = nullptr);

// ---- calibration-aware rounding of the 1x1 convs (calibrate.hip, C-ABI dtype "f16c") -----------------------------------------------
// S pixel rows (indices rows_dev) of a 1x1 stride-1 conv's input view over f32 activations -> dense (S, Cin) f32
void launch_sample_rows(const ConvP& p, const int* rows_dev, int S, float* out_dev, hipStream_t stream);
// H (ci x ci) = X^T X / rows in double
void second_moments(const float* X, int rows, int ci, std::vector<double>& H);
// GPTQ column walk: w (co x ci) f32 -> f16-representable f32 values; 0 ok, < 0: H not positive definite (leave the conv to controlled rounding)
int gptq_round_f16(const float* w, int co, int ci, const double* H, double damp, float* out);

// ---- pooling (pool.hip) ------------------------------------------------------------------------
struct PoolP {
  const void* in; int in_cstride, in_coff;
  void* out; int out_cstride, out_coff;
  int B, H, W, C;        // input dims / channels processed
  int Ho, Wo;
  int k, stride, pad;
  int mode;              // 0 = avg (count_include_pad, pad must be 0), 1 = max (-inf padding),
                         // 2 = avg 2x2 s1 p0 followed by max k s p (k,stride,pad describe the max stage; H,W are the raw input)
};
// The kernel a pool launch takes (conv_direct.hip).  choose_pool is pure (no HIP calls): shape, alignment and the rows-per-thread switch
// decide; it throws on the one shape no kernel runs (mode 2 without 16-byte channel chunks or with a max stage other than k3 s2 p1).
enum PoolKernel : int {
  POOL_SCALAR = 0,            // pool_kernel: one thread per (pixel, channel), any channel count / alignment
  POOL_VEC_MAX1 = 1,          // pool_vec_kernel<T, 1, 1>
  POOL_VEC_MAX2 = 2,          // pool_vec_kernel<T, 2, 1>
  POOL_VEC_MAX3 = 3,          // pool_vec_kernel<T, 3, 1>
  POOL_VEC_MAX5 = 4,          // pool_vec_kernel<T, 5, 1>
  POOL_VEC_AVG2 = 5,          // pool_vec_kernel<T, 2, 0>
  POOL_AVG2_ROWS4 = 6,        // avg2_rows_kernel<T, 4>
  POOL_AVG2_ROWS8 = 7,        // avg2_rows_kernel<T, 8>
  POOL_AVGMAX = 8,            // avgmax_pool_kernel
  POOL_AVGMAX_ROWS2 = 9,      // avgmax_rows2_kernel
};
PoolKernel choose_pool(int dt, const PoolP& p);
// cc_dev_set("pool_rows"): output rows per thread of the avg 2x2 / avg-max kernels, as CLEARCAM_POOL_ROWS (8 / 4 / 1); -1 = the environment / default
extern std::atomic<int> g_pool_rows_override;
void launch_pool(int dt, const PoolP& p, hipStream_t stream, PoolKernel* chosen = nullptr);

// CBFuse (detection/yolov9.py:230-245): out = sum_k nearest_upsample(in_k, 2^shift_k) (+ the last, unscaled input)
struct FuseP {
  int n;                                  // inputs (<= 6)
  const void* in[6]; int H[6], W[6], cstride[6], coff[6], shift[6];
  void* out; int out_cstride, out_coff;
  int B, Ho, Wo, C;
};
void launch_fuse(int dt, const FuseP& p, hipStream_t stream);

// ---- detector pre/post (detect.hip) ------------------------------------------------------------
struct PreP {                 // letterbox: detection/yolov9.py:376-379,390-404
  const void* frames; int frame_f32;      // (B,H,W,3) BGR u8 or f32
  int B, H, W;                            // source dims
  int nh, nw, pad_y, pad_x, Hn, Wn;       // resized dims, padding, network dims
  const int* xlo; const int* xhi; const float* xfr;   // per-axis interpolation tables (device)
  const int* ylo; const int* yhi; const float* yfr;
  void* out; int out_c;                   // (B,Hn,Wn,out_c) storage dtype, colour in ch 0..2, rest 0
  int flip;                               // 1: BGR -> RGB (detector), 0: keep the channel order (BlazeFace)
  float div, sub, pad_val;                // inside the image: v / div - sub; in the padding: pad_val
};
void launch_preprocess(int dt, const PreP& p, hipStream_t stream);

// Ragged batch: B frames of different source sizes that letterbox to ONE network shape (Hn, Wn) run as one batch.  Only the letterbox in
// front of the network and scale_boxes behind it know the source size; each reads this per-frame record from device memory, indexed
// by the image index, instead of the single geometry PreP / NmsP carry.  One record per frame, 96 bytes.
struct FrameDesc {
  long long off;                          // byte offset of the frame in the packed buffer (PreP::frames); float32 frames: a multiple of 4
  int H, W, nh, nw, pad_y, pad_x;         // source dims, resized dims, padding
  const int* xlo; const int* xhi; const float* xfr;   // the frame's six axis tables (device; shared by every frame of that size)
  const int* ylo; const int* yhi; const float* yfr;
  float fpad_x, fpad_y, gain, src_w, src_h;           // scale_boxes, computed on the host as the uniform plan computes NmsP's
  int reserved;
};
// PreP of a ragged launch: frames = the packed buffer, B, Hn, Wn, frame_f32, out, flip / div / sub / pad_val; H, W, nh, nw, pads and tables
// are ignored (the records carry them).  packed_bytes = size of the packed buffer.
void launch_preprocess_ragged(int dt, const PreP& p, const FrameDesc* desc, size_t packed_bytes, hipStream_t stream);

// Letterbox fused into the detector's first conv (3x3 stride 2, 3 -> Cout, bias + SiLU): the network-input tensor
// (B,Hn,Wn,8) is never written or read; 16-bit storage types only (detect.hip).
struct StemP {
  PreP pre;                               // pre.out / pre.out_c unused
  const void* w; const float* bias;       // [Cout][32] storage dtype from stem_pack_weights (k = r*9 + s*3 + c, zero for k >= 27), bias f32
  const void* w_lo; float oscale;         // split weights (ConvP::split): the low plane in the same layout and the exact 2^-e output scale; null / ignored otherwise
  int Cout;                               // 16, 32 or 64
  void* out; int out_cstride, out_coff;   // (B,Ho,Wo,out_cstride) storage dtype
  int Ho, Wo;                             // Hn/2, Wn/2
  int abl;                                // timing ablation bits (development only; 0 in production)
};
bool stem_fused_supported(int dt, int Cout);
// reorder the generic conv's packed weights [Cout][w_row] (k = (r*3+s)*tap_stride + plane_off + c; plain: tap_stride = cin_pad, plane_off = 0;
// split: tap_stride = 2*cin_pad, plane_off = 0 / cin_pad for the high / low plane) into the fused kernel's [Cout][32] rows
void stem_pack_weights(int dt, const void* w_packed, int w_row, int tap_stride, int plane_off, int Cout, void* out, hipStream_t stream);
void launch_stem_fused(int dt, const StemP& p, hipStream_t stream);
// The same over a ragged batch (p.pre as launch_preprocess_ragged takes it).  big: the launch's scratch size - stem_needs_big() of any frame
// of the batch (each block still tests whether ITS tile's source rectangle fits the stage and reads the frame directly where it does not).
bool stem_needs_big(int H, int W, int nh, int nw, int frame_f32);
void launch_stem_fused_ragged(int dt, const StemP& p, const FrameDesc* desc, size_t packed_bytes, bool big, hipStream_t stream);
// tinygrad `interpolate(mode='linear', align_corners=False)` index tables for one axis, evaluated in float32 (yolo_run.hip)
void axis_tables(int n_in, int n_out, std::vector<int>& lo, std::vector<int>& hi, std::vector<float>& fr);

struct DecodeP {              // DDetect decode + class max: detection/yolov9.py:209-220,440-448
  const float* raw[3]; int H[3], W[3];    // per level (B,H,W,144) f32
  int B, A;                               // A = sum H*W
  const float* dfl_w;                     // 16 weights
  float conf;                             // 0.25
  float* det;                             // (B,A,6) x1,y1,x2,y2,score(thresholded),cls
  int* nonfinite;                         // device counter: anchors whose logits were not finite (f16 activations past 65504 -> inf -> NaN); may be null
};
void launch_decode(const DecodeP& p, hipStream_t stream);

// DDetect's last 1x1 convs of both branches + decode in one launch (detection/yolov9.py:202-220,247-282): per level the box branch
// cv2[l][2] (1x1, 64 -> 64, four groups densified) and the class branch cv3[l][2] (1x1, ch -> 80) over their 16-bit inputs, then DFL
// softmax-expectation, dist2bbox, sigmoid, class max / argmax, threshold -> (B, A, 6) rows.  The 144 f32 logits per anchor stay on chip.
// Same MFMA accumulation order as the conv kernels and decode_kernel's own arithmetic: bit-identical rows.
struct HeadTailP {
  const void* bx[3]; const void* cl[3];   // (B,H,W,64) and (B,H,W,ch) storage dtype, dense
  const void* w2[3]; const void* w3[3];   // packed [64][kw2] / [80][kw3]
  const float* b2[3]; const float* b3[3];
  int H[3], W[3];
  int kw2, kw3, ch;
  int split; float os2[3], os3[3];        // split weights: rows are [hi(Cin) | lo(Cin)], os2 / os3 the exact 2^-e output scales per level
  int B, A;
  const float* dfl_w; float conf;
  float* det;                             // (B,A,6)
  int* nonfinite;                         // as DecodeP::nonfinite
};
bool head_tail_supported(int dt, int ch, int split = 0);
void launch_head_tail(int dt, const HeadTailP& p, hipStream_t stream);
// ---- batched face path (crop.hip) ----------------------------------------------------------------
// One record per crop of a packed uint8 HWC buffer: ObjectFinder.img_to_face's letterbox to kFaceBox (resize_linear to dh x dw, centred
// in zeros).  face_box_records computes them on the host exactly as the Python does (double arithmetic) and refuses a crop that lies
// outside the buffer or whose letterboxed side would be 0; launch_face_letterbox writes (B, kFaceBox, kFaceBox, 3) uint8.
constexpr int kFaceBox = 640;
struct FaceBoxRec { long long off; int h, w, dh, dw, top, left, area2, reserved; };
void face_box_records(const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B, size_t pix_bytes, std::vector<FaceBoxRec>& rec);
void launch_face_letterbox(const uint8_t* pix_dev, const FaceBoxRec* rec_dev, int B, uint8_t* out_dev, hipStream_t stream);

// ---- shared runtime (runtime.hip) ---------------------------------------------------------------
// Streams of handles come from a process-wide pool per device and go back to it when a handle dies - they are NEVER destroyed.
// Destroying streams makes the runtime re-deal its few hardware queues, and a handle created afterwards has been seen replaying
// its captured graph 3x slower for its whole life ("Uploads"); parked streams keep the queue assignment stable.
hipStream_t pool_stream_get(int device);                 // a non-blocking stream of `device` (the device must be current)
void pool_stream_put(int device, hipStream_t s);         // idle it and park it for the next handle
// batches in flight: streams for the extra slots of a handle, probed until kernels on them overlap with `base` and each other
bool streams_overlap(hipStream_t a, hipStream_t b);
void grow_slot_streams(int device, hipStream_t base, std::vector<hipStream_t>& slots, int n_extra);
// a handle's slots resized to n batches in flight (slot_stream: n - 1 probed streams, slot_done: n events); the caller idles the streams first
void resize_slots(int device, hipStream_t base, std::vector<hipStream_t>& slot_stream, std::vector<hipEvent_t>& slot_done, int n);
// what is enqueued on `waiter` from now on runs after what `signaller` holds now
void order_after(hipStream_t waiter, hipStream_t signaller);
// cc_dev_set("index_slab_rows"): rows per bounced slab of cc_index_remove_* (index.hip); -1 = the default
extern std::atomic<int> g_index_slab_rows;
// cc_dev_set("index_i8_pass"): queries per scan pass over int8 rows (index.hip, 1..8); -1 = the measured default
extern std::atomic<int> g_index_i8_pass;
// cc_dev_set("index_i8_mfma"): the smallest batch that takes the MFMA kernel over int8 rows (index.hip); 0 = never, -1 = the measured default
extern std::atomic<int> g_index_i8_mfma;

// ---- int8 index rows, batches of queries on the matrix cores (index_i8_mfma.hip) ----------------
constexpr int kIndexI8MfmaMaxDim = 4096;                 // wider rows stay with the scan passes (nothing above it has been measured)
bool index_i8_mfma_supported(int dim, long n);           // dim % 256 == 0, dim <= kIndexI8MfmaMaxDim, 1 <= n < 2^31
size_t index_i8_mfma_plane_bytes(int dim, int Q);        // the three bf16 planes of Q queries, padded to a multiple of 16 queries
// out[q][row] (Q, n) f32 = <decoded row, q>: emb = n int8 rows (dim codes + dim / 32 f32 scales each), q = (Q, dim) f32 on the device,
// planes = scratch of index_i8_mfma_plane_bytes(dim, Q).  Two launches on `stream`: the plane split, then the scores.
void launch_index_i8_mfma(const void* emb, const float* q, void* planes, float* out, long n, int dim, int Q, hipStream_t stream);

// ---- stored index rows decoded to f32 (fetch_rows_kernel in index.hip, the Gram tiles in index_distinct.hip) ----
// One 16-byte piece of a stored row -> its floats, the one decode rule of the index: f32 the bytes as they are (4 floats), bf16 the
// 16 bits moved to the high half (8 floats), int8 (float)code * s with s the scale of the piece's group of 32 (16 floats).
#if defined(__HIPCC__)
__device__ __forceinline__ float i8_code(unsigned w, int b) { return (float)((int)(w << (24 - 8 * b)) >> 24); }
__device__ __forceinline__ void decode_bf16_piece(const uint4 v, float4* o) {
  o[0] = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
  o[1] = make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xffff0000u), __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xffff0000u));
}
__device__ __forceinline__ void decode_i8_piece(const uint4 v, float s, float4* o) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = make_float4(i8_code(w[k], 0) * s, i8_code(w[k], 1) * s, i8_code(w[k], 2) * s, i8_code(w[k], 3) * s);
}
#endif

// ---- which rows compete (index.hip's rankings, index_digest.hip's selection) -----------------------------------------------------
constexpr int kRowNoTs = INT32_MIN;                      // CC_ROW_NO_TS
// cc_row_filter as the kernels take it (by value, in the kernel arguments): a null column = no filter on that attribute.
// dead: one byte per row, non-zero = the row is out of the running (cc_index_rank_like's exclusion and cc_index_rank_terms' REQUIRE /
// REJECT terms and exclusion, both written by terms_fold_kernel); null everywhere else.
struct RowWhere { const int* ts; const int* cls; int ts_min, ts_max; unsigned long long m0, m1, m2, m3; const unsigned char* dead; };
#if defined(__HIPCC__)
__device__ __forceinline__ bool row_allowed(const int* __restrict__ grp, const unsigned char* __restrict__ allowed, int n_allowed, long r) {
  if (!allowed) return true;
  const unsigned g = (unsigned)grp[r];
  return g < (unsigned)n_allowed && allowed[g];
}

// The row competes: its group is allowed, it has the attributes the filter asks for, and it is not dead.  The mask word is chosen by
// compares, not by an index, so the four words stay in scalar registers.
__device__ __forceinline__ bool row_passes(const int* __restrict__ grp, const unsigned char* __restrict__ allowed, int n_allowed, const RowWhere& w, long r) {
  if (!row_allowed(grp, allowed, n_allowed, r)) return false;
  if (w.dead && w.dead[r]) return false;
  if (w.ts) {
    const int t = w.ts[r];
    if (t == kRowNoTs || t < w.ts_min || t > w.ts_max) return false;
  }
  if (w.cls) {
    const unsigned c = (unsigned)w.cls[r];
    if (c > 255u) return false;                                    // -1: no class
    const unsigned long long m = c < 128u ? (c < 64u ? w.m0 : w.m1) : (c < 192u ? w.m2 : w.m3);
    if (!((m >> (c & 63u)) & 1ull)) return false;
  }
  return true;
}
#endif

// ---- distinct ranking: pairwise similarities of stored rows and the greedy thinning of ranked lists (index_distinct.hip) ----
constexpr int kDistinctMaxDepth = 1024;                  // CC_DISTINCT_MAX_DEPTH: rows of one Gram matrix, entries of one list
constexpr int kDistinctWords = kDistinctMaxDepth / 64;   // 64-bit words in one row of a list's bit matrix
// Device scratch of a thinning of Q lists: per list the squeezed rows (int64), their places in the list (int32) and the bit matrix; then
// per list the number of present entries (int32) and of kept ones (int64).  The offsets are distinct_ws's.
struct DistinctWs { long long* rows; int* pos; unsigned long long* bits; int* present; long long* kept; };
size_t distinct_ws_bytes(int Q);
DistinctWs distinct_ws(void* base, int Q);
// out (n, n) f32 = <row rows[i], row rows[j]> of the stored rows decoded as fetch_rows_kernel decodes them; rows: n numbers the device
// can read, each inside [0, size) or the row counts as zeros.  One launch.
void launch_index_gram(const void* emb, long size, int dim, int storage, const long long* rows, int n, float* out, hipStream_t stream);
// idx (Q, depth) -> out_idx / out_score / out_dups (Q, count) and ws.kept, all on the device (score, out_score, out_dups may be null).
// Three launches on `stream`: squeeze, Gram tiles compared with same_at into ws.bits, the walk.
void launch_index_distinct(const void* emb, long size, int dim, int storage, const int* idx, const float* score, int Q, int depth, float same_at,
                           long long start, long long count, const DistinctWs& ws, int* out_idx, float* out_score, int* out_dups, hipStream_t stream);
// The compare epilogue alone over ONE list of n <= kDistinctMaxDepth rows the device can read: bits[i][j >> 6] bit j & 63 = (<row i, row j> >= same_at)
// for the 64 x 64 tiles at and above the diagonal, the float being the one launch_index_gram stores.  One launch.
void launch_index_gram_bits(const void* emb, long size, int dim, int storage, const long long* rows, int n, unsigned long long* bits, float same_at,
                            hipStream_t stream);

// ---- day digest: leader clustering of the competing rows in row order (index_digest.hip) ----
constexpr int kDigestMaxLeaders = 1024;                  // CC_DIGEST_MAX_LEADERS
constexpr int kDigestChunk = 1024;                       // competing rows per piece: one bit matrix, one walk
// Device scratch of one digest (the offsets are digest_ws's): the competing rows in order, the per-block counts and offsets of the
// selection, the two bit matrices of a piece, the leader tables and the counters.
struct DigestWs {
  long long* sel;                                        // (n) competing row numbers, ascending; the first *m are valid
  unsigned* bcnt; unsigned* boff;                        // (blocks of 1024 rows) competing rows in / before each block
  unsigned long long* bits_lead;                         // (1024, 16) piece rows x leaders
  unsigned long long* bits_self;                         // (1024, 16) piece rows x piece rows
  long long* lead_row;                                   // (1024) leaders in order of creation
  int* lead_cnt; int* lead_ts_min; int* lead_ts_max;     // (1024) members, and the extremes of their ts (INT32_MAX / INT32_MIN: none yet)
  int* n_lead; int* m;                                   // leaders so far; competing rows
  long long* totals;                                     // leaders, competing rows, left-over rows
};
size_t digest_ws_bytes(long n);
DigestWs digest_ws(void* base, long n);
// Competing rows of [0, n) -> ws.sel / ws.m, tables and counters cleared; owner (may be null): -1 for every row that does not compete.
// Three launches.  RowWhere / allowed as rank_keys_kernel takes them.
void launch_digest_select(long n, const int* grp, const unsigned char* allowed, int n_allowed, const RowWhere& where, const DigestWs& ws, int* owner,
                          hipStream_t stream);
// One piece: rows ws.sel[first .. first + len), len <= kDigestChunk.  Three launches: piece x leaders tiles, piece x piece tiles, the walk.
void launch_digest_piece(const void* emb, long size, int dim, int storage, long first, int len, float same_at, int max_leaders, const int* ts,
                         const DigestWs& ws, int* owner, hipStream_t stream);
// Sort the leaders by `order` (CC_DIGEST_BY_*), write entries start .. start + count - 1 and the padding behind them, and ws.totals.
void launch_digest_finish(const DigestWs& ws, int order, long long start, long long count, int* out_row, int* out_count, int* out_ts_first,
                          int* out_ts_last, hipStream_t stream);

// ---- seen before: up to 1024 stored rows against all competing rows, reduced per object (index_sightings.hip) ----
constexpr int kSightMaxObjects = 1024;                   // CC_SIGHT_MAX_OBJECTS
constexpr int kSightMaxGroups = 4096;                    // CC_SIGHT_MAX_GROUPS
// sel / m: the competing rows and their number on the device (launch_digest_select); obj: n_obj row numbers on the device, each inside
// [0, size).  out_count (n_obj) and gc (n_obj, n_gc; null with n_gc 0) are ADDED to and `best` (n_obj keys) is RAISED: the caller zeroes
// all three first.  out_best_row / out_best_score (n_obj, either may be null) are written from `best`.  Two launches (one with both null).
void launch_sightings(const void* emb, long size, int dim, int storage, const long long* sel, const int* m, const long long* obj, int n_obj, float same_at,
                      int skip_self, const int* grp, int n_gc, int* out_count, unsigned long long* best, unsigned* gc, int* out_best_row,
                      float* out_best_score, hipStream_t stream);

// ---- together: rows with a partner nearby in time (index_near.hip) ----
constexpr int kNearMaxPartners = 16384;                  // CC_NEAR_MAX_PARTNERS
// The partner list on the device, kNearMaxPartners entries a column (the offsets are near_list's): row and score as the ranking's emit
// kernel writes them (-1 / -inf behind the last entry), then what launch_near_pack reads beside each row.
struct NearList { int* row; int* grp; int* ts; int* trk; float* score; };
size_t near_list_bytes();
NearList near_list(void* base);
// L.row[0 .. cap) -> L.grp / L.ts / L.trk.  One launch.
void launch_near_pack(const NearList& L, int cap, long n, const int* grp, const int* ts, const int* trk, hipStream_t stream);
// S[0 .. n) = Sa -> v in place, dead (n bytes) and pos (n int32: the partner's place in the list, -1 none).  n_list: one word on the
// device, the rows the list would hold without the cap.  where_a / allowed as rank_keys_kernel takes them (where_a.dead null); skip_cut:
// a row with Sa < min_score may skip the walk (a ranking without track reduction).  One launch.
void launch_near_fold(float* S, long n, const int* grp, const int* trk, const int* ts, const unsigned char* allowed, int n_allowed, const RowWhere& where_a,
                      float min_score, int skip_cut, const NearList& L, const unsigned* n_list, int cap, int within, int value, unsigned char* dead, int* pos,
                      hipStream_t stream);
// partner / partner_score (cnt each, either may be null) of the answers idx names; -1 / -inf where idx is -1.  One launch.
void launch_near_gather(const int* idx, const int* pos, const NearList& L, long n, size_t cnt, int cap, int* partner, float* partner_score, hipStream_t stream);

struct NmsP {                 // top-300 + mask NMS + scale_boxes: detection/yolov9.py:406-458
  const float* det; int B, A;
  float iou_thr;
  float pad_x, pad_y, gain; float src_w, src_h;
  float* out;                             // (B,300,6)
};
void launch_topk_nms(const NmsP& p, hipStream_t stream);
// Ragged batch: image b's pad / gain / source size come from desc[b] (p's own are ignored).  `desc` is read when the kernel RUNS: inside a
// captured graph it is a fixed device address whose contents the caller refreshes before each replay.
void launch_topk_nms_ragged(const NmsP& p, const FrameDesc* desc, hipStream_t stream);

// ---- CLIP towers (clip_kernels.hip) -------------------------------------------------------------
// Plain GEMM through the conv kernel:  out[M][N] = act(A[M][K] W[N][K]^T + bias) (+res).
ConvP gemm_params(const void* A, int lda, int M, int K, const void* W, int ldw, const float* bias, int N, void* out, int ldc,
                  int out_f32, int act, const void* res, int ldres, int res_f32);

struct LnP {                  // LayerNorm(eps 1e-5, biased var, affine): models/objects.py:105,123,129,153,176,182
  const float* in; long in_row_stride; const int* row_index;   // row r reads in + (row_index ? row_index[r] : r) * in_row_stride
  const float* w; const float* b;
  void* out; int out_f32;     // [rows][D]
  int rows, D;
};
void launch_layernorm(int dt, const LnP& p, hipStream_t stream);

struct PatchP { const float* x; void* out; int B, S, patch, Kpad; };   // (B,3,S,S) f32 -> (B*g*g, Kpad), k = c*p*p + kh*p + kw
void launch_patchify(int dt, const PatchP& p, hipStream_t stream);

struct AssembleP {            // cat(class_embedding, patches) + positional_embedding -> ln_pre   (objects.py:98-102)
  const void* patches;        // (B*(L-1), D) storage dtype
  const float* cls; const float* pos; const float* w; const float* b;
  float* out;                 // (B*L, D) f32 residual stream
  int B, L, D;
};
void launch_assemble_ln(int dt, const AssembleP& p, hipStream_t stream);

struct EmbedP { const int* tokens; const float* table; const float* pos; float* out; int B, L, D; };   // objects.py:148-149
void launch_embed(const EmbedP& p, hipStream_t stream);

struct AttnP {                // softmax(q k^T / sqrt(dh)) v per head, dh = 64   (objects.py:110-119,160-171)
  const void* qkv;            // (B*L, 3*D) storage dtype: [q | k | v]
  void* ctx;                  // (B*L, D)
  int B, L, H, D; int causal; float scale;
  int abl;                    // development (cc_attn_bench): 1 = stage K / V only, 2 = no staging (tiles over whatever LDS holds), 32 = empty blocks,
                              // 64 = print the occupancy, 128 = one query tile per wave round instead of two; 0 in production
};
void launch_attention(int dt, const AttnP& p, hipStream_t stream);

struct NormP { float* x; int rows, D; float eps; };   // x / (||x||_2 + eps)   (objects.py:132,186)
void launch_l2norm(const NormP& p, hipStream_t stream);

}  // namespace cc
