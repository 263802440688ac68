/* libclearcam_hip — C ABI of the MI355X-native detect / CLIP-encode / search path for clearcam.
 *
 * The reference (roryclear/clearcam) has no FFI for this path: its boundary is three duck-typed Python
 * call surfaces that sit directly on tinygrad.  Each entry point below names the reference interface
 * it stands behind; the Python shim in clearcam_amd/ keeps those surfaces byte-compatible and
 * INTEGRATION.md shows the ctypes binding a clearcam maintainer would add.
 *
 * Conventions: every function returns 0 on success or a negative errno-style code, with a thread-local
 * message available from cc_last_error().  The caller owns every buffer it passes.  A handle belongs to
 * one GPU and one submitting thread at a time (the reference runs all tensor work on its main thread,
 * clearcam.py:1214-1226).  `stream` is a hipStream_t (NULL = the handle's own stream); when results
 * go to host memory the call returns after they have landed, otherwise it only enqueues work.
 */
#ifndef CLEARCAM_HIP_H
#define CLEARCAM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CC_DTYPE_F32 0   /* parity mode: f32 storage, exact-f32 MFMA (157 TFLOP/s class)                                             */
#define CC_DTYPE_F16 1   /* speed mode:  f16 storage (activations AND weights rounded to 11 bits), f32 accumulate                    */
#define CC_DTYPE_BF16 2  /* speed mode:  bf16 storage (8 bits), f32 accumulate                                                       */
#define CC_DTYPE_F16S 3  /* tolerance mode at MFMA rate (detector only): f16 activations, every conv weight carried as */
                         /* TWO f16 planes W = W_hi + W_lo (~22 bits) multiplied into the same f32 accumulator - detections stay      */
                         /* within the reference tolerance for any float32 checkpoint at twice the MFMA issue of CC_DTYPE_F16        */
#define CC_DTYPE_F16H 4  /* CC_DTYPE_F16S where it is needed: two planes for the 1x1 convs of the detector's backbone (blocks up to the     */
                         /* SPPELAN) and the stem conv, one controlled-rounded f16 plane for every other conv (controlled rounding balances  */
                         /* a 3x3 filter's taps; a 1x1 has nothing to balance).  Measured as close to f32 as CC_DTYPE_F16S on un-rounded      */
                         /* checkpoints at 1.15x instead of 2x the MFMA issue of CC_DTYPE_F16 (bench default)                              */

#define CC_DTYPE_F16C 5  /* calibrated mode (detector only): one f16 plane per conv (two in the stem conv), the 1x1 convs' weights rounded with    */
                         /* the errors steered by their inputs' second moments on calibration frames (cc_yolo_calibrate): CC_DTYPE_F16's rate     */

#define CC_MAX_DET 300   /* rows per frame of the detector output (detection/yolov9.py:439) */

const char* cc_last_error(void);
int cc_version(void);
int cc_device_count(int* n);

/* ---------------------------------------------------------------------------------------------
 * Detector — stands behind `YOLOv9(size, res)` and `YOLOv9.__call__(frame)`
 * (detection/yolov9.py:298-388), as called from clearcam.py:583 and test/run_mot.py:34.
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_yolo cc_yolo;

/* YOLOv9.__init__ (yolov9.py:298-371): size in {"t","s","m","c","e"}, res = letterbox target. */
int cc_yolo_create(cc_yolo** h, const char* size, int res, int dtype, int device);
/* load_state_dict (yolov9.py:372-373): one call per state-dict entry, reference key names
 * (SURVEY.md Appendix C), host float32 data, OIHW weights / (Cout,) biases. */
int cc_yolo_load(cc_yolo* h, const char* name, const float* data, const int64_t* shape, int ndim);
/* Packs the loaded tensors into the device layout ([Cout][kh][kw][Cin], storage dtype). Fails if
 * any parameter of the graph is missing. */
int cc_yolo_finalize(cc_yolo* h);
/* dtype 5 ("f16c"): f16 activations and ONE f16 weight plane per conv (two in the stem conv), the 1x1 convs' float32 weights rounded to
 * f16 by a calibration-aware recursion (GPTQ: rounding errors steered by the second moments of each conv's own input) that cc_yolo_finalize
 * runs on an internal float32 pass over calibration frames: plain f16's frame rate, "f16h"'s tolerance on inputs like the calibration
 * frames (INTEGRATION.md says what was measured with mismatched ones).  cc_yolo_calibrate hands over the frames ((B,H,W,3) BGR uint8 or
 * float32 HOST memory, copied) between cc_yolo_load and cc_yolo_finalize; without it four frames of seeded white noise are used.
 * cc_yolo_calibration_info: packed 1x1 convs the recursion rounded / left to the plain controlled rounding (singular second moments). */
int cc_yolo_calibrate(cc_yolo* h, const void* frames, int B, int H, int W, int frame_f32);
int cc_yolo_calibration_info(cc_yolo* h, int* n_calibrated, int* n_fallback);
/* Host-only helper (no GPU needed; tests): the recursion itself - w (cout,cin) float32, H (cin,cin) float64 second moments of the input,
 * damp (ridge on H as a share of its mean diagonal; 0.03 in the library) -> out (cout,cin) float32 values exactly representable in f16. */
int cc_gptq_round_f16(const float* w, int64_t cout, int64_t cin, const double* H, double damp, float* out);
/* YOLOv9.__call__ (yolov9.py:375-388) over a batch: frames (B,H,W,3) BGR, uint8 (frame_f32=0, the
 * production path clearcam.py:582) or float32 (frame_f32=1, the MOT path run_mot.py:33);
 * out (B,300,6) float32 [x1,y1,x2,y2,conf,cls] in source-frame pixels, suppressed rows zero.
 * B=1 is exactly the reference call.  frames_on_device/out_on_device select host or device pointers. */
int cc_yolo_detect(cc_yolo* h, const void* frames, int B, int H, int W, int frame_f32,
                   int frames_on_device, float* out, int out_on_device, void* stream);
/* Range guard of the 16-bit modes: f16 activations saturate at 65504, and a checkpoint that drives them past it yields inf -> NaN logits,
 * which every threshold silently turns into "no detection".  The decode stage counts anchors whose logits were not finite: a
 * cc_yolo_detect call that returns its rows to HOST memory fails with -34 (ERANGE) and a message naming the remedy (dtype bf16 / f32) when
 * the count is non-zero; for device-output and cc_yolo_submit calls cc_yolo_nonfinite waits for the handle's streams and returns (and
 * clears) the count accumulated since the last query. */
int cc_yolo_nonfinite(cc_yolo* h, int* count);
/* Batches in flight - throughput mode for a GPU that serves many cameras (no counterpart in the reference, whose loop is one
 * synchronous batch-1 call per frame, clearcam.py:583).  cc_yolo_set_in_flight(h, n) gives the handle n slots (1..8, default 1), each
 * with its own stream, tensor arena and captured graph (the streams are probed until kernels on them really run side by side);
 * cc_yolo_submit runs one batch on the next slot (round robin), ordered after `stream` (where the caller produced device frames;
 * may be NULL) but WITHOUT making `stream` wait for the result, so the next submission's first layers - and its upload - overlap
 * this one's last; cc_yolo_wait(h, ticket, stream) makes `stream` (NULL: the calling thread) wait until that submission's
 * (B,300,6) rows are in `out`.  frames / out may be host pointers (frames_on_device / out_on_device = 0; pinned memory, or the copies
 * are not asynchronous): upload, detect and download then form one in-order chain on the slot's stream.  Results are bit-identical
 * to cc_yolo_detect.  `frames` must stay valid until the submission has completed; `out` buffers of submissions in flight must be
 * distinct.  Changing the depth drops the cached plans. */
int cc_yolo_set_in_flight(cc_yolo* h, int n);
int cc_yolo_submit(cc_yolo* h, const void* frames, int B, int H, int W, int frame_f32, int frames_on_device, float* out,
                   int out_on_device, void* stream, long long* ticket);
int cc_yolo_wait(cc_yolo* h, long long ticket, void* stream);
/* Ragged batch - one GPU serving cameras of DIFFERENT resolutions (the reference reads every stream's size separately,
 * clearcam.py:145, :403).  The network only sees the letterboxed shape: at res 640, 1080x1920, 720x1280, 2160x3840 and 360x640 all become
 * 384x640.  B frames of any source sizes that share ONE network shape run as one batch of that shape's plan; only the letterbox in front
 * of the network and scale_boxes behind it read a per-frame record.  Packed-buffer convention of cc_crop_preprocess: frame b is
 * heights[b] x widths[b] x 3 (BGR, all uint8 or all float32 - then offsets are multiples of 4), starting at byte offsets[b] of `pixels`;
 * the three tables are HOST arrays and are consumed before the call returns.  Row b of `out` is bit-identical to what cc_yolo_detect
 * returns for frame b alone.  -22 (EINVAL) with a message naming the frame when the frames do not share one network shape or that shape
 * is not a multiple of 32.  The plan is keyed by (B, network shape, element type, slot): a camera that changes resolution reuses it.
 * cc_yolo_submit_ragged / cc_yolo_wait are to cc_yolo_detect_ragged what cc_yolo_submit is to cc_yolo_detect (same rows, bit for bit);
 * `pixels` must stay valid until the submission has completed.  cc_yolo_get_tensor, cc_yolo_last_gpu_ms and cc_yolo_nonfinite work
 * after a ragged call as after a uniform one; cc_yolo_profile / cc_yolo_profile_graph refuse a ragged plan. */
int cc_yolo_detect_ragged(cc_yolo* h, const void* pixels, const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B,
                          int frame_f32, int pixels_on_device, float* out, int out_on_device, void* stream);
int cc_yolo_submit_ragged(cc_yolo* h, const void* pixels, const int64_t* offsets, const int32_t* heights, const int32_t* widths, int B,
                          int frame_f32, int pixels_on_device, float* out, int out_on_device, void* stream, long long* ticket);
/* Host-only helper (no GPU needed): the letterbox of an H x W frame at target `res` (yolov9.py:390-403) - resized size nh x nw and the
 * padding per side; the network shape is (nh + 2 pad_y) x (nw + 2 pad_x).  What the ragged entry points group by. */
int cc_letterbox_geometry(int H, int W, int res, int* nh, int* nw, int* pad_y, int* pad_x);
/* Plans (tensor arena + captured graph) the handle has built so far: a call that finds its plan in the cache leaves it unchanged. */
int cc_yolo_plans_built(cc_yolo* h, int* n);
/* Parity taps: copy a named intermediate of the LAST detect call to host float32.
 * names: "input" (B,Hn,Wn,3) | "p3","p4","p5" (B,H,W,C) | "raw0","raw1","raw2" (B,H,W,144) |
 * "decoded" (B,A,6).  shape receives up to 4 dims; pass out=NULL to query the shape only.
 * In the 16-bit modes the letterbox is fused into the first conv and "input" is rebuilt on demand, and cc_yolo_profile
 * re-runs that kernel: for both, device frames handed to the last cc_yolo_detect call must still be alive (host frames are
 * staged in a buffer the handle owns). */
int cc_yolo_get_tensor(cc_yolo* h, const char* name, float* out, int64_t* shape, int* ndim);
/* The same for frames [b0, b0 + nb) only: shape[0] = nb, and only those frames are copied and converted (a tap of a B = 64 plan can
 * be several GB as float32).  A range outside [0, B) is an error.  "decoded" and "input" behave as in cc_yolo_get_tensor. */
int cc_yolo_get_tensor_frames(cc_yolo* h, const char* name, int b0, int nb, float* out, int64_t* shape, int* ndim);
/* GPU milliseconds of the last detect call's kernels (hipEvents on the launch stream). */
int cc_yolo_last_gpu_ms(cc_yolo* h, float* ms);
/* Eager replay of the last plan's launch list, `iters` times, with a hipEvent pair around every launch
 * on the launch stream.  ms[5] = average per-step milliseconds of {conv/GEMM, pooling, decode, top-k+NMS, fused letterbox +
 * first conv (0 when that fusion is off: f32 mode or CLEARCAM_FUSE_STEM=0; its time is then in the conv slot and in the
 * separate letterbox launch)}; alg_macs_per_step / n_conv_launches cover the launches timed in the conv slot. */
int cc_yolo_profile(cc_yolo* h, int iters, float* ms, double* alg_macs_per_step, int* n_conv_launches);
/* A subset of the last plan's launch list captured into a hipGraph of its own and replayed `iters` times between ONE hipEvent
 * pair on the launch stream (no per-launch event records): average milliseconds per replay.
 * which = 0: the conv / GEMM launches (the ones cc_yolo_profile counts in its conv slot), 1: every other launch (pooling, decode,
 * top-k + NMS, CBFuse, and the fused letterbox + first conv), 2: the whole step. */
int cc_yolo_profile_graph(cc_yolo* h, int iters, int which, float* ms_per_replay);
void cc_yolo_destroy(cc_yolo* h);

/* Single-layer entry used by the parity tests: NHWC conv + bias + optional SiLU on device buffers.
 * x (B,H,W,Cin) and out (B,Ho,Wo,Cout) in storage dtype `dtype`; w OIHW float32 host, bias host.
 * groups>1 is densified to block-diagonal weights exactly as the detector does for the head convs.
 * force_direct selects the kernel: 0 = what the detector would pick, 1 = direct (non-MFMA) fallback, 2 = generic MFMA
 * implicit GEMM, 4 = weights-stationary 3x3, ... 10 = weights-resident streaming 1x1, 12 = 3x3 64 -> 64 tile kernel (ConvVariant in
 * csrc/conv_select.h lists them all; the specialised ones fail if the shape is not eligible, a value that names no kernel fails). */
int cc_conv2d_nhwc(int dtype, const void* x_dev, int B, int H, int W, int Cin, const float* w_oihw,
                   const float* bias, int Cout, int k, int stride, int groups, int act, void* out_dev,
                   int force_direct, void* stream);
/* Single-layer entry of the epilogue tests: ONE launch of any conv the CLIP, AdaFace and BlazeFace plans describe.
 * dtype 0 / 1 / 2 (f32 / f16 / bf16 storage); x (B,H,W,Cin) in the storage type; w OIHW float32 host (Cout, Cin/groups, k, k), packed
 * as the face nets pack theirs (groups densified, converted to the storage type: values already representable there are kept as they
 * are); bias, slope: host float32[Cout] or null (slope is required for act 3).
 * act: 0 none, 1 SiLU, 2 tanh-GELU, 3 PReLU (before the residual), 4 ReLU (after the residual).
 * pad < 0: k/2.  Ho / Wo <= 0: (H + 2 pad - k) / stride + 1; larger values add zero rows / columns at the bottom / right.
 * out: pixels of out_cstride channels (<= 0: Cout), the result in channels [out_coff, out_coff + Cout), float32 if out_f32 else the
 * storage type.  res (null: none): the same pixel grid, res_cstride (<= 0: Cout) / res_coff, float32 if res_f32; it may be `out` itself.
 * variant: as cc_conv2d_nhwc's force_direct.  choice (int[4] or null) receives the kernel that ran: ConvKernel, phase schedule, tile
 * pixels, tile channels (csrc/conv_select.h).  Synchronises the stream.
 * cc_conv2d_ex_route: the same launch, choice (int[8] or null) receiving those four and then what picks the K loop: simple, two, cprw
 * (16-byte chunks per LDS row), ns (LDS stages) - the eight ints cc_dev_conv_det reports.  An entry of its own so that cc_conv2d_ex
 * never writes past the four ints its callers hand it. */
typedef struct {
  int dtype, B, H, W, Cin, Cout, k, stride, groups, act;
  int pad, Ho, Wo;
  int out_f32, out_cstride, out_coff;
  int res_f32, res_cstride, res_coff;
  int variant;
} cc_conv_desc;
int cc_conv2d_ex(const cc_conv_desc* d, const void* x_dev, const float* w_oihw, const float* bias, const float* slope,
                 const void* res_dev, void* out_dev, int* choice, void* stream);
int cc_conv2d_ex_route(const cc_conv_desc* d, const void* x_dev, const float* w_oihw, const float* bias, const float* slope,
                       const void* res_dev, void* out_dev, int* choice, void* stream);
/* Single-launch entries of the post-processing tests: ONE launch of a detector / face post-processing kernel through its production
 * launcher, on inputs the caller crafts.  Device pointers end in _dev; everything else is host memory.  Each validates its arguments
 * (an error, and no launch, on null pointers, B <= 0, an empty level, an unsupported dtype / ch, or a misaligned map), synchronises
 * `stream` and frees what it allocated.  H, W: int[3], the three levels' map sizes (strides 8, 16, 32), A = sum H*W.
 *
 * cc_dev_decode: decode_kernel.  raw_dev[3]: float32 (B,H_l,W_l,144) maps, 16-byte aligned; dfl_w16: the 16 DFL weights; det_dev
 * (B,A,6) rows [x1,y1,x2,y2,score (0 below conf),class]; *nonfinite: anchors whose logits were not finite.
 * cc_dev_head_tail: head_tail_kernel.  dtype 1 / 2 / 3 (f16 / bf16 / f16s), ch 128 or 256; per level bx_dev (B,H,W,64) and cl_dev
 * (B,H,W,ch) in the storage type, 16-byte aligned, and the OIHW float32 weights of cv2[l][2] (64,16,1,1: four groups) and cv3[l][2]
 * (80,ch,1,1) with their biases, packed as the detector packs them (groups densified, controlled rounding, two planes for f16s).
 * cc_dev_topk_nms: topk_nms_kernel over rows_dev (B,A,6) -> out_dev (B,300,6).  geometry = (pad_x, pad_y, gain, src_w, src_h) of
 * scale_boxes: 5 floats (ragged = 0), or B x 5 (ragged = 1: the ragged launcher, frame records with only these fields filled).
 * cc_dev_blaze_post: blaze_post_kernel over float32 head outputs r8 (B,16,16,32), r16 (B,8,8,96), c8 (B,16,16,2), c16 (B,8,8,6) and
 * host anchors (896,4) -> out_dev (B,896,17), first_dev (B,17), first_idx_dev (B) as cc_blaze_detect_batch / cc_face_locate produce
 * them. */
int cc_dev_decode(const float* const* raw_dev, const int* H, const int* W, int B, const float* dfl_w16, float conf, float* det_dev,
                  int* nonfinite, void* stream);
int cc_dev_head_tail(int dtype, int ch, const void* const* bx_dev, const void* const* cl_dev, const float* const* w2, const float* const* b2,
                     const float* const* w3, const float* const* b3, const int* H, const int* W, int B, const float* dfl_w16, float conf,
                     float* det_dev, int* nonfinite, void* stream);
int cc_dev_topk_nms(const float* rows_dev, int B, int A, float iou_thr, const float* geometry, int ragged, float* out_dev, void* stream);
int cc_dev_blaze_post(const float* r8_dev, const float* r16_dev, const float* c8_dev, const float* c16_dev, int B, const float* anchors,
                      float scale, int pad_top, int pad_left, float* out_dev, float* first_dev, int32_t* first_idx_dev, void* stream);
/* Single-launch entries of the CLIP kernel tests: ONE launch of a CLIP tower kernel other than the GEMMs through its production launcher
 * (launch_attention, launch_layernorm, launch_assemble_ln, launch_patchify, launch_embed, launch_l2norm).  Every tensor is a device
 * pointer the caller owns (the entries allocate nothing, so alignment and buffer size are the caller's; only cc_dev_embed takes HOST
 * tokens and holds a device copy for the call).  Each validates its arguments (an error, and no launch, on null pointers, non-positive
 * sizes, an unsupported dtype, or what the launcher itself refuses) and synchronises `stream`.  dtype 0 / 1 / 2 = f32 / f16 / bf16.
 *
 * cc_dev_attention: qkv_dev (B*L, 3*D) and ctx_dev (B*L, D) in the storage type, D = 64*H; 1 <= L <= 288, scale > 0; f16 / bf16 run
 * attn_mfma_kernel (qkv_dev 16-byte, ctx_dev 8-byte aligned), f32 attn_simple_kernel.
 * cc_dev_layernorm: row r reads in_dev + (row_index_dev ? row_index_dev[r] : r) * in_row_stride (float32, D <= 1024) and writes row r
 * of out_dev (rows, D): float32 when out_f32, else the storage type.
 * cc_dev_assemble_ln: patches_dev (B*(L-1), D) in the storage type, cls_dev (D), pos_dev (L, D), LayerNorm w_dev / b_dev (D) -> out_dev
 * (B*L, D) float32; D <= 1024.
 * cc_dev_patchify: x_dev float32 (B,3,S,S) -> out_dev (B*g*g, Kpad) in the storage type, g = S / patch; S % patch == 0,
 * Kpad >= 3*patch*patch, columns past 3*patch*patch zero.
 * cc_dev_embed: tokens HOST int32 (B,L), each checked against vocab before anything is uploaded; table_dev (vocab, D), pos_dev (L, D)
 * -> out_dev (B*L, D), all float32.
 * cc_dev_l2norm: x_dev float32 (rows, D) in place, x / (||x|| + eps); eps >= 0. */
int cc_dev_attention(int dtype, const void* qkv_dev, int B, int L, int H, int causal, float scale, void* ctx_dev, void* stream);
int cc_dev_layernorm(int dtype, const float* in_dev, long long in_row_stride, const int32_t* row_index_dev, const float* w_dev, const float* b_dev,
                     void* out_dev, int out_f32, int rows, int D, void* stream);
int cc_dev_assemble_ln(int dtype, const void* patches_dev, const float* cls_dev, const float* pos_dev, const float* w_dev, const float* b_dev,
                       float* out_dev, int B, int L, int D, void* stream);
int cc_dev_patchify(int dtype, const float* x_dev, void* out_dev, int B, int S, int patch, int Kpad, void* stream);
int cc_dev_embed(const int32_t* tokens, int vocab, const float* table_dev, const float* pos_dev, float* out_dev, int B, int L, int D, void* stream);
int cc_dev_l2norm(float* x_dev, int rows, int D, float eps, void* stream);
/* Single-launch entries of the glue-kernel tests: ONE launch of a kernel that sits between the convs, through its production launcher, on
 * device buffers the caller crafts.  Each validates its arguments (an error, and no launch, on null pointers, non-positive sizes, a
 * channel view outside its buffer, windows outside the input, or whatever the launcher itself refuses) and synchronises `stream`.
 * What a launcher refuses is refused before the first HIP call.  dtype 0 / 1 / 2 = f32 / f16 / bf16.
 *
 * cc_dev_pool: launch_pool over channels [in_coff, in_coff + C) of a (B,H,W,in_cstride) buffer into channels [out_coff, out_coff + C)
 * of a (B,Ho,Wo,out_cstride) one.  mode 0 = average (pad 0, windows inside the input), 1 = max with -inf padding, 2 = the 2x2 stride-1
 * average followed by the max (k, stride, pad describe the max stage: only 3 / 2 / 1 runs).  *kernel (may be null) receives the
 * PoolKernel that ran (csrc/kernels.h): 0 scalar, 1-4 vector max k = 1 / 2 / 3 / 5, 5 vector avg 2x2, 6 / 7 avg 2x2 with four / eight rows per
 * thread, 8 avg-max, 9 avg-max with two rows per thread.
 * cc_dev_pool_choice: the same arguments and the same validation, no launch and no HIP call: *kernel = what cc_dev_pool would run.
 * cc_dev_fuse: launch_fuse (CBFuse): out = sum over the n <= 6 inputs of input i read at (ho >> shift[i], wo >> shift[i]); arrays of n
 * entries; every pointer 16-byte aligned, C / coff / cstride whole 16-byte chunks (else refused).
 * cc_dev_conv_src: ONE conv over the channel concat of two source views (s1 null: one source), each read as it is (shift 0), nearest-
 * upsampled by 2^shift, or - first source alone - through its 2x2 stride-1 average (shift -1: conv_adown.hip, 16-bit storage, 3x3 stride 2,
 * Cin a multiple of 64).  d: dtype 0 .. 3 (3 = f16 storage, split weights), H x W = the conv's logical input, Cin = s0.C + s1.C,
 * groups 1, act 0 .. 2, no residual; w OIHW float32 and bias host arrays, packed as the detector packs them (controlled rounding: values
 * already representable are kept; two planes for dtype 3).  choice (int[6] or null) receives ConvKernel, phase schedule, tile pixels,
 * tile channels, simple loader, two-source eight-wave loader (csrc/conv_select.h); the averaging kernel reports CC_DEV_CONV_ADOWN,
 * 0, 128, its channel tile (64 / 128), 0, 0.
 * cc_dev_conv_det: the same launch as the detector's plans build it: the same two views and descriptor, and also d->groups (weights
 * (Cout, Cin / groups, k, k), densified to block-diagonal rows as the detector packs its DDetect box branch) and a residual res_dev (null:
 * none) read through d->res_f32 / res_cstride / res_coff on the output's pixel grid, added after the activation.  res_dev may be out_dev
 * (RepNBottleneck's x + cv2(cv1(x)) in place) when it is the output's own view (same type, cstride and coff); not with the averaging
 * loader.  choice (int[8] or null) receives ConvKernel, phase schedule, tile pixels, tile channels, simple loader, two-source loader, then
 * the generic kernel's 16-byte chunks per LDS row and LDS stages (cprw, ns of ConvChoice, csrc/conv_select.h).  Everything is validated,
 * and the selector asked, before the first HIP call.
 * cc_dev_conv_det_choice: the same checks on the same arguments without weights, no launch and no HIP call: choice = what
 * cc_dev_conv_det would run (the pointers are only checked for null and alignment).
 * cc_dev_affine: affine_kernel (AdaFace's BatchNorm in front of a padded conv): y = x * scale[c] + shift[c] over n elements of C-channel
 * pixels in the storage type (x may be y); scale / shift device float32[C]; C whole 16-byte chunks.
 * cc_dev_face_pre: face_pre_kernel: (B,112,112,3) uint8 or float32 frames -> (B,112,112,cpad) storage type, channels reversed,
 * ((v / 255) - 0.5) / 0.5, channels 3 .. cpad zero. */
typedef struct { const void* ptr; int H, W, cstride, coff, C, shift; } cc_src_desc;
#define CC_DEV_CONV_ADOWN 100
int cc_dev_pool(int dtype, const void* in_dev, int in_cstride, int in_coff, void* out_dev, int out_cstride, int out_coff, int B, int H, int W,
                int C, int Ho, int Wo, int k, int stride, int pad, int mode, int* kernel, void* stream);
int cc_dev_pool_choice(int dtype, const void* in_dev, int in_cstride, int in_coff, void* out_dev, int out_cstride, int out_coff, int B, int H,
                       int W, int C, int Ho, int Wo, int k, int stride, int pad, int mode, int* kernel);
int cc_dev_fuse(int dtype, int n, const void* const* in_dev, const int* H, const int* W, const int* cstride, const int* coff, const int* shift,
                void* out_dev, int out_cstride, int out_coff, int B, int Ho, int Wo, int C, void* stream);
int cc_dev_conv_src(const cc_conv_desc* d, const cc_src_desc* s0, const cc_src_desc* s1, const float* w_oihw, const float* bias, void* out_dev,
                    int* choice, void* stream);
int cc_dev_conv_det(const cc_conv_desc* d, const cc_src_desc* s0, const cc_src_desc* s1, const float* w_oihw, const float* bias,
                    const void* res_dev, void* out_dev, int* choice, void* stream);
int cc_dev_conv_det_choice(const cc_conv_desc* d, const cc_src_desc* s0, const cc_src_desc* s1, const void* res_dev, void* out_dev, int* choice);
int cc_dev_affine(int dtype, const void* x_dev, void* y_dev, const float* scale_dev, const float* shift_dev, long long n, int C, void* stream);
int cc_dev_face_pre(int dtype, const void* img_dev, int img_f32, void* out_dev, int B, int cpad, void* stream);
/* Single-launch entries of the fused multi-conv kernels (csrc/dev_fused.hip): ONE launch of a kernel that keeps its intermediates on
 * chip, through its production launcher, on device buffers the caller crafts.  Every argument is validated before the first HIP call
 * (an error with its text behind cc_last_error, and no launch, on whatever the launcher itself would refuse); weights are host float32
 * OIHW arrays packed as the detector packs them; `stream` is synchronised and everything packed is freed.
 *
 * cc_dev_csp: one RepNCSP block with one bottleneck (csrc/csp_fused.hip, csp_tile.hip) over channels [x_coff, x_coff + 2 hid) of a
 * (B,H,W,x_cstride) buffer into channels [out_coff, out_coff + 2 hid) of a (B,H,W,out_cstride) one.  dtype 1 / 2 = f16 / bf16 storage;
 * split 0 = one weight plane, 1 = two f16 planes in all convs, 2 = in the 1x1 convs only (f16 storage); hid 32 or 64.  w / bias: five
 * host pointers each - cv1 (hid,2hid,1,1), cv2 (hid,2hid,1,1), m.0.cv1 folded to one 3x3 (hid,hid,3,3), m.0.cv2 (hid,hid,3,3),
 * cv3 (2hid,2hid,1,1).  variant 0 = the launcher's own rule (CLEARCAM_CSP_TILE / cc_dev_set("csp_tile")), 1 = csp_fused_kernel as the
 * launcher picks it by width, 2 = csp_fused_kernel with streamed weights, 3 = csp_tile_kernel (hid 32, split 0 / 2, no dbg), 4 = the
 * four conv launches the kernel replaces, on the same packed weights.  dbg 1 .. 3: stop after that stage and leave [a | b], t (hid
 * channels) or [u | b] in the output view (inner pixels of every tile; not with variant 3).  *choice (may be null) receives what ran:
 * 0 csp_fused_kernel with resident weights, 1 csp_fused_kernel with streamed weights, 2 csp_tile_kernel, CC_DEV_CSP_LAYERS the four launches.
 * cc_dev_csp_choice: the same checks on the same arguments without the buffers, no launch and no HIP call: *choice = what cc_dev_csp would run.
 * cc_dev_stem: letterbox + first conv (3x3 stride 2, 3 -> Cout, bias, SiLU; csrc/detect.hip stem_fused_kernel) from B frames (BGR uint8,
 * or float32 with frame_f32) at byte offsets[b] of frames_dev with heights[b] x widths[b], for a detector of resolution `res`, into
 * channels [out_coff, out_coff + Cout) of a (B,Hn/2,Wn/2,out_cstride) buffer.  ragged 0 = the uniform launch (frames of one size, one
 * behind the other), 1 = the launch over per-frame records; either way the frames must letterbox to ONE network shape Hn x Wn that is a
 * multiple of 32 (else refused, as the plans refuse it).  dtype 1 / 2; split 1 = two f16 weight planes (f16 storage); w (Cout,3,3,3) and
 * bias host arrays, Cout 16 / 32 / 64.  info (int[3] or null) receives Hn, Wn and whether the launch took the 36 KB scratch. */
#define CC_DEV_CSP_LAYERS 3
int cc_dev_csp(int dtype, int split, int hid, const void* x_dev, int x_cstride, int x_coff, void* out_dev, int out_cstride, int out_coff,
               int B, int H, int W, const float* const* w, const float* const* bias, int variant, int dbg, int* choice, void* stream);
int cc_dev_csp_choice(int dtype, int split, int hid, int B, int H, int W, int variant, int dbg, int* choice);
int cc_dev_stem(int dtype, int split, const void* frames_dev, int frame_f32, const int64_t* offsets, const int32_t* heights, const int32_t* widths,
                int B, int res, int ragged, const float* w_oihw, const float* bias, int Cout, void* out_dev, int out_cstride, int out_coff,
                int* info, void* stream);
/* Route log (cc_dev_set key "route_log"): moves up to `cap` records of 23 ints each into `records` and sets *n to the number of records
 * the log held; records that did not fit (*n > cap) stay in the log for the next call.  A record: kernel, schedule, tile pixels, tile channels, k, stride, Ho / Wo beyond the symmetric formula,
 * act, residual (0 none / 1 storage type / 2 float32), out_f32, Cout / out_coff / out_cstride all multiples of 8, then B, H, W, Cin,
 * Cout, Ho, Wo of the layer, then what picks the K loop: two weight planes, simple loader, two-source loader, 16-byte chunks per LDS row and
 * LDS stages of the generic kernel. */
int cc_route_log_take(int* records, int cap, int* n);
/* Diagnostic (kernel tuning, tools/dev/stream_ab.py, variant_sweep.py): average device milliseconds of one launch of the conv above on random
 * 16-bit data resident in HBM, weights packed once, `iters` launches between two events.  Not part of the drop-in surface. */
int cc_conv_bench(int dtype, int B, int H, int W, int Cin, int Cout, int k, int stride, int act, int variant, int iters, float* ms);
/* Diagnostic (kernel tuning): average device milliseconds of one attention launch (B images, L tokens, H heads of 64)
 * on random 16-bit data; abl: 0 the kernel, 1 K / V staging only, 2 tiles without staging.  Not part of the drop-in surface. */
int cc_attn_bench(int dtype, int B, int L, int H, int causal, int abl, int iters, float* ms);
/* Host-only helper (no GPU needed; tests / tooling): the CONTROLLED rounding cc_yolo_finalize applies to a conv's OIHW float32 weights
 * (cout, cin, k, k) for the plain 16-bit storage types (dtype 1 / 2): every weight goes to one of its two neighbours in the storage
 * type, chosen so that each output channel's total, the tap-sums of each input channel's filter, the channel-sums at each tap and the
 * first moments over the taps stay within about an ulp of their float32 values.  out[i] = the value the storage type holds, as float32. */
int cc_round_weights(int dtype, const float* w, int64_t cout, int64_t cin, int64_t k, float* out);
/* Diagnostic (kernel tuning): set a process-wide tuning switch at run time so that one process can A/B kernel variants.
 * key "phase_flags": the CLEARCAM_PHASE_FLAGS bit set of the eight-wave kernel (-1 = back to the environment / default);
 * key "stream": the weights-resident streaming 1x1 kernel off (0) / on (1) / as CLEARCAM_STREAM says (-1);
 * key "tile64_w": tile geometry of the 3x3 64 -> 64 tile kernel, 32 (8 x 32 pixels) / 16 (16 x 16) / -1 (its own rule);
 * key "stream_flags": the CLEARCAM_STREAM_FLAGS bit set of the streaming 1x1 kernel (-1 = back to the environment / default);
 * keys "stream_abl", "tile64_abl": timing ablations of development builds (no effect otherwise);
 * key "index_slab_rows": rows per bounced slab of cc_index_remove_* (-1 = the measured default), so that a test can force many
 *     slabs on a small index; rounded up to a multiple of 64.
 * key "index_i8_pass": queries per scan pass over the rows of a CC_INDEX_I8 index, 1 .. 8 (-1 = the measured default, 8), read at every
 *     search, so that the measuring tool can sweep it; scores do not depend on it.
 * key "index_i8_mfma": the smallest batch of queries a CC_INDEX_I8 index scores with its MFMA kernel instead of scan passes, read at every
 *     search: -1 = the measured default (18), 0 = never, T >= 1 = every batch of at least T queries (rows wider than 4096 elements stay
 *     with the scan whatever the key says).  cc_index_last_path tells which kernel ran.
 * key "pool_rows": output rows per thread of the avg 2x2 / avg-max pool kernels, as CLEARCAM_POOL_ROWS (8 / 4 / 1; -1 = back to the
 *     environment / default), read at every pool launch, so that one process can reach every row variant.
 * key "csp_tile": which kernel a fused RepNCSP launch at hidden width 32 takes, as CLEARCAM_CSP_TILE (0 = csp_fused_kernel, 1 = csp_tile_kernel
 *     from 256 of its tiles on, 2 = csp_tile_kernel at every size; -1 = back to the environment / default), read at every launch.
 * key "route_log": 1 = every conv / GEMM launch appends one record to a process-wide list (cc_route_log_take), 0 = off (default).
 * Plans already built keep the launches they were built with.  Not part of the drop-in surface. */
int cc_dev_set(const char* key, int value);

/* ---------------------------------------------------------------------------------------------
 * CLIP — stands behind `OpenCLIP.precompute_embedding(x)` (models/objects.py:94-133) and
 * `encode_text(model, tokens)` (models/objects.py:145-186); tokenisation stays on the host
 * (utils/clip_tokenizer.py).
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_clip cc_clip;
typedef struct {
  int image_size, patch, v_width, v_layers, v_heads, v_mlp;
  int t_ctx, t_vocab, t_width, t_layers, t_heads, t_mlp, embed;
} cc_clip_config;   /* ViT-L/14: {224,14,1024,24,16,4096, 77,49408,768,12,12,3072, 768} */

int cc_clip_create(cc_clip** h, const cc_clip_config* cfg, int dtype, int device);
int cc_clip_load(cc_clip* h, const char* name, const float* data, const int64_t* shape, int ndim);
int cc_clip_finalize(cc_clip* h);
/* precompute_embedding: x (B,3,S,S) float32 normalised pixels -> out (B,embed) float32 unit-norm. */
int cc_clip_encode_image(cc_clip* h, const float* x, int B, int x_on_device, float* out, int out_on_device, void* stream);
/* encode_text: tokens (B,t_ctx) int32 (SOT ... EOT, zero padded) -> out (B,embed) float32 unit-norm.
 * The reference only ever passes B=1 and picks row argmax(tokens) (= EOT) of batch 0. */
int cc_clip_encode_text(cc_clip* h, const int32_t* tokens, int B, float* out, int out_on_device, void* stream);
/* Batches in flight for the image tower: the contract of cc_yolo_set_in_flight / cc_yolo_submit / cc_yolo_wait above.  Pays for
 * small batches (the reference encodes one crop per call, models/objects.py:356-363); a 255-image batch fills the GPU by itself. */
int cc_clip_set_in_flight(cc_clip* h, int n);
int cc_clip_submit_image(cc_clip* h, const float* x, int B, int x_on_device, float* out, int out_on_device, void* stream,
                         long long* ticket);
int cc_clip_wait(cc_clip* h, long long ticket, void* stream);
int cc_clip_last_gpu_ms(cc_clip* h, float* ms);
void cc_clip_destroy(cc_clip* h);

/* `ObjectFinder.preprocess(img)` (models/objects.py:237-242) for a batch of crops: cv2.resize(img,(S,S),INTER_CUBIC)
 * (OpenCV 4.10 8-bit fixed-point cubic, requirements.txt:3) -> float32/255 -> (x-0.5)/0.5 -> HWC->CHW.
 * pixels: packed uint8 HWC crops (3 channels, channel order untouched), crop b = heights[b] x widths[b] starting at
 * byte offsets[b]; the three tables are host arrays.  out_dev: device float32 (B,3,S,S), ready for
 * cc_clip_encode_image(x_on_device=1).  Synchronises `stream` before returning. */
int cc_crop_preprocess(const uint8_t* pixels, const int64_t* offsets, const int32_t* heights, const int32_t* widths,
                       int B, int pixels_on_device, int out_size, float* out_dev, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * AdaFace IR-50 face embedder — stands behind `ADAFACE.__call__(x)` (models/adaface.py:79-95), called as
 * `object_finder.adaface(Tensor(face_img))` (clearcam.py:674,1236) on a 112x112x3 aligned face.
 * Parameters by the reference's state-dict names (conv0.weight, bn0.*, prelu_weight, body.list.<i>.*, bn.*,
 * linear.*, bn2.running_*).  faces: (B,112,112,3) uint8 or float32 in the order the reference receives them
 * (it flips [:,:,::-1] itself) -> out (B,512) float32, each row x / ||x||_2.
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_face cc_face;
int cc_face_create(cc_face** h, int dtype, int device);
int cc_face_load(cc_face* h, const char* name, const float* data, const int64_t* shape, int ndim);
int cc_face_finalize(cc_face* h);
int cc_face_embed(cc_face* h, const void* faces, int B, int img_f32, int faces_on_device, float* out, int out_on_device, void* stream);
void cc_face_destroy(cc_face* h);

/* The two OpenCV calls of `ObjectFinder.img_to_face` (models/objects.py:247,318,332) for uint8 HWC 3-channel host images:
 * cv2.resize(src, (dw,dh)) with the default INTER_LINEAR, and cv2.warpAffine(src, M, (dw,dh)) with the defaults
 * INTER_LINEAR / BORDER_CONSTANT 0 (M = the forward 2x3 matrix, row-major doubles, exactly what cv2 is given). */
int cc_cv_resize_linear_u8(const uint8_t* src, int H, int W, uint8_t* dst, int dh, int dw, int device);
int cc_cv_warp_affine_u8(const uint8_t* src, int H, int W, const double* M, uint8_t* dst, int dh, int dw, int device);

/* ---------------------------------------------------------------------------------------------
 * BlazeFace face detector — stands behind `BlazeFace.__call__(img)` (models/blazeface.py:165-192), called by
 * `ObjectFinder.img_to_face` (models/objects.py:253-255).  Parameters by the reference's state-dict names
 * (conv_tiny.*, backbone_tiny.list.<i>.conv{0,1}_tiny.*, final.*, classifier_{8,16}_tiny.*, regressor_{8,16}_tiny.*, anchors).
 * img: (H,W,3) uint8 or float32, channel order untouched -> out (896,17) float32 rows
 * [ymin,xmin,ymax,xmax, 6 x (kx,ky), score] in source pixels, score-descending, suppressed rows zeroed before the back-map.
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_blaze cc_blaze;
int cc_blaze_create(cc_blaze** h, int dtype, int device);
int cc_blaze_load(cc_blaze* h, const char* name, const float* data, const int64_t* shape, int ndim);
int cc_blaze_finalize(cc_blaze* h);
int cc_blaze_detect(cc_blaze* h, const void* img, int H, int W, int img_f32, int img_on_device, float* out, int out_on_device, void* stream);
void cc_blaze_destroy(cc_blaze* h);
/* B images of one size: imgs (B,H,W,3) -> out (B,896,17), row block b = what cc_blaze_detect returns for image b.  One plan (buffers +
 * captured graph) per (H, W, dtype of the images, B); cc_blaze_detect is its B = 1 case. */
int cc_blaze_detect_batch(cc_blaze* h, const void* imgs, int B, int H, int W, int img_f32, int imgs_on_device, float* out, int out_on_device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched face path — `ObjectFinder.img_to_face` (models/objects.py:243-354) for B crops in two device passes.  The crops are packed as
 * for cc_crop_preprocess (crop b = heights[b] x widths[b] x 3 uint8 at byte offsets[b] of `pixels`, `pixels_bytes` long; host tables).
 *
 * cc_face_locate: every crop letterboxed to 640 x 640 (bit-equal to cc_cv_resize_linear_u8 + a zero border), BlazeFace over the batch,
 * and per crop the FIRST row whose ymin is not 0 - the caller's own filter in img_to_face - to first[b] (17 floats, zeros when there is
 * none) and its row number, or -1, to first_idx[b].  Both are HOST arrays, complete on return.  -22 with a message naming the crop when
 * a letterboxed side would be 0.
 *
 * cc_face_align: n faces cut, levelled and placed in one launch -> out_dev (n,112,112,3) uint8 on `device`, channels reversed like
 * img_to_face's result.  Record i: the crop (offset, h, w), the cut rectangle inside it, the two FORWARD matrices exactly as
 * cv2.warpAffine is given them (rot: cut -> levelled image of out_w x out_h, place: levelled -> 112 x 112).  Bit-equal to two
 * cc_cv_warp_affine_u8 calls with the uint8 image between them, which is never written.  Synchronises `stream` before returning. */
typedef struct cc_face_align_rec {
  int64_t offset; int32_t h, w;
  int32_t cx1, cy1, cw, ch;
  int32_t out_w, out_h;
  double rot[6], place[6];
} cc_face_align_rec;
int cc_face_locate(cc_blaze* h, const uint8_t* pixels, int64_t pixels_bytes, const int64_t* offsets, const int32_t* heights, const int32_t* widths,
                   int B, int pixels_on_device, float* first, int32_t* first_idx, void* stream);
int cc_face_align(const uint8_t* pixels, int64_t pixels_bytes, int pixels_on_device, const cc_face_align_rec* records, int n,
                  uint8_t* out_dev, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * OC-SORT tracker (host code, no GPU) — stands behind `OCSort(...)` / `OCSort.update(preds, thresh)`
 * (ocsort_tracker/ocsort.py:164-308), the consumer of the detector output (clearcam.py:239,585).
 * dets: n rows [x1,y1,x2,y2,score,class] float32 exactly as cc_yolo_detect writes them (zero rows allowed).
 * out: up to cap rows of 9 doubles [tlx,tly,w,h,track_id,tracklet_len,class_id,score,speed] = the STrack fields
 * (ocsort_tracker/STrack.py:5-17), newest track first; *n_out = rows produced.  One handle per camera.
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_ocsort cc_ocsort;
int cc_ocsort_create(cc_ocsort** h, int max_age, int min_hits, double iou_threshold, int delta_t, double inertia, int use_byte);
int cc_ocsort_update(cc_ocsort* h, const float* dets, int n, double det_thresh, double* out, int cap, int* n_out);
/* One frame for each of `count` cameras: camera c reads rows_per rows at dets + c*rows_per*6 (e.g. the (B,300,6) detector
 * output as is) and writes n_out[c] <= cap_per rows at out + c*cap_per*9; cameras run on up to n_threads host threads. */
int cc_ocsort_update_many(cc_ocsort* const* hs, int count, const float* dets, int rows_per, double det_thresh, double* out,
                          int cap_per, int* n_out, int n_threads);
int cc_ocsort_num_tracks(cc_ocsort* h, int* n);
void cc_ocsort_destroy(cc_ocsort* h);

/* ---------------------------------------------------------------------------------------------
 * Embedding index — stands behind the scoring loop of `ObjectFinder.search`
 * (models/objects.py:365-376: sim = img_emb @ text_emb.T per item) over a device-resident matrix.
 * Path filtering stays in the Python shim (one byte per directory group); best-per-track-id and the sort run on the
 * device in cc_index_search_tracks.
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_index cc_index;
int cc_index_create(cc_index** h, int dim, int64_t capacity, int device);        /* f32 rows */
/* storage 0: f32 rows, exact f32 dot products.  storage 2: rows rounded to bf16 (half the bytes per scan; scores within
 * ~1e-3 of the f32 index for unit vectors; dim % 256 == 0 and dim <= 40960, or the call fails: one query of a scan pass has to fit
 * into the LDS of a CU).  `capacity` is the initial allocation: the matrix grows
 * geometrically (device-to-device copy) when cc_index_add* runs past it.
 * storage CC_INDEX_I8 (8, clear of the CC_DTYPE_* numbers): int8 rows, dim % 256 == 0 (and dim <= 16384).  A stored row is dim int8
 * codes (two's complement, element order) followed by dim / 32 float32 scales, one per group of 32 consecutive elements:
 * dim + dim / 8 bytes, 864 for dim 768.  The rule, per group with elements x_i, all in float32:
 *   a = max |x_i|;  s = a / 127.0f (correctly rounded division);  if s is zero or subnormal: s = 0 and every code 0;
 *   otherwise code_i = clamp(rintf(x_i / s), -127, 127) (round half to even).  The decoded element is (float)code_i * s.
 * A score is sum over groups of s_g * (sum_i code_i * q_i), accumulated in f32 in a fixed order: deterministic, ties break by row id,
 * and the same however a query batch is split into passes.  |score - exact| <= sum_g (s_g / 2) * ||q_g||_1 plus f32 summation error
 * (about 1e-3 at most, 2e-4 rms for unit 768-d rows).  Queries stay f32.  A batch of fewer than 18 queries goes through repeated
 * scan passes and is bit-identical to single queries.  From 18 queries on (dim <= 4096) ONE launch scores the whole batch on the matrix
 * cores: the codes as bf16 (exact), each query as three bf16 planes whose sum is the f32 query bit for bit, one MFMA K step per scale
 * group, then the same f32 fma by s_g.  That is the same sum of the same exact products in another order: last-bit differences from
 * the scan, as between the f32 index's GEMM and its scan, and the bound above is unchanged.  On either path the score of a (query,
 * row) pair depends on that pair alone - not on the batch, the query's place in it or the row's place in the index - so equal stored
 * rows tie exactly and ties break by row id.  Measured on 1 M x 768 rows, search of 64 queries: 0.82 ms, beside 0.70 ms on bf16 rows and
 * 3.1 ms with scan passes only (docs/measurement.md, "int8 rows").  Rows must be finite: a NaN or infinite element leaves the codes and the scale of ITS group of 32 undefined (the
 * row then scores NaN or nonsense); other groups and other rows are not affected, and nothing checks for it. */
#define CC_INDEX_I8 8
int cc_index_create_ex(cc_index** h, int dim, int64_t capacity, int device, int storage);
int cc_index_add(cc_index* h, const float* emb, int64_t n, int on_device);       /* append n rows (n,dim) f32, group 0 */
/* the same with one group id (0 <= id < 2^24) per row on the HOST: the caller's (camera, day folder) bucket, the unit
 * `ObjectFinder.search` filters by (models/objects.py:368-371: `/cameras/<cam>/`, `/objects/<day>/` substrings) */
int cc_index_add_grouped(cc_index* h, const float* emb, int64_t n, int on_device, const int32_t* groups);
int cc_index_size(cc_index* h, int64_t* n);
int cc_index_info(cc_index* h, int64_t* capacity, int* storage, int* dim);       /* any pointer may be NULL */
int cc_index_scores(cc_index* h, const float* q, int Q, float* scores, int on_device, void* stream); /* (Q,N) */
/* Diagnostic: which kernel produced the scores of the last scoring call on this handle (scores, search*, rank): 0 = scan passes,
 * 1 = the f32 / bf16 MFMA GEMM, 2 = the int8 MFMA kernel. */
int cc_index_last_path(cc_index* h, int* path);
/* top-k per query by score (ties: lower row id first): idx (Q,k) int32, score (Q,k) f32; rows past N: -1/-inf */
int cc_index_search(cc_index* h, const float* q, int Q, int k, int32_t* idx, float* score, int on_device, void* stream);
/* top-k restricted to rows whose group is allowed: `allowed` = n_groups bytes on the HOST (non-zero keeps the group),
 * NULL = no filter; fewer than k allowed rows -> -1/-inf padding */
int cc_index_search_groups(cc_index* h, const float* q, int Q, int k, const uint8_t* allowed, int n_groups, int32_t* idx, float* score,
                           int on_device, void* stream);
/* cc_index_add_grouped plus one track slot per row on the HOST: a dense number in [0, 2^24) the caller assigns to each
 * distinct track id, or -1 for a crop without one.  NULL = all -1, which is also what the other add calls store. */
int cc_index_add_tracked(cc_index* h, const float* emb, int64_t n, int on_device, const int32_t* groups, const int32_t* tracks);
/* The tail of `ObjectFinder.search` (models/objects.py:378-390) on the device: among the allowed rows every track slot
 * is reduced to its best row (equal scores: the lower row), rows of slot -1 stand for themselves, and the top k of
 * those answers come back by descending score.  Equal scores: tracks in the order of their first allowed row, then the
 * slot-less rows by row id (a dict in insertion order + a stable sort).  idx is the row of the track's best crop.
 * Arguments, k in [1, 1024] and the -1/-inf padding as in cc_index_search_groups; the index must hold < 2^31 rows. */
int cc_index_search_tracks(cc_index* h, const float* q, int Q, int k, const uint8_t* allowed, int n_groups, int32_t* idx, float* score,
                           int on_device, void* stream);
/* Any window of the WHOLE descending order: answers start .. start + count - 1 (0-based) of every query, at any depth and of any
 * length, in one call.  With CC_RANK_TRACKS the answers are those of cc_index_search_tracks (one per track slot plus the
 * slot-less rows, the same order); without it every allowed row is its own answer, ordered as cc_index_search_groups orders
 * them.  Only answers with score >= min_score (compared in f32; -INFINITY: no cut) exist: ranks are taken among them, and
 * total (Q int64 on the HOST, may be NULL; asking for it waits for the stream) receives their number per query.
 * idx / score are (Q, count), -1 / -inf past the last answer; allowed, on_device and stream as in cc_index_search_tracks.
 * For start 0 and count <= 1024 without a cut the result equals cc_index_search_tracks / cc_index_search_groups element for
 * element.  Errors (-22, nothing changed): NaN min_score, start < 0, count < 1, Q < 1, unknown flag bits, a bad n_groups,
 * an index of 2^31 rows or more. */
#define CC_RANK_TRACKS 1   /* reduce per track slot exactly as cc_index_search_tracks; 0: every allowed row is its own answer */
int cc_index_rank(cc_index* h, const float* q, int Q, int64_t start, int64_t count, float min_score, int flags,
                  const uint8_t* allowed, int n_groups,
                  int32_t* idx, float* score, int64_t* total, int on_device, void* stream);
/* Two attributes per row beside its group and its track slot, both read from the crop's name '<ts>_<track>_<class>.jpg':
 *   ts  - int32, the seconds into that day's recording (CC_ROW_NO_TS: the row has none);
 *   cls - int32 in [-1, 255], the detector's class (-1: the row has none).
 * cc_index_add_described is cc_index_add_tracked plus the two tables, all four on the HOST and each may be NULL (group 0, slot -1,
 * no ts, no class); the other add calls store "none" for both.  A cls outside [-1, 255] is an error (-22, nothing added).  The
 * attributes follow their rows through growth and through cc_index_remove_* (the same stable compaction, the same new numbers).
 * cc_index_row_info reads them back: rows row0 .. row0 + n - 1 into ts_out / cls_out (n int32 each on the HOST, either may be
 * NULL); a range outside the index is an error (-22). */
#define CC_ROW_NO_TS INT32_MIN
int cc_index_add_described(cc_index* h, const float* emb, int64_t n, int on_device, const int32_t* groups, const int32_t* tracks,
                           const int32_t* ts, const int32_t* cls);
int cc_index_row_info(cc_index* h, int64_t row0, int64_t n, int32_t* ts_out, int32_t* cls_out);
/* A row filter for ranking.  A row competes when its group is allowed AND (use_ts == 0 OR it has a ts with ts_min <= ts <= ts_max)
 * AND (use_cls == 0 OR it has a class c with bit c of cls_mask set: cls_mask[c / 64] >> (c % 64) & 1).  A row without the attribute
 * never passes a filter on that attribute.  The struct travels as kernel arguments: no allocation, no copy. */
typedef struct { int32_t use_ts, ts_min, ts_max;   /* inclusive at both ends */
                 int32_t use_cls; uint64_t cls_mask[4]; /* bit c set: class c passes */ } cc_row_filter;
/* cc_index_rank among the competing rows only.  Everything else is cc_index_rank's contract: with CC_RANK_TRACKS a track is reduced
 * among its PASSING rows and its place among equal scores is its first PASSING row, so the call answers as an index built from the
 * passing rows alone would (same slots, same groups): scores bit for bit, rows under their numbers in THIS index, total equal.
 * where == NULL: exactly cc_index_rank.  Errors (-22, nothing changed): those of cc_index_rank, ts_min > ts_max with use_ts, an
 * all-zero mask with use_cls. */
int cc_index_rank_where(cc_index* h, const float* q, int Q, int64_t start, int64_t count, float min_score, int flags,
                        const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                        int32_t* idx, float* score, int64_t* total, int on_device, void* stream);
/* How the answers of a query spread over time: a histogram of the answers cc_index_rank_where would rank (same cut, flags, filters).
 * An answer's time is the ts of the row `idx` would name for it (a track: its best passing crop, not its first row).  It is counted
 * in bin floor((ts - t0) / bin_seconds), computed in 64 bits; an answer without ts, or with a bin outside [0, n_bins), is counted in
 * total only, so sum(counts[q]) <= total[q], and total[q] equals cc_index_rank_where's.  counts: (Q, n_bins) uint32, on the device
 * with on_device (queries then too); total: Q int64 on the HOST, may be NULL.  The call waits for the stream unless on_device is
 * set and total is NULL.  bin_seconds >= 1, 1 <= n_bins <= 4096, otherwise -22 like the errors of cc_index_rank_where.
 * Integer sums: the result does not depend on the order in which blocks arrive. */
int cc_index_timeline(cc_index* h, const float* q, int Q, float min_score, int flags, const uint8_t* allowed, int n_groups,
                      const cc_row_filter* where, int32_t t0, int32_t bin_seconds, int n_bins,
                      uint32_t* counts, int64_t* total, int on_device, void* stream);
/* What the index holds for some rows, decoded to f32: rows = n numbers on the HOST, any order, repeats allowed, 1 <= n <= 65535
 * -> out (n, dim) f32 on the host or the device (on_device).  f32 rows: the bytes as they are; bf16 rows: the 16 bits in the high
 * half of the word; CC_INDEX_I8 rows: the decoded element of the rule above, (float)code_i * s_g (one f32 multiply).  One gather
 * launch on `stream` (NULL: the handle's own); a host `out` waits for it.  Up to CC_LIKE_MAX_ROWS numbers travel in the kernel
 * arguments, a longer list through pinned memory.  A number outside [0, size), or n outside the range: -22, out untouched. */
int cc_index_fetch_rows(cc_index* h, const int64_t* rows, int n, float* out, int on_device, void* stream);
/* "More like these stored rows": the queries are rows of the index itself, gathered on the device (no embedding crosses the bus
 * in either direction), and a row's score is its best score against any of them.  ONE answer list comes back: idx / score of
 * `count` entries and one total.
 *   1. Q = cc_index_fetch_rows(rows), n_rows queries in the order given.
 *   2. S (n_rows, N) is bit for bit what cc_index_scores(h, Q, n_rows) returns, by the same route for that batch size and index size
 *      (scan passes, the f32 / bf16 GEMM, the int8 MFMA kernel); cc_index_last_path reports it.
 *   3. v[r] = max over q of S[q][r], the maximum in the total order of the ranking keys (+0 beats -0; NaN is not supported).
 *   4. A row is out of the running when it is dead (the exclude flags below), when `allowed` forbids its group or when `where`
 *      rejects it.
 *   5. The result is that of cc_index_rank_where for a single query whose score vector is v, among the rows left: the same keys and
 *      tie rules (a track's place is its first competing row, slot-less rows behind tracks of equal score), the same min_score
 *      cut, total, -1 / -inf padding, on_device and stream semantics.  It answers as an index built from the competing rows would.
 *   6. flags: CC_RANK_TRACKS and the two exclude bits.  CC_LIKE_EXCLUDE_ROWS: the query rows are dead.  CC_LIKE_EXCLUDE_TRACK: every
 *      row that shares BOTH the group and the track slot of the query rows is dead, and so are the query rows (TRACK implies ROWS).
 *      A byte-equal copy of a dead row elsewhere still competes, with the dead row's score.
 *   7. Errors (-22, nothing changed): those of cc_index_rank_where; n_rows outside [1, CC_LIKE_MAX_ROWS]; a row number outside
 *      [0, size); unknown flag bits; CC_LIKE_EXCLUDE_TRACK when the query rows do not all share one group and one slot >= 0.
 *   8. The row numbers, and for CC_LIKE_EXCLUDE_TRACK the group and the slot of the query rows, are checked on the host before any
 *      launch (the handle keeps a host copy of the two columns, 8 bytes a row): an error costs no device work and no wait.
 * With one query row and no exclude bit the launches are those of cc_index_rank_where for one device query behind a gather of one
 * row; otherwise one more pass folds S into v in place and writes the dead bytes. */
#define CC_LIKE_MAX_ROWS 64
#define CC_LIKE_EXCLUDE_ROWS  2   /* the query rows do not compete */
#define CC_LIKE_EXCLUDE_TRACK 4   /* no row that shares BOTH group and track slot with the query rows competes */
int cc_index_rank_like(cc_index* h, const int64_t* rows, int n_rows, int64_t start, int64_t count, float min_score, int flags,
                       const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                       int32_t* idx, float* score, int64_t* total, int on_device, void* stream);
/* Compound search: up to CC_TERMS_MAX terms in ONE ranking.  A term is a vector the caller brings (a text or image embedding) or a
 * stored row, and it has a role: it contributes to the ranking value (RANK, through the combine rule and its weight), it must hold
 * (REQUIRE: "person AND it looks like this crop") or it must not (REJECT: "white van, but not this one").  ONE answer list comes
 * back, as from cc_index_rank_like, and optionally the term that made each answer's value.
 *   1. Terms.  T = n_vec + n_rows, 1 <= T <= CC_TERMS_MAX.  Terms 0 .. n_vec-1 are the vectors q ((n_vec, dim) f32, on the device
 *      with on_device, as cc_index_rank's queries); terms n_vec .. T-1 are the stored rows `rows` (numbers on the HOST, gathered on
 *      the device as cc_index_fetch_rows decodes them).  terms[t] describes term t; the array is read on the host at the call.
 *   2. Scores.  S (T, N) is bit for bit what cc_index_scores returns for those T vectors in that order, by the same route for that
 *      batch size and index size (scan passes, the f32 / bf16 GEMM, the int8 MFMA kernel); cc_index_last_path reports it.  No
 *      embedding crosses the bus for a stored row.
 *   3. Ranking value v[r], from the RANK terms only, in ascending term order:
 *        CC_COMBINE_MAX / CC_COMBINE_MIN: the maximum / minimum of S[t][r] in the total order of the ranking keys (+0 above -0);
 *        CC_COMBINE_SUM: v = +0.0f; then for each RANK term v = v + weight_t * S[t][r], the product and the sum each rounded to f32
 *        on its own (never fused), so plain float32 arithmetic in that order reproduces v bit for bit.
 *      weight is ignored for MAX / MIN; a negative weight ("less of this") is allowed.
 *   4. Dead rows.  A row is dead when a REQUIRE term scores it below its cut (NOT S[t][r] >= cut), when a REJECT term scores it at
 *      or above its cut (S[t][r] >= cut; IEEE f32 compares, -0 == +0), or by cc_index_rank_like's two exclude bits, which here act
 *      on the stored rows that are RANK terms: CC_LIKE_EXCLUDE_ROWS: those rows are dead; CC_LIKE_EXCLUDE_TRACK: every row that
 *      shares their common group and slot is dead (they must share one group and one slot >= 0, as in cc_index_rank_like).  A score
 *      depends on its (vector, row) pair alone, so a byte-equal copy of a REJECT row elsewhere is rejected with it, while a copy of
 *      an EXCLUDED row still competes, as in cc_index_rank_like: "not this object" against "not this stored crop".
 *   5. Result.  That of cc_index_rank_where for a single query whose score vector is v, among the rows that are not dead, allowed
 *      and passing `where`: the same keys, tie rules, min_score cut (on v), total, -1 / -inf padding, on_device and stream
 *      semantics.  A track is reduced among its surviving rows and placed by its first surviving row: the call answers as an index
 *      built from the surviving rows would.
 *   6. which may be NULL.  Otherwise `count` int32 (on the device with on_device): for each answer the term that made v at the row
 *      idx names (a track: its best surviving crop).  MAX / MIN: the lowest-numbered RANK term attaining v.  SUM: the RANK term with
 *      the largest product weight_t * S[t][r] in key order, the lowest-numbered on ties.  -1 where idx is -1.
 *   7. cc_index_timeline_terms is cc_index_timeline (one query) on the same v and the same dead rows; its total equals
 *      cc_index_rank_terms'.
 *   8. Errors (-22, nothing changed, checked on the host before any launch): those of cc_index_rank_where / cc_index_timeline; T out
 *      of range, a negative n_vec / n_rows, a null q / rows with a positive count, a null terms; no RANK term; an unknown role or
 *      combine; a non-finite weight on a RANK term under SUM; a NaN cut on a REQUIRE / REJECT term; a row number outside [0, size);
 *      an exclude bit without a stored-row RANK term; unknown flag bits.  NaN scores are not supported, as everywhere.
 * Launches: the vectors are copied and the rows gathered where queries stand, ONE scoring call scores all T, one pass
 * (terms_fold_kernel) folds S into v in place over its row 0 and writes one dead byte a row (only when a term or a flag can kill a
 * row) and one `which` byte a row (only when asked for), then the launches of cc_index_rank_where / cc_index_timeline for one query
 * follow unchanged, plus a gather of `count` entries for `which`.  One RANK vector, MAX or MIN, nothing else: no fold at all. */
#define CC_TERMS_MAX 64
#define CC_TERM_RANK    0   /* contributes to the ranking value v through the combine rule */
#define CC_TERM_REQUIRE 1   /* a row competes only if S[t][r] >= cut  (IEEE f32 compare) */
#define CC_TERM_REJECT  2   /* a row is dead if S[t][r] >= cut */
#define CC_COMBINE_MAX 0
#define CC_COMBINE_MIN 1
#define CC_COMBINE_SUM 2
typedef struct { int32_t role; float weight; float cut; } cc_term;
int cc_index_rank_terms(cc_index* h, const float* q, int n_vec, const int64_t* rows, int n_rows,
                        const cc_term* terms, int combine,
                        int64_t start, int64_t count, float min_score, int flags,
                        const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                        int32_t* idx, float* score, int32_t* which, int64_t* total, int on_device, void* stream);
int cc_index_timeline_terms(cc_index* h, const float* q, int n_vec, const int64_t* rows, int n_rows,
                            const cc_term* terms, int combine, float min_score, int flags,
                            const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                            int32_t t0, int32_t bin_seconds, int n_bins,
                            uint32_t* counts, int64_t* total, int on_device, void* stream);
/* Together: rank the rows of one question that have a partner - an answer of a second question - nearby in time in the same folder
 * ("a person while a white van is at the gate", "someone near my car").  Two objects at once, one ranking; the join runs on the device
 * over the ts, group and track columns.
 *   1. Sides.  A is what is ranked, B is what must be nearby.  Each side is either a vector (qa / qb: dim f32, on the device with
 *      on_device) or a stored row (row_a / row_b with a NULL vector; gathered on the device as cc_index_fetch_rows decodes it; -1 beside a
 *      vector).  A side needs exactly one of the two.
 *   2. Scores.  Sa, Sb (N each) are bit for bit what cc_index_scores returns for the batch of the two vectors (A first).  Two queries go
 *      by the scan route in every storage, so these are also the bits of the single-query calls.
 *   3. Partner list.  The first max_partners answers of an ungrouped ranking of B: cc_index_rank_where(qb, start 0, count max_partners,
 *      min_score cut_b, flags 0, allowed, where_b), restricted to rows that have a ts: a row with CC_ROW_NO_TS is never a partner and
 *      takes no place in the list.  The order is that ranking's: score descending, equal scores by ascending row.
 *      1 <= max_partners <= CC_NEAR_MAX_PARTNERS; CC_NEAR_DEFAULT_PARTNERS is what callers pass who have no opinion.  n_partners (one
 *      int64 on the HOST, may be NULL; asking for it waits for the stream as total does) receives the number of rows that would be in the
 *      list without the cap, so a caller sees a truncated list.
 *   4. Join.  Entry p of the list qualifies for row r when p != r, grp[p] == grp[r], r has a ts, |ts[p] - ts[r]| <= within with the
 *      difference taken in 64 bits, and NOT (trk[r] >= 0 and trk[p] == trk[r]): a crop of the same track in the same folder is nobody's
 *      partner ("person near a red thing" must not answer with the person's own red jacket).  within: seconds, in [0, INT32_MAX].  The
 *      partner of r is the FIRST qualifying entry in list order, which is the best-scoring one.
 *   5. Value and dead rows.  A row without a partner is dead.  Otherwise CC_NEAR_VALUE_A: v[r] = Sa[r]; CC_NEAR_VALUE_MIN: v[r] = the
 *      smaller of Sa[r] and Sb[partner] in the total order of the ranking keys (+0 above -0), the fuzzy AND of CC_COMBINE_MIN.
 *   6. Result.  That of cc_index_rank_where for a single query whose score vector is v, among the rows that are not dead, allowed and
 *      passing where_a: the same keys, tie rules, min_score cut (on v), total, -1 / -inf padding, on_device and stream semantics.  With
 *      CC_RANK_TRACKS a track is reduced among its surviving rows and placed by its first surviving row.  partner (count int32) and
 *      partner_score (count f32; either may be NULL; on the device with on_device) name for each answer the partner of the row idx names
 *      and its Sb, -1 / -inf where idx is -1.
 *   7. cc_index_timeline_near is cc_index_timeline (one query) on the same v and the same dead rows; its total and n_partners equal
 *      cc_index_rank_near's.
 *   8. Errors (-22, nothing changed, checked on the host before any launch): those of cc_index_rank_where / cc_index_timeline (for both
 *      filters); both or neither of vector and row on a side; a row number outside [0, size); within < 0; max_partners out of range; a
 *      NaN cut_b; an unknown value; unknown flag bits (CC_RANK_TRACKS is the only one).
 * Launches: the vectors are copied and the rows gathered where queries stand, ONE scoring call scores both, the selection launches of
 * cc_index_rank_where run on B's score row and leave the list on the device, one small kernel packs it into columns, near_fold_kernel
 * (one thread per row, the list staged through LDS 1024 entries at a time, the walk stopped at the first qualifying entry) writes v in
 * place over score row 0, one dead byte and the partner's place per row, then the launches of cc_index_rank_where / cc_index_timeline
 * for one query follow unchanged, plus a gather of `count` partner entries.  Nothing is read back inside the call.  Scratch: 4 bytes a
 * row and 350 KB beside what cc_index_rank_terms uses.  The walk costs up to N x max_partners compares when nothing qualifies anywhere;
 * a row that cannot be an answer (a forbidden group, rejected by where_a, no ts, or - without CC_RANK_TRACKS - Sa below min_score) skips
 * it. */
#define CC_NEAR_MAX_PARTNERS     16384
#define CC_NEAR_DEFAULT_PARTNERS 4096
#define CC_NEAR_VALUE_A   0   /* v = Sa: rank by A alone, B only decides who competes */
#define CC_NEAR_VALUE_MIN 1   /* v = min(Sa, Sb[partner]) in key order */
int cc_index_rank_near(cc_index* h, const float* qa, int64_t row_a, const float* qb, int64_t row_b,
                       int32_t within, int max_partners, float cut_b, int value,
                       int64_t start, int64_t count, float min_score, int flags,
                       const uint8_t* allowed, int n_groups, const cc_row_filter* where_a, const cc_row_filter* where_b,
                       int32_t* idx, float* score, int32_t* partner, float* partner_score, int64_t* total, int64_t* n_partners,
                       int on_device, void* stream);
int cc_index_timeline_near(cc_index* h, const float* qa, int64_t row_a, const float* qb, int64_t row_b,
                           int32_t within, int max_partners, float cut_b, int value, float min_score, int flags,
                           const uint8_t* allowed, int n_groups, const cc_row_filter* where_a, const cc_row_filter* where_b,
                           int32_t t0, int32_t bin_seconds, int n_bins,
                           uint32_t* counts, int64_t* total, int64_t* n_partners, int on_device, void* stream);
/* Distinct answers: thin ranked lists so that the same picture, stored under many track ids, on many days or by many cameras,
 * answers once.  The embedding-space counterpart of what the detector does with boxes, behind any of the ranking calls above. */
#define CC_DISTINCT_MAX_DEPTH 1024
#define CC_DISTINCT_MAX_Q     64
/* Pairwise similarities of stored rows: rows = n numbers on the HOST, 1 <= n <= CC_DISTINCT_MAX_DEPTH, any order, repeats allowed
 * -> out (n, n) f32 on the host or the device (on_device): out[i][j] = the f32 dot product of what the index holds for rows[i] and
 * rows[j], i.e. of the rows cc_index_fetch_rows decodes, for all three storages.  Part of the contract, because cc_index_distinct is
 * defined on top of it: (a) out[i][j] depends on the two stored rows alone, not on i, j, n or the rest of the list (a byte-equal copy
 * at another row number gives the same bits); (b) out[i][j] == out[j][i] bit for bit.  The summation order is otherwise free: one
 * chain of f32 fused multiply-adds over the row (exact f32 MFMA), within the order-free float64 bound of the stored rows.  One launch
 * on `stream` (NULL: the handle's own); a host `out` waits for it.  A number outside [0, size) or n out of range: -22, out untouched,
 * checked on the host before any launch. */
int cc_index_gram(cc_index* h, const int64_t* rows, int n, float* out, int on_device, void* stream);
/* Thin Q ranked lists: an answer is kept only if it is not "the same picture" as an answer kept before it.
 *   1. idx (Q, depth) int32: Q lists in the order given (the call does not sort), typically the idx of cc_index_rank* for start 0
 *      and count = depth.  An entry < 0 or >= size is absent and skipped (each entry is tested on the device), so the -1 padding of
 *      the ranking calls passes straight through.  score (Q, depth) f32 or NULL is only passed through.  on_device: idx, score and
 *      the three outputs are device pointers, otherwise all are host pointers.
 *   2. With c_0, c_1, ... the present entries of a list in order and G = cc_index_gram of them: c_0 is kept; c_j is kept iff no KEPT
 *      c_i, i < j, has G[i][j] >= same_at (compared in f32).  The greedy rule: a dropped answer suppresses nothing (unlike the
 *      detector's mask rule).  A dropped c_j is counted to the first (lowest i) kept c_i with G[i][j] >= same_at.
 *   3. The kept entries in order are the answers.  out_idx / out_score (Q, count) receive answers start .. start+count-1 and -1 / -inf
 *      past the last; out_score is the input score of the kept entry (ignored when score is NULL).  out_dups (Q, count) int32, may
 *      be NULL: the dropped entries counted to that answer, 0 in the padding.  total: Q int64 on the HOST, may be NULL: the number
 *      of kept entries; asking for it waits for the stream, as a host caller always does.
 *   4. same_at above every similarity drops nothing: the list with its absent entries squeezed out, windowed.  -inf keeps c_0 alone.
 *   5. A repeated row number in a list is an ordinary pair, G of a row with itself.
 *   6. Errors (-22, nothing written, no launch): NaN same_at; depth outside [1, CC_DISTINCT_MAX_DEPTH]; Q outside
 *      [1, CC_DISTINCT_MAX_Q]; start < 0; count < 1 (or Q * count >= 2^40); a NULL idx or out_idx, or a score without an out_score.
 *   7. The handle's scratch grows on demand (136 KB a list); the index is not modified.  Three launches on `stream`: squeeze, the
 *      Gram tiles of each list compared with same_at into a bit matrix (the accumulation is cc_index_gram's, so a bit is the
 *      comparison of the very float cc_index_gram returns), and one sequential walk per list. */
int cc_index_distinct(cc_index* h, const int32_t* idx, const float* score, int Q, int depth, float same_at,
                      int64_t start, int64_t count,
                      int32_t* out_idx, float* out_score, int32_t* out_dups, int64_t* total,
                      int on_device, void* stream);
/* Day digest: "what was on this camera today?" - every distinct object among the competing rows once, with how often and when it was
 * seen.  No query and no scores: leader clustering in row order, which is ingest order and therefore time order within a folder.
 *   1. The rows that compete are those of cc_index_rank_where without CC_RANK_TRACKS: allowed / n_groups and where mean the same,
 *      NULL means no filter.  They are walked in ascending row number.
 *   2. A row JOINS the first-created leader l for which element [0][1] of cc_index_gram over rows (l, r) is >= same_at (compared in
 *      f32; the accumulation is cc_index_gram's, so it is that very float).  If none matches and fewer than max_leaders leaders exist
 *      it BECOMES a leader; if the cap is reached it is LEFT OVER: counted, owning nothing, neither suppressing nor attracting any
 *      row.  A member never attracts rows either (the greedy rule of cc_index_distinct: in a chain a~b, b~c, a!~c, b joins a and c
 *      leads).  The answer does not depend on how the implementation cuts the rows into pieces.
 *   3. Per leader: row (the leader itself, the object's first sighting), count (its members, itself included), ts_first / ts_last
 *      (the min / max ts over members that have one, CC_ROW_NO_TS if none has).  Leaders are sorted by `order`; entries
 *      start .. start+count-1 go to the four (count,) outputs, -1 / 0 / CC_ROW_NO_TS / CC_ROW_NO_TS past the last leader.  out_count,
 *      out_ts_first and out_ts_last may each be NULL.
 *   4. owner, may be NULL: one int32 per index row - the leader's row number for a member (a leader owns itself), -1 for a row that
 *      did not compete, -2 for a left-over row.  totals, may be NULL: 3 int64 on the HOST - leaders, competing rows, left-over rows;
 *      asking for it waits for the stream.  The counts of all leaders sum to totals[1] - totals[2].
 *   5. on_device: the five outputs are device pointers; otherwise host pointers, and the call waits.  No competing rows: success,
 *      zero totals, all padding.  same_at = +inf makes every competing row a leader up to the cap, -inf one leader that owns all.
 *   6. Errors (-22, nothing written, no launch): NaN same_at; max_leaders outside [1, CC_DIGEST_MAX_LEADERS]; an unknown order;
 *      start < 0; count < 1; a NULL out_row; the n_groups and filter errors of cc_index_rank_where; an index of 2^31 rows or more.
 *   7. The index is not modified; the handle's scratch grows on demand (8 bytes a row + 290 KB).  On `stream`: the selection (three
 *      launches and ONE readback, the number of competing rows), then per piece of up to 1024 competing rows three launches (piece x
 *      leaders tiles, piece x piece tiles, one sequential walk), then a sort of the leaders.  Nothing waits between the pieces. */
#define CC_DIGEST_MAX_LEADERS 1024
#define CC_DIGEST_BY_COUNT 0   /* count descending, equal counts: lower leader row first */
#define CC_DIGEST_BY_FIRST 1   /* leader row ascending: order of first appearance */
int cc_index_digest(cc_index* h, float same_at, int max_leaders, int order,
                    const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                    int64_t start, int64_t count,
                    int32_t* out_row, int32_t* out_count, int32_t* out_ts_first, int32_t* out_ts_last,
                    int32_t* owner, int64_t* totals, int on_device, void* stream);
/* Seen before? - "which of today's objects have we seen before, where, and which are new?": up to CC_SIGHT_MAX_OBJECTS stored rows (the
 * objects, typically the leaders of a cc_index_digest) against ALL competing rows, reduced per object.  Many to many, no ranking.
 *   1. rows: n row numbers on the HOST, 1 <= n <= CC_SIGHT_MAX_OBJECTS, in any order, repeats allowed (each position is its own
 *      object).  They are checked on the host before any launch, as cc_index_gram checks its rows.
 *   2. The rows that compete are those of cc_index_rank_where without CC_RANK_TRACKS: allowed / n_groups and where mean the same,
 *      NULL means no filter.  An object need not compete itself.
 *   3. The pair value of object i and competing row r is g = element [0][1] of cc_index_gram over rows (rows[i], r): that very float
 *      (one chain of f32 fused multiply-adds over k on the exact f32 MFMA, in cc_index_gram's accumulation order), independent of
 *      tile, side, kernel and the rest of the launch.  With CC_SIGHT_SKIP_SELF the pair with r == rows[i] does not exist for object
 *      i; a byte-equal copy at another row number still counts.
 *   4. Per object, (n,) each: out_count[i] = the number of pairs with g >= same_at (compared in f32).  out_best_row[i] /
 *      out_best_score[i] = the pair with the largest g in the total order of the ranking keys (+0 beats -0; NaN unsupported), among
 *      equal g the lowest row number; it does not depend on same_at; -1 / -inf with no pair.  out_best_row and out_best_score may
 *      each be NULL, out_count may not.
 *   5. out_group_counts (n, n_group_counts) uint32, may be NULL (then n_group_counts must be 0, else 1 <= n_group_counts <=
 *      CC_SIGHT_MAX_GROUPS): entry [i][g] = the matching pairs (g >= same_at) of object i whose row has group g.  A match in a group
 *      >= n_group_counts is counted in out_count only.
 *   6. total: one int64 on the HOST, may be NULL: the number of competing rows; asking for it waits for the stream.  on_device: the
 *      four outputs are device pointers (rows stays on the host) and the call does not wait unless total is asked for; otherwise
 *      they are host pointers and the call waits.  There is no readback inside the call: the number of competing rows stays on the
 *      device, where the kernels read it.
 *   7. Every reduction is an integer sum or a maximum of totally ordered keys: the answer does not depend on the arrival of the
 *      blocks or on how the rows are cut into strips, and two calls give equal bytes.
 *   8. No competing rows: success, zero counts, -1 / -inf.  same_at = -inf counts every pair, +inf none; best is unaffected.
 *   9. Errors (-22, nothing written, no launch): NaN same_at; n outside [1, CC_SIGHT_MAX_OBJECTS]; a row outside [0, size); unknown
 *      flag bits; a NULL rows or out_count; out_group_counts / n_group_counts inconsistent or out of range; the n_groups and filter
 *      errors of cc_index_rank_where; an index of 2^31 rows or more.
 *  10. The index is not modified; the handle's scratch grows on demand: the digest's (8 bytes a row + 290 KB, shared with
 *      cc_index_digest) + 16 KB, and for a host caller n * (12 + 4 * n_group_counts) bytes.  On `stream`: the selection (the digest's
 *      three launches), the zeroing of the outputs, ONE scoring launch (a persistent grid of 128-row strips x object tiles that keeps
 *      its per-object tables in LDS and folds them into the outputs once per block) and one launch that decodes the best keys. */
#define CC_SIGHT_MAX_OBJECTS 1024
#define CC_SIGHT_MAX_GROUPS  4096
#define CC_SIGHT_SKIP_SELF   1
int cc_index_sightings(cc_index* h, const int64_t* rows, int n, float same_at, int flags,
                       const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                       int32_t* out_count, int32_t* out_best_row, float* out_best_score,
                       uint32_t* out_group_counts, int n_group_counts,
                       int64_t* total, int on_device, void* stream);
/* Remove rows; survivors keep their order and are renumbered densely (new id = survivors before the row).
 * drop: n bytes on the HOST, non-zero removes the row; n must equal the current size (else an error, index untouched).
 * *removed (may be NULL) receives the count.  Capacity and track slots are unchanged.  Synchronous like cc_index_add*. */
int cc_index_remove_rows(cc_index* h, const uint8_t* drop, int64_t n, int64_t* removed);
/* The same for every row whose group id g has drop[g] != 0; groups >= n_groups are kept. */
int cc_index_remove_groups(cc_index* h, const uint8_t* drop, int n_groups, int64_t* removed);
void cc_index_destroy(cc_index* h);

/* ---------------------------------------------------------------------------------------------
 * Text-described alerts at ingest — the walk of clearcam.py:1289-1307 for a whole batch of crop embeddings in one call.
 * Per crop the reference goes through its camera's alerts in order, skips those that fired less than 60 s ago, are inactive or
 * have no description, and the first whose `desc_emb @ emb.T` is STRICTLY above its threshold notifies and ends the walk.  A crop
 * fires at most one alert, and a fired alert is spent for the crops behind it in the batch (a later crop can still fire the next
 * alert in order).  The table of descriptions stands on the device; which alerts are armed (cooldown, active, described) is the
 * caller's byte per alert.
 * Scores: every (crop, alert) score is the f32 dot product summed in the order of the index's scan (16 lanes a row, lane j takes
 * elements 64 t + 4 j + {0,1,2,3} for t ascending with fma from 0, then a 16-lane xor butterfly at 8, 4, 2, 1).  It depends on
 * that pair alone - not on B, A or the position in either table - and equals, bit for bit, the score an f32 cc_index holding the
 * crop gives a single query with the description.  An alert that fired with score s is therefore found by searching for its
 * description with exactly s.
 * Handles are not thread-safe.  Errors: a negative code, text behind cc_last_error().
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_watch cc_watch;
/* The most alerts one table holds: cc_watch_match settles a batch on ONE wave, in which each of the 64 lanes owns one 32-bit word
 * of the armed mask in a register (64 x 32).  A larger table is refused by cc_watch_set. */
#define CC_WATCH_MAX_ALERTS 2048
int cc_watch_create(cc_watch** h, int dim, int device);                          /* dim % 256 == 0 and dim <= 4096 */
/* Replace the whole table: desc (A,dim) f32, threshold A floats, group A camera numbers in [0, 2^24), all on the HOST.  Index in
 * the table is priority (the camera's dict order).  A == 0 clears it; A > CC_WATCH_MAX_ALERTS or a group outside the range is an
 * error and leaves the table as it was.  Synchronous: waits for the handle's own stream; calls given another stream are the caller's to order. */
int cc_watch_set(cc_watch* h, const float* desc, const float* threshold, const int32_t* group, int A);
int cc_watch_size(cc_watch* h, int* A);
/* The (B,A) scores, row-major: emb (B,dim) f32 on the host or the device (emb_on_device), scores to the host or the device
 * (on_device).  What the reference prints as `sim =`.  Nothing is written when B or A is 0. */
int cc_watch_scores(cc_watch* h, const float* emb, int B, int emb_on_device, float* scores, int on_device, void* stream);
/* The walk.  crop_group: B camera numbers on the HOST; armed: A bytes on the HOST (non-zero = armed), NULL = all armed.
 * alert[b] = the table index of the alert crop b fires, -1 where none; score[b] = that alert's score, 0 where none; both to the
 * host or the device (on_device).  Alert a can fire for crop b when it is armed, not yet fired by an earlier crop of this batch,
 * group[a] == crop_group[b] and score > threshold[a] in f32 (a NaN score never fires); the lowest such a fires.
 * Two launches on `stream` (NULL: the handle's own): scores + hit bits, then the sequential rule on one wave.  B == 0 does nothing;
 * A == 0 launches no kernel and answers -1 / 0.  Host outputs wait for the stream; device outputs wait for nothing. */
int cc_watch_match(cc_watch* h, const float* emb, int B, int emb_on_device, const int32_t* crop_group, const uint8_t* armed,
                   int32_t* alert, float* score, int on_device, void* stream);
void cc_watch_destroy(cc_watch* h);

#ifdef __cplusplus
}
#endif
#endif
