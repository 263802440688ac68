// Which kernel runs a conv / GEMM (conv_mfma.hip: choose_conv) and the process-wide switches that steer the choice.
#pragma once
#include <atomic>
#include "common.h"

namespace cc {

// ConvP::variant: 0 lets choose_conv pick; any other value forces a kernel (tests, tools/dev, the C ABI's force_direct / variant).
// A forced kernel fails with an error on a shape it cannot run; a value that names no kernel is refused.
enum ConvVariant : int {
  CONV_AUTO = 0,
  CONV_DIRECT = 1,            // direct (non-MFMA) kernel, conv_direct.hip
  CONV_GENERIC = 2,           // generic implicit GEMM, conv_mfma_kernel (deep K on 128-wide channel tiles: conv_big_kernel<T, 128>)
  CONV_WS = 4,                // weights-stationary narrow 3x3, conv3x3_ws_kernel
  CONV_BIG256 = 5,            // single-barrier schedule with 256 x 256 tiles, conv_big_kernel<T, 256>
  CONV_BIG128 = 6,            // the same with 128 x 128 tiles
  CONV_PHASE = 7,             // eight-wave two-group 256 x 256 kernel, conv_phase.hip / conv_persist.hip
  CONV_WAVE = 8,              // wave-autonomous narrow 3x3, conv_wave.hip
  CONV_SMALL = 9,             // few-tile configuration: narrow channel tiles, 3-6 LDS stages
  CONV_STREAM = 10,           // weights-resident streaming 1x1, conv_stream.hip
  CONV_TILE64 = 12,           // persistent 3x3 64 -> 64 tile kernel, conv_tile64.hip
  CONV_SMALL_32_4 = 91,       // tuning sweeps of the few-tile configuration: 32-wide channel tiles, 4 stages
  CONV_SMALL_32_6 = 92,       //   32-wide, 6 stages
  CONV_SMALL_64_3 = 93,       //   64-wide, 3 stages
  CONV_PIX64_6 = 94,          // 64-pixel tiles on 256 threads, 6 stages
  CONV_PIX64_4 = 95,          //   4 stages
  CONV_PIX32_6 = 96,          // 32-pixel tiles, 6 stages
  CONV_PIX32_4 = 97,          //   4 stages
};

enum class ConvKernel : int { Direct, Generic, Big, Phase, Ws, Wave, Tile64, Stream };

// Phase schedules: conv_phase_kernel<T, 0 | 1 | 2> (two-barrier / one tile per block / buffer-descriptor DMA) or the persistent loop
enum { PHASE_SCHED0 = 0, PHASE_ONE_TILE = 1, PHASE_BUFFER = 2, PHASE_PERSIST = 3 };

struct ConvChoice {
  ConvKernel kernel = ConvKernel::Generic;
  // Generic: conv_mfma_kernel<T, bm, bn, wm, simple, cprw, ns, nth>;  Big: conv_big_kernel<T, bm> (bn = bm);  Phase: bn = 256
  int bm = 128, bn = 128, wm = 2, cprw = 8, ns = 2, nth = 256;
  bool simple = false;        // one source, no upsample, ks <= 3 (the incremental-pointer loader)
  int sched = 0;              // Phase: PHASE_*
  bool two = false;           // Phase: 1x1 over the concat of two sources
  int flags = 0;              // Phase: ConvAux::flags;  Stream: StreamAux::flags
  int tile64_w = 32;          // Tile64: 8 x 32-pixel tiles (32) or 16 x 16 (16)
  int cin = 0, cout = 0;      // Ws / Wave / Stream: the channel counts of the instantiation
};

// Pure (no HIP calls).  Throws on a variant that names no kernel and on a forced kernel the shape is not eligible for.
ConvChoice choose_conv(int dt, const ConvP& p);

// conv_tile64.hip takes a 3x3 64 -> 64 layer of B frames of H x W (eligible shape assumed): CLEARCAM_TILE64 on, one full round of its
// 256-pixel tiles and the better of 16 x 16 / 8 x 32 tiles within 1.25x of the map.  yolo.hip's RepNCSP fusion (Builder::fuse_csp) asks the same question.
bool conv_tile64_takes(int B, int H, int W);

// launch_conv_mfma, handing back the choice it launched with (`chosen` may be null): the same choose_conv call serves both.
void launch_conv_chosen(int dt, const ConvP& p, hipStream_t stream, ConvChoice* chosen);

// Route log (development, tests): with cc_dev_set("route_log", 1) every launch through launch_conv_chosen appends one record to a
// process-wide, mutex-guarded list; cc_route_log_take reads and clears it.  Off by default: one relaxed load per launch.
// A record is ROUTE_REC_INTS ints: kernel, sched, bm, bn, ks, stride, asym (Ho / Wo exceed the symmetric formula), act, residual kind
// (0 none, 1 storage type, 2 f32), out_f32, aligned8 (Cout, out_coff, out_cstride all multiples of 8), then the layer's shape
// B, Hin, Win, Cin, Cout, Ho, Wo, then what picks the K loop: split (two weight planes), simple, two, cprw, ns of the ConvChoice.
constexpr int ROUTE_REC_INTS = 23;
extern std::atomic<int> g_route_log;
void route_log_append(const ConvP& p, const ConvChoice& c);
int route_log_take(int* recs, int cap);                // moves up to `cap` records out (the rest stay), returns how many the list held

// CLEARCAM_* selection switches, read from the environment once per process (thread-safe static initialisation)
struct ConvSwitches {
  int stream, stream_min_pix, stream_flags;   // CLEARCAM_STREAM (1), CLEARCAM_STREAM_MIN_PIX (200000), CLEARCAM_STREAM_FLAGS (10)
  int ws, small_tiles, small_pix, wave;       // CLEARCAM_WS, CLEARCAM_SMALL_TILES, CLEARCAM_SMALL_PIX, CLEARCAM_WAVE (1 each)
  int tile64, tile64_w;                       // CLEARCAM_TILE64 (1), CLEARCAM_TILE64_W (0: the width rule)
  int big_tile, phase, phase_flags;           // CLEARCAM_BIG_TILE (1), CLEARCAM_PHASE (2), CLEARCAM_PHASE_FLAGS (-1: the default rule)
};
const ConvSwitches& conv_switches();

// cc_dev_set overrides: -1 = the environment / default.  Read at every choice, so a cc_dev_set call wins at any time.
extern std::atomic<int> g_stream_override, g_phase_flags_override, g_tile64_w_override, g_stream_flags_override;
extern std::atomic<int> g_stream_abl, g_tile64_abl;   // timing ablations of development builds (0 = off)

}  // namespace cc
