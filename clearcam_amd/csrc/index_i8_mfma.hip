// Batches of queries against int8-stored index rows (CC_INDEX_I8) on the matrix cores: one launch scores every query of the batch
// against every row, and a row comes from HBM once.  index.hip's compute_scores chooses between this kernel and the scan passes.
//
// The arithmetic is the scan's, in another order.  An int8 code (|c| <= 127) is exact in bf16.  A query stays f32: it is split once
// per call into three bf16 planes, hi = bf16(q), mid = bf16(q - hi), lo = bf16(q - hi - mid), whose sum is q bit for bit (24
// significand bits in 3 x 8, and bf16 has the exponent range of f32), so every product plane x code is exact in f32.  One
// v_mfma_f32_16x16x32_bf16 spans K = 32 = exactly ONE scale group of a row: per group the three planes accumulate into a fresh f32
// partial, then acc = fmaf(partial, scale, acc) in f32, the step scan_i8_kernel takes.  The scale is never folded into a 16-bit
// operand, so a one-hot query still returns round_f32(code * scale) exactly.
//
// Roles: queries on the A side, index rows on the B side.  Lane l holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15], and
// of C/D the column l & 15, rows 4 (l >> 4) + reg: a lane's four accumulators are four queries of ONE index row, and a group's scale
// is one value per lane.
//
// Shape of the kernel: a workgroup of four waves takes a tile of kTile = 256 rows, 64 per wave (four 16-row sets), and walks the row
// in chunks of 256 codes (eight groups) like the scan does.  A chunk of the tile (256 B of codes + 32 B of scales per row) is staged
// into LDS by coalesced 16-byte loads (16 lanes cover one row's 256 B, as in scan_i8_kernel) and read back transposed, 8 bytes per
// lane: LDS is what turns "consecutive lanes = consecutive bytes of a row" into "consecutive lanes = consecutive rows".  The code
// image has a row stride of 272 B = 68 dwords, so the 16 rows of a ds_read_b64 start 4 banks apart and the four lane quarters 2
// banks apart: no conflict.  76 KB of LDS per workgroup, single-buffered: TWO workgroups share a CU and one computes while the
// other loads.  The A fragments come from the plane buffer, which the pre-kernel writes in fragment order and in the order of the
// walk (a wave's load of one plane of a fragment is 1 KB contiguous, and the next fragment is the next 3 KB) and L2 holds: 12 KB per
// group for 64 queries, read once per wave and 64 rows, each fragment asked for one step (12 MFMAs) before it is multiplied.
// A pass holds up to 64 queries (4 x 4 x 4 accumulators); a larger batch walks the same tile again for the next 64, with the rows
// then served by the caches, not by HBM.  Measured (docs/measurement.md, "int8 rows"): 1 M x 768, 64 queries, search(q, 100) in
// 0.82 ms where scan passes take 3.1 ms and bf16 rows 0.70 ms; the time grows by about 0.14 ms per 16 queries, four times the MFMA
// issue time, which points at the A loads' latency and the VALU work beside the MFMAs.  A ring of four fragments (three steps ahead)
// spilled inside the loop at 256 registers and was not kept.
#include <type_traits>
#include "kernels.h"
#include "mfma.h"

namespace cc {

namespace {

constexpr int kTile = 256;                    // rows per workgroup tile: 4 waves x kSets x 16
constexpr int kSets = 4;                      // 16-row sets per wave
constexpr int kCodeStride = 272;              // bytes per row of the LDS code image: 256 + 16 of padding (see above)
constexpr int kLdsBytes = kTile * kCodeStride + kTile * 32;

// The plane buffer in the order the score kernel walks it.  Query tiles go in passes of four (the last pass has what is left, nt tiles);
// pass P starts at fragment 4 P G, and inside it the fragment of group g, tile t is number g * nt + t.  A fragment is three planes
// (0 hi, 1 mid, 2 lo) of 64 lanes x 16 bytes: lane `lane` holds, of query 16 qt + (lane & 15), the elements 32 g + 8 (lane >> 4) + j,
// j = 0..7 - what it feeds as A.  Queries >= Q are zero.
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ q, uint4* __restrict__ planes, int Q, int dim, long cnt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;         // (qt, g, lane)
  if (i >= cnt) return;
  const int lane = (int)(i & 63), G = dim >> 5;
  const int g = (int)((i >> 6) % G), qt = (int)((i >> 6) / G);
  const int qi = qt * 16 + (lane & 15);
  unsigned w[3][4] = {};
  if (qi < Q) {
    const float* src = q + (size_t)qi * dim + 32 * g + 8 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = src[j];
      const uint16_t hi = f32_to_bf16_bits(x);
      const float r1 = x - bf16_bits_to_f32(hi);                // exact
      const uint16_t mid = f32_to_bf16_bits(r1);
      const float r2 = r1 - bf16_bits_to_f32(mid);              // exact, and itself a bf16 value
      const uint16_t lo = f32_to_bf16_bits(r2);
      const int sh = 16 * (j & 1);
      w[0][j >> 1] |= (unsigned)hi << sh; w[1][j >> 1] |= (unsigned)mid << sh; w[2][j >> 1] |= (unsigned)lo << sh;
    }
  }
  const int qtiles = (Q + 15) >> 4, pass = qt >> 2, nt = min(4, qtiles - 4 * pass);
  const size_t frag = (size_t)4 * pass * G + (size_t)g * nt + (qt & 3);
#pragma unroll
  for (int p = 0; p < 3; ++p) planes[frag * 192 + p * 64 + lane] = make_uint4(w[p][0], w[p][1], w[p][2], w[p][3]);
}

__device__ __forceinline__ unsigned bf16_pair(unsigned w, int b) {            // codes b and b + 1 of w as two bf16 (exact)
  const float f0 = (float)((int)(w << (24 - 8 * b)) >> 24), f1 = (float)((int)(w << (16 - 8 * b)) >> 24);
  return (__float_as_uint(f0) >> 16) | (__float_as_uint(f1) & 0xffff0000u);
}

struct TileArgs {
  const char* emb; const uint4* planes; float* out;
  long n, r0; int dim, Q, last;                 // r0: the tile's first row, last: its last row that exists, counted from r0
  char* codes; float* scales;                   // the LDS images
};

// One pass of one tile: NT query tiles of 16 (from tile qt0 on) against the tile's 256 rows.
template <int NT>
__device__ __forceinline__ void tile_pass(const TileArgs& k, int qt0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int steps = k.dim >> 8, G = k.dim >> 5;
  const unsigned rb = (unsigned)k.dim + (k.dim >> 3);
  f32x4 acc[kSets][NT];
#pragma unroll
  for (int rs = 0; rs < kSets; ++rs)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rs][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // The A fragments are walked step by step (group by group, inside a group query tile by query tile: step s = g * NT + t) through
  // two halves, a[s & 1][plane]: the fragment of step s + 1 is asked for when step s is multiplied.  A pair of groups has 2 * NT steps,
  // so inside a pair every s & 1 is a compile-time constant and a[] stays in registers.
  uint4 a[2][3];
  const int S = G * NT;
  auto load_a = [&](uint4* dst, int s) {
    if (s < S) {
      const uint4* at = k.planes + ((size_t)qt0 * G + s) * 192 + lane;        // a pass's fragments lie in the order of its walk
      dst[0] = at[0]; dst[1] = at[64]; dst[2] = at[128];
    }
  };
  load_a(a[0], 0);
  // A lane's 16 code pieces are 16 bytes of rows (tid >> 4) + 16 i, its 2 scale pieces 16 bytes of rows (tid >> 1) + 128 i.  Rows past the
  // end of the index are read from the tile's last row (their scores are never stored).
  const char* src = k.emb + (size_t)k.r0 * rb;
  for (int st = 0; st < steps; ++st) {
    __syncthreads();                                              // the previous chunk has been read by every wave
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = i * 16 + (tid >> 4);
      *reinterpret_cast<uint4*>(k.codes + row * kCodeStride + (tid & 15) * 16) =
          *reinterpret_cast<const uint4*>(src + ((unsigned)min(row, k.last) * rb + (unsigned)(st * 256 + (tid & 15) * 16)));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = i * 128 + (tid >> 1);
      *reinterpret_cast<uint4*>(k.scales + row * 8 + (tid & 1) * 4) =
          *reinterpret_cast<const uint4*>(src + ((unsigned)min(row, k.last) * rb + (unsigned)(k.dim + st * 32 + (tid & 1) * 16)));
    }
    __syncthreads();
    // one group; gi = its number inside the chunk modulo two (a compile-time constant)
    auto group = [&](int gl, auto gi_) {
      constexpr int gi = decltype(gi_)::value;
      uint4 b[kSets]; float sc[kSets];
#pragma unroll
      for (int rs = 0; rs < kSets; ++rs) {
        const int row = wave * 64 + rs * 16 + col;
        const uint2 w = *reinterpret_cast<const uint2*>(k.codes + row * kCodeStride + gl * 32 + quad * 8);
        b[rs] = make_uint4(bf16_pair(w.x, 0), bf16_pair(w.x, 2), bf16_pair(w.y, 0), bf16_pair(w.y, 2));
        sc[rs] = k.scales[row * 8 + gl];
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int slot = (gi * NT + t) & 1;                       // folds: t is unrolled
        load_a(a[1 - slot], (st * 8 + gl) * NT + t + 1);          // the next step's fragment travels while this one is multiplied
        const uint4* at = a[slot];
#pragma unroll
        for (int rs = 0; rs < kSets; ++rs) {
          f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};                 // smallest plane first
          Mma<bf16_t>::run(at[2], b[rs], part);
          Mma<bf16_t>::run(at[1], b[rs], part);
          Mma<bf16_t>::run(at[0], b[rs], part);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[rs][t][r] = fmaf(part[r], sc[rs], acc[rs][t][r]);
        }
      }
    };
#pragma unroll 1
    for (int gl = 0; gl < 8; gl += 2) {
      group(gl, std::integral_constant<int, 0>());
      group(gl + 1, std::integral_constant<int, 1>());
    }
  }
#pragma unroll
  for (int rs = 0; rs < kSets; ++rs) {
    const long row = k.r0 + wave * 64 + rs * 16 + col;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = (qt0 + t) * 16 + quad * 4 + r;
        if (row < k.n && qi < k.Q) k.out[(size_t)qi * k.n + row] = acc[rs][t][r];
      }
  }
}

__global__ __launch_bounds__(256, 2) void index_i8_mfma_kernel(const char* __restrict__ emb, const uint4* __restrict__ planes, float* __restrict__ out,
                                                               long n, int dim, int Q, int qtiles) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  TileArgs k;
  k.emb = emb; k.planes = planes; k.out = out; k.n = n; k.dim = dim; k.Q = Q;
  k.codes = lds; k.scales = reinterpret_cast<float*>(lds + kTile * kCodeStride);
  const long tiles = (n + kTile - 1) / kTile;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    k.r0 = tile * kTile;
    k.last = (int)min((long)kTile, n - k.r0) - 1;
    for (int qt0 = 0; qt0 < qtiles; qt0 += 4)
      switch (min(4, qtiles - qt0)) {                             // uniform over the grid
        case 1: tile_pass<1>(k, qt0); break;
        case 2: tile_pass<2>(k, qt0); break;
        case 3: tile_pass<3>(k, qt0); break;
        default: tile_pass<4>(k, qt0); break;
      }
  }
}

}  // namespace

bool index_i8_mfma_supported(int dim, long n) { return dim % 256 == 0 && dim <= kIndexI8MfmaMaxDim && n >= 1 && n < (1L << 31); }

size_t index_i8_mfma_plane_bytes(int dim, int Q) { return (size_t)((Q + 15) / 16 * 16) * dim * 6; }

void launch_index_i8_mfma(const void* emb, const float* q, void* planes, float* out, long n, int dim, int Q, hipStream_t s) {
  const int qtiles = (Q + 15) / 16;
  const long cnt = (long)qtiles * (dim >> 5) * 64;
  hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, q, reinterpret_cast<uint4*>(planes), Q, dim, cnt);
  ensure_max_lds(index_i8_mfma_kernel, kLdsBytes);
  const long tiles = (n + kTile - 1) / kTile;
  const int blocks = (int)std::min<long>(tiles, 2L * cu_count());   // two workgroups per CU: one sweep of the grid is 512 rows per CU
  hipLaunchKernelGGL(index_i8_mfma_kernel, dim3(blocks), dim3(256), kLdsBytes, s, reinterpret_cast<const char*>(emb), reinterpret_cast<const uint4*>(planes),
                     out, n, dim, Q, qtiles);
  CC_HIP(hipGetLastError());
}

}  // namespace cc
