// One 64 x 64 tile of dot products of stored index rows: what gram_kernel (index_distinct.hip) and digest_leaders_kernel
// (index_digest.hip) share.  Both gather their rows with stage_rows, run gram_tile_accumulate and, where they compare, gram_tile_bits,
// so an element is the same float wherever it is computed: ONE chain of fused multiply-adds over k on the exact f32 MFMA (16x16x4), in
// an order that is the same for every element of every tile, and a * b is commutative.  The value of a pair depends on its two stored
// rows alone - not on the tile, the side of the tile, the kernel or the other rows of the launch.  sightings_kernel (index_sightings.hip)
// stages with stage_rows and feeds each of its accumulators the same MFMAs in the same order over a 128-row tile of its own.
#pragma once
#include "kernels.h"
#include "mfma.h"

namespace cc {

constexpr int kGramTile = 64;                   // rows and columns of a tile: one tile row = one 64-bit word of a bit matrix
constexpr int kGramBK = 64;                     // floats of K staged per step
constexpr int kGramLd = kGramBK + 4;            // LDS row stride in floats: 16-byte aligned, the 16 rows of a fragment read on 64 distinct banks

#if defined(__HIPCC__)
// ROWS rows x kGramBK floats of K from k0 on -> dst[ROWS][kGramLd].  A row outside the list or the index, and K past dim, are zeros.
template <int STORAGE, int ROWS = kGramTile>
__device__ __forceinline__ void stage_rows(const char* __restrict__ emb, long size, int dim, const long long* srow, int k0, float* dst, int tid) {
  constexpr int FP = STORAGE == F32 ? 4 : STORAGE == BF16 ? 8 : 16;   // floats in one 16-byte piece of the stored row
  constexpr int PPR = kGramBK / FP;
  for (int e = tid; e < ROWS * PPR; e += 256) {
    const int r = e / PPR, k = k0 + (e % PPR) * FP;
    float4 f[FP / 4];
#pragma unroll
    for (int i = 0; i < FP / 4; ++i) f[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const long long row = srow[r];
    if ((unsigned long long)row < (unsigned long long)size && k < dim) {
      if (STORAGE == F32) f[0] = *reinterpret_cast<const float4*>(emb + ((size_t)row * dim + k) * 4);
      else if (STORAGE == BF16) decode_bf16_piece(*reinterpret_cast<const uint4*>(emb + ((size_t)row * dim + k) * 2), f);
      else {
        const char* er = emb + (size_t)row * ((size_t)dim + (dim >> 3));
        decode_i8_piece(*reinterpret_cast<const uint4*>(er + k), reinterpret_cast<const float*>(er + dim)[k >> 5], f);
      }
    }
    float4* o = reinterpret_cast<float4*>(dst + r * kGramLd + (e % PPR) * FP);
#pragma unroll
    for (int i = 0; i < FP / 4; ++i) o[i] = f[i];
  }
}

// The K loop of a 256-thread block: srow[0 .. 63] are the rows of the tile's rows, srow[64 .. 127] those of its columns; As / Bs hold
// kGramTile * kGramLd floats each.  Wave w owns the 32 x 32 quadrant (wr = w >> 1, wc = w & 1); accumulator element r of acc[m][c2]:
// tile row wr * 32 + m * 16 + (lane >> 4) * 4 + r, tile column wc * 32 + c2 * 16 + (lane & 15).  Ends with a barrier: As is free.
template <int STORAGE>
__device__ __forceinline__ void gram_tile_accumulate(const char* __restrict__ emb, long size, int dim, const long long* srow, float* As, float* Bs, int tid,
                                                     f32x4 (&acc)[2][2]) {
  const int lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[m][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < dim; k0 += kGramBK) {
    stage_rows<STORAGE>(emb, size, dim, srow, k0, As, tid);
    stage_rows<STORAGE>(emb, size, dim, srow + kGramTile, k0, Bs, tid);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kGramBK / 16; ++c) {
      uint4 a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = *reinterpret_cast<const uint4*>(As + (wr * 32 + m * 16 + (lane & 15)) * kGramLd + c * 16 + (lane >> 4) * 4);
        b[m] = *reinterpret_cast<const uint4*>(Bs + (wc * 32 + m * 16 + (lane & 15)) * kGramLd + c * 16 + (lane >> 4) * 4);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) Mma<float>::run(a[m], b[c2], acc[m][c2]);
    }
    __syncthreads();
  }
}

// The compare epilogue: every element against same_at, the 64 answers of tile row r -> one word.  `fl` is kGramTile * kGramTile bytes
// of LDS (As behind gram_tile_accumulate).  Returns, in lanes 0 .. 15 of wave w, the word of tile row w * 16 + lane; other lanes 0.
__device__ __forceinline__ unsigned long long gram_tile_bits(const f32x4 (&acc)[2][2], float same_at, unsigned char* fl, int tid) {
  const int lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        fl[(wr * 32 + m * 16 + (lane >> 4) * 4 + r) * kGramTile + wc * 32 + c2 * 16 + (lane & 15)] = acc[m][c2][r] >= same_at ? 1 : 0;
  __syncthreads();
  unsigned long long mine = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const unsigned long long word = __ballot(fl[(wave * 16 + r) * kGramTile + lane] != 0);
    if (lane == r) mine = word;
  }
  return mine;
}
#endif

}  // namespace cc
