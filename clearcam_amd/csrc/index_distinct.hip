// Distinct ranking on the embedding index: the pairwise similarities of stored rows (cc_index_gram) and the greedy thinning of ranked
// lists built on them (cc_index_distinct).  The C entry points stand with the handle in index.hip; this file holds the kernels.
//
// Three launches thin Q lists of up to 1024 entries:
//   squeeze_kernel   one block per list: the present entries (0 <= idx < size) moved to the front in order, with their places.
//   gram_kernel      one block per 64 x 64 tile of the upper triangle of a list's Gram matrix.  The rows are gathered straight from the
//                    stored form (decode_*_piece of kernels.h, the rule of fetch_rows_kernel), staged in LDS as f32 and multiplied on
//                    the exact f32 MFMA (16x16x4).  Every element is ONE chain of fused multiply-adds over k in an order that is the
//                    same for every element of every tile: the value of a pair depends on its two rows alone, and since a * b is
//                    commutative it does not depend on which of the two stands first either.  Only tiles with tj >= ti are computed.
//                    Epilogue FLOATS (cc_index_gram): the element is stored at [i][j] and at [j][i], so the matrix is symmetric bit for
//                    bit by construction.  Epilogue BITS (cc_index_distinct): the element is compared with same_at and the 64 answers
//                    of a tile row become one 64-bit word of the list's bit matrix (1024 rows x 16 words = 128 KB instead of 4 MB of
//                    floats).  Both epilogues sit behind the same accumulation, so a bit is the comparison of the very float the other
//                    epilogue would store.
//   walk_kernel      one block per list.  All threads load the bit matrix into LDS, cleared where the walk must not look: at and
//                    below the diagonal, past the last present entry, and in the tiles below the diagonal, which nobody wrote.
//                    One wave then walks the entries in order, lane w holding word w of the dropped set: entry j is kept iff its bit
//                    is clear, and a kept entry ORs its row into the set.  The bits a kept row ADDS are exactly the entries it is the
//                    first keeper of; they are written back over the row, and their count is its `dups`.  All threads then place
//                    the kept entries (rank = popcount of the kept bits before them), cut the window and pad it.
// Nothing here uses atomics: every word and every output has one writer.
// The staging, the K loop and the compare epilogue of gram_kernel stand in gram_tile.h: the day digest (index_digest.hip) runs its tiles of
// rows against leaders through the same code, so that it compares the very floats cc_index_gram returns.
#include "gram_tile.h"
#include "../../include/clearcam_hip.h"

namespace cc {

namespace {

constexpr int kTile = kGramTile, kLd = kGramLd;                               // gram_tile.h: the tile, its staging and its one accumulation
constexpr size_t kWalkLds = (size_t)kDistinctMaxDepth * kDistinctWords * 8;   // the bit matrix of one list

static_assert(CC_DISTINCT_MAX_DEPTH == kDistinctMaxDepth, "the header and kernels.h disagree");
static_assert(kDistinctMaxDepth == 1024, "squeeze_kernel and walk_kernel run one thread per entry in one block");

__global__ __launch_bounds__(1024) void squeeze_kernel(const int* __restrict__ idx, int depth, long size, long long* __restrict__ rows, int* __restrict__ pos,
                                                       int* __restrict__ present) {
  __shared__ int wcnt[16];
  const int t = threadIdx.x, q = blockIdx.x, lane = t & 63, wave = t >> 6;
  const int v = t < depth ? idx[(size_t)q * depth + t] : -1;
  const bool ok = v >= 0 && (long)v < size;
  const unsigned long long b = __ballot(ok);
  if (lane == 0) wcnt[wave] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) { before += w < wave ? wcnt[w] : 0; all += wcnt[w]; }
  const int p = before + __popcll(b & ((1ull << lane) - 1));
  if (ok) { rows[(size_t)q * kDistinctMaxDepth + p] = v; pos[(size_t)q * kDistinctMaxDepth + p] = t; }
  if (t == 0) present[q] = all;
}

// grid (tiles, tiles, lists), 256 threads: wave w owns the 32 x 32 quadrant (w >> 1, w & 1) of tile (ti = blockIdx.y, tj = blockIdx.x).
template <int STORAGE, bool BITS>
__global__ __launch_bounds__(256) void gram_kernel(const char* __restrict__ emb, long size, int dim, const long long* __restrict__ rows, int n_fixed,
                                                   const int* __restrict__ present, float* __restrict__ out, unsigned long long* __restrict__ bits,
                                                   float same_at) {
  __shared__ __attribute__((aligned(16))) float As[kTile * kLd];
  __shared__ __attribute__((aligned(16))) float Bs[kTile * kLd];
  __shared__ long long srow[2 * kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int ti = blockIdx.y, tj = blockIdx.x, q = blockIdx.z;
  const int n = present ? present[q] : n_fixed;
  if (tj < ti || tj * kTile >= n) return;                       // the whole block: below the diagonal, or past the list
  rows += (size_t)q * kDistinctMaxDepth;
  if (tid < 2 * kTile) {
    const int li = (tid < kTile ? ti * kTile : tj * kTile - kTile) + tid;
    srow[tid] = li < n ? rows[li] : -1;
  }
  __syncthreads();
  f32x4 acc[2][2];
  gram_tile_accumulate<STORAGE>(emb, size, dim, srow, As, Bs, tid, acc);
  // accumulator element r of tile (m, c2): row (lane >> 4) * 4 + r, column lane & 15
  if (!BITS) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = ti * kTile + wr * 32 + m * 16 + (lane >> 4) * 4 + r, gj = tj * kTile + wc * 32 + c2 * 16 + (lane & 15);
          if (gi < n && gj < n && gj >= gi) {
            const float v = acc[m][c2][r];
            out[(size_t)gi * n + gj] = v;
            out[(size_t)gj * n + gi] = v;
          }
        }
  } else {
    const unsigned long long mine = gram_tile_bits(acc, same_at, reinterpret_cast<unsigned char*>(As), tid);   // the K loop ended with a barrier
    const int gi = ti * kTile + wave * 16 + lane;
    if (lane < 16 && gi < n) bits[((size_t)q * kDistinctMaxDepth + gi) * kDistinctWords + tj] = mine;
  }
}

__global__ __launch_bounds__(1024) void walk_kernel(const unsigned long long* __restrict__ bits, const long long* __restrict__ rows, const int* __restrict__ pos,
                                                    const int* __restrict__ present, const float* __restrict__ score, int depth, long long start, long long count,
                                                    int* __restrict__ out_idx, float* __restrict__ out_score, int* __restrict__ out_dups,
                                                    long long* __restrict__ kept_out) {
  extern __shared__ unsigned long long sb[];                    // [n][16]: the bit matrix, then per kept row the entries it dropped
  __shared__ unsigned long long skeep[kDistinctWords];
  const int tid = threadIdx.x, q = blockIdx.x;
  const int n = present[q];
  bits += (size_t)q * kDistinctMaxDepth * kDistinctWords;
  for (int e = tid; e < n * kDistinctWords; e += 1024) {
    const int i = e >> 4, w = e & 15;
    unsigned long long v = 0;
    if (w >= (i >> 6) && w * 64 < n) {                          // a tile the Gram epilogue of THIS call wrote
      v = bits[e];
      if (w == (i >> 6)) v &= ~((2ull << (i & 63)) - 1);        // only entries behind i
      if (n - w * 64 < 64) v &= (1ull << (n - w * 64)) - 1;     // only present entries
    }
    sb[e] = v;
  }
  __syncthreads();
  if (tid < 64) {                                               // lanes 16 .. 63 mirror lanes 0 .. 15
    const int lw = tid & 15;
    unsigned long long drop = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned long long rowbits = sb[j * kDistinctWords + lw];
      const unsigned lo = __builtin_amdgcn_readlane((unsigned)drop, j >> 6), hi = __builtin_amdgcn_readlane((unsigned)(drop >> 32), j >> 6);
      const bool kept = !(((j & 32 ? hi : lo) >> (j & 31)) & 1u);
      const unsigned long long newly = kept ? rowbits & ~drop : 0ull;
      drop |= newly;
      if (tid < kDistinctWords) sb[j * kDistinctWords + lw] = newly;
    }
    if (tid < kDistinctWords) {
      unsigned long long k = ~drop;
      if (tid * 64 >= n) k = 0;
      else if (n - tid * 64 < 64) k &= (1ull << (n - tid * 64)) - 1;
      skeep[tid] = k;
    }
  }
  __syncthreads();
  int total = 0, before = 0;
#pragma unroll
  for (int w = 0; w < kDistinctWords; ++w) { const int c = __popcll(skeep[w]); total += c; before += w < (tid >> 6) ? c : 0; }
  if (tid < n && ((skeep[tid >> 6] >> (tid & 63)) & 1ull)) {
    const long long p = before + __popcll(skeep[tid >> 6] & ((1ull << (tid & 63)) - 1)) - start;
    if (p >= 0 && p < count) {
      const size_t o = (size_t)q * count + p;
      out_idx[o] = (int)rows[(size_t)q * kDistinctMaxDepth + tid];
      if (out_score) out_score[o] = score[(size_t)q * depth + pos[(size_t)q * kDistinctMaxDepth + tid]];
      if (out_dups) {
        int d = 0;
#pragma unroll
        for (int w = 0; w < kDistinctWords; ++w) d += __popcll(sb[tid * kDistinctWords + w]);
        out_dups[o] = d;
      }
    }
  }
  const long long first = total > start ? (total - start < count ? total - start : count) : 0;
  for (long long p = first + tid; p < count; p += 1024) {
    const size_t o = (size_t)q * count + p;
    out_idx[o] = -1;
    if (out_score) out_score[o] = -__builtin_huge_valf();
    if (out_dups) out_dups[o] = 0;
  }
  if (tid == 0) kept_out[q] = total;
}

template <bool BITS>
void launch_gram(const void* emb, long size, int dim, int storage, const long long* rows, int n, const int* present, int Q, float* out,
                 unsigned long long* bits, float same_at, hipStream_t s) {
  const int T = (n + kTile - 1) / kTile;
  const dim3 grid(T, T, Q), block(256);
  const char* e = static_cast<const char*>(emb);
  if (storage == F32) hipLaunchKernelGGL((gram_kernel<F32, BITS>), grid, block, 0, s, e, size, dim, rows, n, present, out, bits, same_at);
  else if (storage == BF16) hipLaunchKernelGGL((gram_kernel<BF16, BITS>), grid, block, 0, s, e, size, dim, rows, n, present, out, bits, same_at);
  else hipLaunchKernelGGL((gram_kernel<CC_INDEX_I8, BITS>), grid, block, 0, s, e, size, dim, rows, n, present, out, bits, same_at);
  CC_HIP(hipGetLastError());
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

size_t distinct_ws_bytes(int Q) {
  const size_t e = (size_t)Q * kDistinctMaxDepth;
  return up256(e * kDistinctWords * 8) + up256(e * 8) + up256(e * 4) + up256((size_t)Q * 8) + up256((size_t)Q * 4);
}

DistinctWs distinct_ws(void* base, int Q) {
  const size_t e = (size_t)Q * kDistinctMaxDepth;
  char* p = static_cast<char*>(base);
  DistinctWs ws;
  ws.bits = reinterpret_cast<unsigned long long*>(p); p += up256(e * kDistinctWords * 8);
  ws.rows = reinterpret_cast<long long*>(p); p += up256(e * 8);
  ws.pos = reinterpret_cast<int*>(p); p += up256(e * 4);
  ws.kept = reinterpret_cast<long long*>(p); p += up256((size_t)Q * 8);
  ws.present = reinterpret_cast<int*>(p);
  return ws;
}

void launch_index_gram(const void* emb, long size, int dim, int storage, const long long* rows, int n, float* out, hipStream_t stream) {
  launch_gram<false>(emb, size, dim, storage, rows, n, nullptr, 1, out, nullptr, 0.f, stream);
}

void launch_index_gram_bits(const void* emb, long size, int dim, int storage, const long long* rows, int n, unsigned long long* bits, float same_at,
                            hipStream_t stream) {
  launch_gram<true>(emb, size, dim, storage, rows, n, nullptr, 1, nullptr, bits, same_at, stream);
}

void launch_index_distinct(const void* emb, long size, int dim, int storage, const int* idx, const float* score, int Q, int depth, float same_at,
                           long long start, long long count, const DistinctWs& ws, int* out_idx, float* out_score, int* out_dups, hipStream_t stream) {
  hipLaunchKernelGGL(squeeze_kernel, dim3(Q), dim3(1024), 0, stream, idx, depth, size, ws.rows, ws.pos, ws.present);
  CC_HIP(hipGetLastError());
  launch_gram<true>(emb, size, dim, storage, ws.rows, depth, ws.present, Q, nullptr, ws.bits, same_at, stream);
  ensure_max_lds(walk_kernel, kWalkLds);
  hipLaunchKernelGGL(walk_kernel, dim3(Q), dim3(1024), kWalkLds, stream, ws.bits, ws.rows, ws.pos, ws.present, score, depth, start, count, out_idx,
                     score ? out_score : nullptr, out_dups, ws.kept);
  CC_HIP(hipGetLastError());
}

}  // namespace cc
