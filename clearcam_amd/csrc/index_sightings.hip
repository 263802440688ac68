// Seen before? (cc_index_sightings): up to 1024 stored rows (the objects) against all competing rows, reduced per object to the number
// of pairs at or above same_at, the best pair and the matching pairs per group.  The C entry point stands with the handle in index.hip;
// this file holds the scoring kernel and the finish.  The selection of the competing rows is the digest's (launch_digest_select).
//
// The pair value is the float cc_index_gram returns: every element of every tile here is ONE accumulator fed by the 16x16x4 f32 MFMAs
// of gram_tile_accumulate in its order (K in steps of 16 floats, ascending, up to dim rounded up to kGramBK with zeros; the four MFMAs
// of a step take floats j, 4 + j, 8 + j, 12 + j), read from LDS rows laid out by stage_rows.  Only the shape of the tile differs.
//
//   sightings_kernel<STORAGE, NT>   256 threads, a tile of 128 competing rows (a strip) x 16 * NT objects; wave w owns strip rows
//                    32 w .. 32 w + 31 against all objects of the tile: acc[2][NT], one LDS read of A feeds NT MFMA groups.  NT = 8
//                    (128 objects) is the MFMA-bound end, NT = 4 and 1 (64 / 16 objects) spend less of the pipe on padding when few
//                    objects make the call HBM-bound: then the strips come from HBM exactly once.  With more than one object tile a
//                    strip is read once per object tile, by blocks that run at the same time, so HBM serves it once and the caches
//                    the rest; the objects (at most 3 MB decoded) are the side that is re-read per strip, from L2.
//                    The grid is persistent: a block keeps ONE object tile (blockIdx % object tiles) and walks the strips
//                    blockIdx / object tiles, + blocks per object tile, ...; the number of competing rows is read on the device.
//                    Per tile each wave reduces its 32 rows per object in registers and across its four lane groups, then adds
//                    the count and raises the key ordered(g) << 32 | ~row in the block's LDS tables (integer sum, integer maximum:
//                    order-free; the largest g, among equal g the lowest row).  The tables go to the global ones once, when the block
//                    has walked its strips: blocks x objects-per-tile atomics in all, not strips x objects.
//                    Group counts: matches are sparse, so they go to global memory as they are found - one atomic per wave and
//                    object where the strip is all one group (folders are contiguous in ingest order), one per match otherwise.
//   sightings_finish_kernel   keys -> out_best_row / out_best_score (-1 / -inf where an object met no pair).
#include "gram_tile.h"
#include "../../include/clearcam_hip.h"

namespace cc {

namespace {

static_assert(CC_SIGHT_MAX_OBJECTS == kSightMaxObjects && CC_SIGHT_MAX_GROUPS == kSightMaxGroups, "the header and kernels.h disagree");

constexpr int kSightStrip = 128;                                // competing rows of a tile

__device__ __forceinline__ unsigned sight_ordered(float f) {   // monotone float -> uint, the ranking keys' order (index.hip)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sight_unordered(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

constexpr size_t sight_lds(int NT) { return (size_t)(kSightStrip + 16 * NT) * kGramLd * 4; }

template <int STORAGE, int NT>
__global__ __launch_bounds__(256) void sightings_kernel(const char* __restrict__ emb, long size, int dim, const long long* __restrict__ sel,
                                                        const int* __restrict__ m_ptr, const long long* __restrict__ obj, int n_obj, int n_ot,
                                                        float same_at, int skip_self, const int* __restrict__ grp, int n_gc,
                                                        int* __restrict__ out_count, unsigned long long* __restrict__ best,
                                                        unsigned* __restrict__ gc) {
  constexpr int TN = 16 * NT;
  extern __shared__ __attribute__((aligned(16))) float tile[];  // As[kSightStrip][kGramLd], Bs[TN][kGramLd]
  __shared__ long long srow_a[kSightStrip], srow_b[TN];
  __shared__ int sgrp[kSightStrip];
  __shared__ int scnt[TN];
  __shared__ unsigned long long sbest[TN];
  float* As = tile;
  float* Bs = tile + kSightStrip * kGramLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ot = blockIdx.x % n_ot, per_ot = gridDim.x / n_ot;  // the grid is a multiple of n_ot
  const long m = *m_ptr;
  if (tid < TN) {
    const int oi = ot * TN + tid;
    srow_b[tid] = oi < n_obj ? obj[oi] : -1;
    scnt[tid] = 0; sbest[tid] = 0ull;
  }
  const int kend = (dim + kGramBK - 1) / kGramBK * kGramBK;
  for (long strip = blockIdx.x / n_ot; strip * kSightStrip < m; strip += per_ot) {
    if (tid < kSightStrip) {
      const long li = strip * kSightStrip + tid;
      const long long r = li < m ? sel[li] : -1;
      srow_a[tid] = r;
      sgrp[tid] = (gc && r >= 0) ? grp[r] : -1;
    }
    __syncthreads();
    const int g0 = sgrp[0];                                     // row 0 of a strip competes
    const int one_group = __syncthreads_and(tid >= kSightStrip || srow_a[tid] < 0 || sgrp[tid] == g0);
    f32x4 acc[2][NT];
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
      for (int c = 0; c < NT; ++c) acc[mm][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kend; k0 += kGramBK) {
      stage_rows<STORAGE, kSightStrip>(emb, size, dim, srow_a, k0, As, tid);
      stage_rows<STORAGE, TN>(emb, size, dim, srow_b, k0, Bs, tid);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < kGramBK / 16; ++c) {
        uint4 a[2], b[NT];
#pragma unroll
        for (int mm = 0; mm < 2; ++mm) a[mm] = *reinterpret_cast<const uint4*>(As + (wave * 32 + mm * 16 + (lane & 15)) * kGramLd + c * 16 + (lane >> 4) * 4);
#pragma unroll
        for (int c2 = 0; c2 < NT; ++c2) b[c2] = *reinterpret_cast<const uint4*>(Bs + (c2 * 16 + (lane & 15)) * kGramLd + c * 16 + (lane >> 4) * 4);
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
          for (int c2 = 0; c2 < NT; ++c2) Mma<float>::run(a[mm], b[c2], acc[mm][c2]);
      }
      __syncthreads();
    }
    // acc[mm][c2][r]: strip row wave * 32 + mm * 16 + (lane >> 4) * 4 + r, object c2 * 16 + (lane & 15)
#pragma unroll
    for (int c2 = 0; c2 < NT; ++c2) {
      const int col = c2 * 16 + (lane & 15), oi = ot * TN + col;
      const long long orow = srow_b[col];
      int cnt = 0;
      unsigned long long key = 0ull;
#pragma unroll
      for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int li = wave * 32 + mm * 16 + (lane >> 4) * 4 + r;
          const long long crow = srow_a[li];
          if (crow < 0 || orow < 0 || (skip_self && crow == orow)) continue;
          const float g = acc[mm][c2][r];
          const unsigned long long k = ((unsigned long long)sight_ordered(g) << 32) | (unsigned)(~(unsigned)crow);
          key = k > key ? k : key;
          if (g >= same_at) {
            ++cnt;
            if (gc && !one_group) {
              const unsigned gg = (unsigned)sgrp[li];
              if (gg < (unsigned)n_gc) atomicAdd(&gc[(size_t)oi * n_gc + gg], 1u);
            }
          }
        }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        const unsigned long long k = __shfl_xor(key, o, 64);
        key = k > key ? k : key;
      }
      if (lane < 16) {
        if (cnt) {
          atomicAdd(&scnt[col], cnt);
          if (gc && one_group && (unsigned)g0 < (unsigned)n_gc) atomicAdd(&gc[(size_t)oi * n_gc + g0], (unsigned)cnt);
        }
        if (key) atomicMax(&sbest[col], key);
      }
    }
    __syncthreads();                                            // srow_a and sgrp are rewritten by the next strip
  }
  __syncthreads();
  if (tid < TN && ot * TN + tid < n_obj) {
    if (scnt[tid]) atomicAdd(&out_count[ot * TN + tid], scnt[tid]);
    if (sbest[tid]) atomicMax(&best[ot * TN + tid], sbest[tid]);
  }
}

__global__ __launch_bounds__(1024) void sightings_finish_kernel(const unsigned long long* __restrict__ best, int n_obj, int* __restrict__ out_row,
                                                                float* __restrict__ out_score) {
  const int i = threadIdx.x;
  if (i >= n_obj) return;
  const unsigned long long k = best[i];                         // 0: no pair (no float but a NaN has the ordered value 0)
  if (out_row) out_row[i] = k ? (int)(~(unsigned)k) : -1;
  if (out_score) out_score[i] = k ? sight_unordered((unsigned)(k >> 32)) : -__builtin_inff();
}

template <int STORAGE, int NT>
void launch_tiles(const char* emb, long size, int dim, const long long* sel, const int* m, const long long* obj, int n_obj, float same_at, int skip_self,
                  const int* grp, int n_gc, int* out_count, unsigned long long* best, unsigned* gc, hipStream_t stream) {
  constexpr int TN = 16 * NT;
  const size_t lds = sight_lds(NT);
  if (lds > 65536) ensure_max_lds(sightings_kernel<STORAGE, NT>, lds);
  const int n_ot = (n_obj + TN - 1) / TN;
  const long strips = (size - 1) / kSightStrip + 1;             // at most: every row competes
  const long slots = (long)cu_count() * (long)std::max<size_t>(1, std::min<size_t>(4, (size_t)160 * 1024 / (lds + 4096)));
  const long per_ot = std::max<long>(1, std::min<long>(strips, slots / n_ot));
  hipLaunchKernelGGL((sightings_kernel<STORAGE, NT>), dim3((unsigned)(per_ot * n_ot)), dim3(256), lds, stream, emb, size, dim, sel, m, obj, n_obj, n_ot,
                     same_at, skip_self, grp, n_gc, out_count, best, gc);
}

template <int STORAGE>
void launch_storage(const char* emb, long size, int dim, const long long* sel, const int* m, const long long* obj, int n_obj, float same_at, int skip_self,
                    const int* grp, int n_gc, int* out_count, unsigned long long* best, unsigned* gc, hipStream_t stream) {
  if (n_obj <= 16) launch_tiles<STORAGE, 1>(emb, size, dim, sel, m, obj, n_obj, same_at, skip_self, grp, n_gc, out_count, best, gc, stream);
  else if (n_obj <= 64) launch_tiles<STORAGE, 4>(emb, size, dim, sel, m, obj, n_obj, same_at, skip_self, grp, n_gc, out_count, best, gc, stream);
  else launch_tiles<STORAGE, 8>(emb, size, dim, sel, m, obj, n_obj, same_at, skip_self, grp, n_gc, out_count, best, gc, stream);
}

}  // namespace

void launch_sightings(const void* emb, long size, int dim, int storage, const long long* sel, const int* m, const long long* obj, int n_obj, float same_at,
                      int skip_self, const int* grp, int n_gc, int* out_count, unsigned long long* best, unsigned* gc, int* out_best_row,
                      float* out_best_score, hipStream_t stream) {
  const char* e = static_cast<const char*>(emb);
  if (size > 0) {
    if (storage == F32) launch_storage<F32>(e, size, dim, sel, m, obj, n_obj, same_at, skip_self, grp, n_gc, out_count, best, gc, stream);
    else if (storage == BF16) launch_storage<BF16>(e, size, dim, sel, m, obj, n_obj, same_at, skip_self, grp, n_gc, out_count, best, gc, stream);
    else launch_storage<CC_INDEX_I8>(e, size, dim, sel, m, obj, n_obj, same_at, skip_self, grp, n_gc, out_count, best, gc, stream);
    CC_HIP(hipGetLastError());
  }
  if (out_best_row || out_best_score) {
    hipLaunchKernelGGL(sightings_finish_kernel, dim3(1), dim3(1024), 0, stream, best, n_obj, out_best_row, out_best_score);
    CC_HIP(hipGetLastError());
  }
}

}  // namespace cc
