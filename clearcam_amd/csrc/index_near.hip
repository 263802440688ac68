// Together (cc_index_rank_near / cc_index_timeline_near): rank the rows of question A that have a partner - an answer of question B -
// nearby in time in the same folder.  The C entry points stand with the handle in index.hip, where rank() / timeline() take the join as a
// third kind of FoldQuery; this file holds the three kernels that are new.  What runs around them is the ranking's own: one scoring call
// for both vectors, the selection launches of cc_index_rank_where on B's score row (ungrouped, cut at cut_b, rows with a ts only), which
// leave the partner list on the device in ranking order, and behind the fold the launches of cc_index_rank_where / cc_index_timeline for
// ONE query.
//
//   near_pack_kernel    the list as the emit kernel left it (row, score; -1 behind the last entry) -> structure of arrays: the group, the
//                       ts and the track slot of every entry beside its row and its score, 20 bytes an entry, 320 KB at the cap.
//   near_fold_kernel    one thread per row r of the index.  The block stages the list kNearChunk entries at a time into LDS (four
//                       columns, 16 KB) and every thread walks the chunk IN LIST ORDER and stops at the first entry that qualifies for
//                       its row: another row, the same group, |ts - ts[r]| <= within in 64 bits, not the row's own track.  The list is in
//                       descending order of B's score, so the first qualifying entry is the best-scoring partner: nothing is folded, no
//                       atomics, no order to depend on.  All lanes of a wave read the same LDS words (a broadcast): four entries' groups and
//                       four entries' ts per step.  The common case - no
//                       entry of the four qualifies by group and time - costs per entry one compare of the group, one v_sad_u32
//                       and one compare of the time, and a wave none of whose rows shares a folder with the four leaves after the first.  The difference of two int32 lies within +-(2^32 - 1), so its absolute
//                       value fits an unsigned 32-bit word exactly: with both ts moved to unsigned order (the sign bit flipped),
//                       |a - b| = v_sad_u32(a, b, 0) never wraps and equals the 64-bit rule of the contract (a first version took the
//                       differences in 64 bits inside a branch per entry: 0.7 ms more per call at 4096 entries on 1 M rows whose
//                       folders are interleaved, docs/measurement.md, "Together").  Row and slot are read only for an
//                       entry that passed both.  A block leaves the list as
//                       soon as none of its rows is still looking.  A thread writes v over S[0][r] in place (CC_NEAR_VALUE_MIN: the smaller
//                       of Sa[r] and the partner's Sb in key order), dead[r] and pos[r], the partner's place in the list, of its own row
//                       only.  A row that cannot be an answer skips the walk and is written dead: its v is never observed.
//   near_gather_kernel  behind the last emit: partner / partner_score of the `count` answers from pos[] and the list.
#include "kernels.h"
#include "../../include/clearcam_hip.h"

namespace cc {

namespace {

static_assert(CC_NEAR_MAX_PARTNERS == kNearMaxPartners, "the header and kernels.h disagree");
static_assert(CC_ROW_NO_TS == kRowNoTs, "the header and kernels.h disagree");

constexpr int kNearChunk = 1024;                                // list entries staged per step; kNearMaxPartners is a multiple

__device__ __forceinline__ unsigned near_ordered(float f) {     // monotone float -> uint, the ranking keys' order (index.hip)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// |a - b| of two unsigned words, exact (it never exceeds 2^32 - 1): one v_sad_u32 where max - min would be three instructions
__device__ __forceinline__ unsigned near_absdiff(unsigned a, unsigned b) {
  unsigned d;
  asm("v_sad_u32 %0, %1, %2, 0" : "=v"(d) : "v"(a), "v"(b));
  return d;
}

__global__ __launch_bounds__(256) void near_pack_kernel(const NearList L, int cap, long n, const int* __restrict__ grp, const int* __restrict__ ts,
                                                        const int* __restrict__ trk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const int r = L.row[i];
  const bool ok = r >= 0 && (long)r < n;                          // -1: behind the last entry
  L.grp[i] = ok ? grp[r] : 0;
  L.ts[i] = ok ? ts[r] : kRowNoTs;
  L.trk[i] = ok ? trk[r] : -1;
}

// n_list: the number of rows the list would hold without the cap (the total of the selection's key pass); the list holds min(that, cap).
__global__ __launch_bounds__(256) void near_fold_kernel(float* __restrict__ S, long n, const int* __restrict__ grp, const int* __restrict__ trk,
                                                        const int* __restrict__ ts, const unsigned char* __restrict__ allowed, int n_allowed,
                                                        const RowWhere where_a, float min_score, int skip_cut, const NearList L,
                                                        const unsigned* __restrict__ n_list, int cap, int within, int value,
                                                        unsigned char* __restrict__ dead, int* __restrict__ pos) {
  __shared__ __attribute__((aligned(16))) int s_grp[kNearChunk];
  __shared__ __attribute__((aligned(16))) unsigned s_ts[kNearChunk];   // in unsigned order: the sign bit flipped
  __shared__ int s_row[kNearChunk], s_trk[kNearChunk];
  const int tid = threadIdx.x;
  const long r = (long)blockIdx.x * 256 + tid;
  const int len = (int)min(*n_list, (unsigned)cap);
  bool look = false;
  int g = 0, k = -1; unsigned t = 0u; float sa = 0.f;
  if (r < n) {
    sa = S[r];
    const int tr = ts[r];
    // allowed / where_a: the ranking rejects the row whatever it is worth; no ts: no partner by the rule; below the cut (skip_cut: a
    // ranking without track reduction, where v <= Sa is cut whatever the partner): never observed either
    look = tr != kRowNoTs && row_passes(grp, allowed, n_allowed, where_a, r) && !(skip_cut && sa < min_score);
    if (look) { g = grp[r]; k = trk[r]; t = (unsigned)tr ^ 0x80000000u; }
  }
  const unsigned w = (unsigned)within;                              // within >= 0 (checked on the host)
  int found = -1;
  for (int c0 = 0; c0 < len; c0 += kNearChunk) {
    if (!__syncthreads_or(look && found < 0)) break;               // also the barrier between the readers of a chunk and the next staging
    const int m = min(kNearChunk, len - c0);
    for (int i = tid; i < m; i += 256) {
      s_grp[i] = L.grp[c0 + i]; s_ts[i] = (unsigned)L.ts[c0 + i] ^ 0x80000000u; s_row[i] = L.row[c0 + i]; s_trk[i] = L.trk[c0 + i];
    }
    __syncthreads();
    if (look && found < 0) {
      const int4* g4p = reinterpret_cast<const int4*>(s_grp);
      const uint4* t4p = reinterpret_cast<const uint4*>(s_ts);
      const int nq = (m + 3) >> 2;                                 // the last four may end in stale entries: p < m is tested below
      for (int i = 0; i < nq; ++i) {
        const int4 g4 = g4p[i]; const uint4 t4 = t4p[i];           // both loads in flight; the other waves of the SIMD hide their latency
        const bool e0 = g4.x == g, e1 = g4.y == g, e2 = g4.z == g, e3 = g4.w == g;
        if (!(e0 | e1 | e2 | e3)) continue;                        // rows stand folder by folder in ingest order: most waves leave here
        // no short circuit: four differences and eight compares without a branch between them
        const bool n0 = near_absdiff(t4.x, t) <= w, n1 = near_absdiff(t4.y, t) <= w, n2 = near_absdiff(t4.z, t) <= w, n3 = near_absdiff(t4.w, t) <= w;
        const bool h[4] = {bool(e0 & n0), bool(e1 & n1), bool(e2 & n2), bool(e3 & n3)};
        if (!(h[0] | h[1] | h[2] | h[3])) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = 4 * i + j;
          if (found >= 0 || !h[j] || p >= m) continue;
          if ((long)s_row[p] == r) continue;
          if (k >= 0 && s_trk[p] == k) continue;                   // the same track of the same folder: the row's own object
          found = c0 + p;
        }
        if (found >= 0) break;
      }
    }
  }
  if (r < n) {
    dead[r] = found >= 0 ? 0 : 1;
    pos[r] = found;
    if (found >= 0 && value == CC_NEAR_VALUE_MIN) {
      const float sb = L.score[found];
      if (near_ordered(sb) < near_ordered(sa)) S[r] = sb;
    }
  }
}

// idx may be pinned host memory (the zero-copy route), as for which_gather_kernel; the tests keep every load inside its column.
__global__ __launch_bounds__(256) void near_gather_kernel(const int* __restrict__ idx, const int* __restrict__ pos, const NearList L, long n, size_t cnt, int cap,
                                                          int* __restrict__ partner, float* __restrict__ partner_score) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (size_t)gridDim.x * 256) {
    const int r = idx[i];
    const int p = (r >= 0 && (long)r < n) ? pos[r] : -1;
    const bool ok = p >= 0 && p < cap;
    if (partner) partner[i] = ok ? L.row[p] : -1;
    if (partner_score) partner_score[i] = ok ? L.score[p] : -INFINITY;
  }
}

}  // namespace

size_t near_list_bytes() { return (size_t)kNearMaxPartners * 5 * 4; }

NearList near_list(void* base) {
  NearList L;
  L.row = reinterpret_cast<int*>(base); L.grp = L.row + kNearMaxPartners; L.ts = L.grp + kNearMaxPartners; L.trk = L.ts + kNearMaxPartners;
  L.score = reinterpret_cast<float*>(L.trk + kNearMaxPartners);
  return L;
}

void launch_near_pack(const NearList& L, int cap, long n, const int* grp, const int* ts, const int* trk, hipStream_t stream) {
  hipLaunchKernelGGL(near_pack_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, stream, L, cap, n, grp, ts, trk);
  CC_HIP(hipGetLastError());
}

void launch_near_fold(float* S, long n, const int* grp, const int* trk, const int* ts, const unsigned char* allowed, int n_allowed, const RowWhere& where_a,
                      float min_score, int skip_cut, const NearList& L, const unsigned* n_list, int cap, int within, int value, unsigned char* dead, int* pos,
                      hipStream_t stream) {
  hipLaunchKernelGGL(near_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, S, n, grp, trk, ts, allowed, n_allowed, where_a, min_score,
                     skip_cut, L, n_list, cap, within, value, dead, pos);
  CC_HIP(hipGetLastError());
}

void launch_near_gather(const int* idx, const int* pos, const NearList& L, long n, size_t cnt, int cap, int* partner, float* partner_score, hipStream_t stream) {
  hipLaunchKernelGGL(near_gather_kernel, dim3((unsigned)std::min<size_t>((cnt + 255) / 256, 4096)), dim3(256), 0, stream, idx, pos, L, n, cnt, cap, partner,
                     partner_score);
  CC_HIP(hipGetLastError());
}

}  // namespace cc
