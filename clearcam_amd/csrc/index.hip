// Device-resident embedding index: brute-force cosine scan + top-k.
//
// Stands behind the scoring loop of ObjectFinder.search (models/objects.py:365-376), where the reference
// evaluates `(img_embedding @ text_embedding.T).item()` once per stored crop in a Python loop.  Here the
// (N, dim) float32 matrix lives in HBM and one query costs one streaming pass over it (HBM-bound:
// N*dim*4 bytes), followed by a two-stage radix-select top-k.  Scores are exact f32 dot products
// (sequential fma per lane + wave tree), so ranking ties break by row id exactly as a stable sort would.
//
// cc_index_search_tracks also does the reference's tail (:378-390: best crop per track id, id-less crops kept, stable
// sort) on the device.  Every row carries a track slot (-1: none).  Between the scan and the selection one pass over
// scores + slots reduces each track to ordered(score) << 32 | ~row with a 64-bit integer atomic maximum and finds each
// track's first allowed row with an atomic minimum; the selection then runs over one key per track (placed at that
// first row, so equal scores order by first appearance like a dict does) plus one per slot-less row.  Integer max / min
// do not depend on the arrival order: the answer is deterministic, ties included.
//
// cc_index_remove_rows / cc_index_remove_groups take rows out by stable compaction in place ("Removing rows"):
// keep flags -> per-granule counts -> one-block scan -> one mover launch per slab, ordered by the stream alone.
//
// Every row also carries ts (seconds into the day's recording) and cls (the detector's class), the other two facts of a crop's name.
// cc_index_rank_where tests them where the group filter is tested (row_passes, in the track reduction and in the key pass), and
// cc_index_timeline counts the answers of a ranking into bins of their ts (timeline_kernel) instead of selecting a window.
//
// cc_index_rank_like takes its queries from the matrix itself ("more like this stored crop / this whole track"): fetch_rows_kernel
// gathers and decodes them, terms_fold_kernel (every row a RANK term under MAX) folds their score vectors into one by the row-wise
// maximum and marks the excluded rows, which row_passes then keeps out of the ranking like rows the filter rejects (DESIGN.md
// section 4, "Query by stored rows").
//
// cc_index_rank_terms / cc_index_timeline_terms rank a compound question: up to 64 terms (vectors the caller brings and stored rows) are
// scored in one batch, terms_fold_kernel folds them by role (RANK through max / min / a weighted sum, REQUIRE and REJECT into the dead
// bytes) into one vector, and the same ranking of ONE query follows ("Compound search").
//
// cc_index_rank_near / cc_index_timeline_near rank the rows of one question that have an answer of a second question nearby in time:
// both are scored in one batch, the selection below leaves B's first answers on the device as the partner list, near_fold_kernel
// (index_near.hip) joins every row against it, and the same ranking of ONE query follows ("Together").
//
// cc_index_gram / cc_index_distinct, cc_index_digest and cc_index_sightings have their entry points here and their kernels in
// index_distinct.hip, index_digest.hip and index_sightings.hip.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>
#include "kernels.h"
#include "../../include/clearcam_hip.h"

using namespace cc;

struct cc_index {
  int dim = 0, device = 0; int64_t capacity = 0, n = 0;
  int storage = F32;                              // F32: exact f32 dot products; BF16: rows rounded to bf16 (half the scan bytes, scores within ~1e-3);
                                                  // CC_INDEX_I8: int8 codes + one f32 scale per 32 elements (dim * 9 / 8 bytes a row)
  float* emb = nullptr;                           // (capacity, row_bytes()) rows in the storage type
  int* grp = nullptr;                             // (capacity) group id of each row (camera/day bucket chosen by the caller); 0 by default
  int* trk = nullptr;                             // (capacity) track slot of each row: dense per distinct track id, -1 = a crop without one (the default)
  int* ts = nullptr;                              // (capacity) seconds into the day's recording of each row; CC_ROW_NO_TS = none (the default)
  int* cls = nullptr;                             // (capacity) detector class of each row in [0, 255]; -1 = none (the default)
  int* attr_tmp = nullptr; size_t attr_tmp_cap = 0;   // removal: the ts and cls columns as they were, the source of the scatter
  int n_slots = 0;                                // highest slot + 1
  unsigned long long* best = nullptr; size_t best_cap = 0;   // (Q, n_slots) per-track maximum of the current track search: ordered(score) << 32 | ~row
  unsigned* first = nullptr; size_t first_cap = 0;           // (n_slots) first allowed row of each track in the current track search
  unsigned* key_hi = nullptr; size_t key_hi_cap = 0;         // (Q, n) high words of the selection keys of the current track search
  unsigned char* allowed = nullptr; int allowed_cap = 0;   // per-group filter of the current search (device copy)
  size_t row_bytes() const { return storage == CC_INDEX_I8 ? (size_t)dim + dim / 8 : (size_t)dim * (storage == F32 ? 4 : 2); }
  hipStream_t stream = nullptr;
  float* q_dev = nullptr; int q_cap = 0;
  uint16_t* q16 = nullptr; int q16_cap = 0;     // bf16 copy of the queries (bf16 index, many queries: one MFMA GEMM pass)
  void* q_planes = nullptr; size_t q_planes_cap = 0;   // three bf16 planes of the queries (int8 index, a batch on the MFMA kernel: index_i8_mfma.hip)
  int last_path = 0;                            // which kernel wrote `scores` last (cc_index_last_path): 0 scan passes, 1 the f32 / bf16 MFMA GEMM, 2 the int8 MFMA kernel
  float* scores = nullptr; size_t scores_cap = 0;
  unsigned long long* cand = nullptr; size_t cand_cap = 0;
  int* idx_dev = nullptr; float* sc_dev = nullptr; size_t out_cap = 0;
  char* pin = nullptr; size_t pin_cap = 0;      // pinned, device-visible host staging: queries in, small results out
  // removal (cc_index_remove_*): scratch of the current call, kept for the next one
  unsigned char* keep = nullptr; size_t keep_cap = 0;          // (n) in: the caller's drop bytes (row removal); out: 1 = the row survives
  unsigned char* drop_grp = nullptr; size_t drop_grp_cap = 0;  // per-group drop table (group removal)
  unsigned* gcnt = nullptr; size_t gcnt_cap = 0;               // survivors per granule of kGran rows
  unsigned long long* goff = nullptr; size_t goff_cap = 0;     // survivors before each granule, and the total behind the last one
  char* bounce = nullptr; size_t bounce_cap = 0;               // one slab of survivors: rows, then their groups, then their slots
  char* rank_ws = nullptr; size_t rank_ws_cap = 0;             // cc_index_rank: per query and select the state, a 256-bin table and a window counter; per query the total
  // query by stored rows (cc_index_fetch_rows / cc_index_rank_like)
  unsigned char* dead = nullptr; size_t dead_cap = 0;          // (n) one byte per row of the current cc_index_rank_like / cc_index_rank_terms: non-zero = dead, does not compete
  long long* rows_pin = nullptr; size_t rows_pin_cap = 0;      // pinned, device-visible: the row numbers of a gather of more than CC_LIKE_MAX_ROWS rows, read by fetch_rows_kernel
  hipEvent_t rows_ev = nullptr;                                // recorded behind that gather: rows_pin is rewritten only after it
  std::vector<int32_t> grp_host, trk_host;                     // the grp / trk columns on the host (n each): CC_LIKE_EXCLUDE_TRACK is checked without a device round trip
  // compound search (cc_index_rank_terms): touched by no other call
  unsigned char* which_row = nullptr; size_t which_row_cap = 0;   // (n) one byte per row: the RANK term that made the row's value, written by terms_fold_kernel
  int* which_dev = nullptr; size_t which_dev_cap = 0;             // (count) a host caller's `which` on the device, when the result is too large for the pinned block
  // together (cc_index_rank_near / cc_index_timeline_near, kernels in index_near.hip): touched by no other call
  char* near_ws = nullptr; size_t near_ws_cap = 0;             // the partner list (near_list), then the selects, bin tables and window counters of its selection, then its total
  int* near_pos = nullptr; size_t near_pos_cap = 0;            // (n) the place of each row's partner in the list, -1 = none, written by near_fold_kernel
  int* near_dev = nullptr; size_t near_dev_cap = 0;            // (2, count) a host caller's partner / partner_score on the device, when the result is too large for the pinned block
  // distinct ranking (cc_index_gram / cc_index_distinct, kernels in index_distinct.hip)
  char* dist_ws = nullptr; size_t dist_ws_cap = 0;             // per list: squeezed rows, their places, the bit matrix, the counts (distinct_ws)
  char* dist_io = nullptr; size_t dist_io_cap = 0;             // a host caller's lists and answers, or its Gram matrix, on the device
  // day digest (cc_index_digest, kernels in index_digest.hip)
  char* digest_ws = nullptr; size_t digest_ws_cap = 0;         // the competing rows, two bit matrices of a piece, the leader tables (digest_ws)
  char* digest_io = nullptr; size_t digest_io_cap = 0;         // a host caller's window and owner column on the device
  int* digest_pin = nullptr;                                   // pinned: the number of competing rows, the call's one readback
  // seen before (cc_index_sightings, kernels in index_sightings.hip); the selection lives in digest_ws
  char* sight_ws = nullptr; size_t sight_ws_cap = 0;           // the objects' row numbers (1024 int64), then their best keys (1024 uint64)
  char* sight_io = nullptr; size_t sight_io_cap = 0;           // a host caller's four outputs on the device
};

namespace {

constexpr int kChunk = 16384;     // rows per stage-1 block
constexpr int kMaxK = 1024;
// scan_kernel and scan_bf16_kernel keep the queries of a pass in LDS, dim floats each.  A pass takes as many as the 160 KB of a gfx950
// CU hold, at most 8: 8 up to dim 5120 (768 and 512 among them), 7 at 5376, 5 at 8192, 2 at 16384, 1 from 20736 to 40960, the
// widest bf16 row cc_index_create_ex accepts.  Per query the order of the additions does not depend on the width of the pass.
constexpr int kScanLdsFloats = 40960;
inline int scan_pass_width(int dim) { return std::max(1, std::min(8, kScanLdsFloats / dim)); }

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// scores[q][row] = <emb[row], query[q]>; one wave per row (grid-stride), up to 4 queries per pass.
template <int QB>
__global__ __launch_bounds__(256) void scores_kernel(const float* __restrict__ emb, const float* __restrict__ q, float* __restrict__ out,
                                                      long n, int dim, int nq) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long row = wave; row < n; row += nwaves) {
    const float* e = emb + row * dim;
    float acc[QB];
#pragma unroll
    for (int c = 0; c < QB; ++c) acc[c] = 0.f;
    for (int j = lane * 4; j < dim; j += 256) {
      const float4 v = *reinterpret_cast<const float4*>(e + j);
#pragma unroll
      for (int c = 0; c < QB; ++c) {
        if (c < nq) {
          const float4 w = *reinterpret_cast<const float4*>(q + (long)c * dim + j);
          acc[c] = fmaf(v.x, w.x, acc[c]); acc[c] = fmaf(v.y, w.y, acc[c]); acc[c] = fmaf(v.z, w.z, acc[c]); acc[c] = fmaf(v.w, w.w, acc[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < QB; ++c) {
      const float s = wsum(acc[c]);
      if (lane == 0 && c < nq) out[(long)c * n + row] = s;
    }
  }
}

// The same scores with more memory parallelism (dim % 256 == 0, e.g. 768 / 512 / 1024): a row is covered by 16 lanes,
// so one wave reads four rows per load instruction and keeps four independent 16-byte loads per lane in flight (16 KB
// per wave); the queries sit in LDS; the per-row reduction is 4 shuffle steps instead of 6.  Each lane accumulates its
// 16-byte slots in ascending order with fma, then the 16 partial sums are added as a butterfly: a fixed order, so
// scores are deterministic and ties still break by row id.
template <int QB>
__global__ __launch_bounds__(256) void scan_kernel(const float* __restrict__ emb, const float* __restrict__ q, float* __restrict__ out,
                                                    long n, int dim) {
  extern __shared__ float4 qs[];                                  // QB x dim/4
  const int nchunk = dim >> 2;
  for (int i = threadIdx.x; i < QB * nchunk; i += 256) qs[i] = reinterpret_cast<const float4*>(q)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const int steps = dim >> 6;                                     // 16 lanes x 4 floats per step; a multiple of 4
  for (long r0 = wave * 4; r0 < n; r0 += nwaves * 4) {
    const long row = r0 + grp;
    const bool live = row < n;
    const float4* e = reinterpret_cast<const float4*>(emb + (live ? row : n - 1) * dim) + sub;
    float acc[QB];
#pragma unroll
    for (int c = 0; c < QB; ++c) acc[c] = 0.f;
    for (int t0 = 0; t0 < steps; t0 += 4) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = e[(t0 + u) * 16];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < QB; ++c) {
          const float4 w = qs[c * nchunk + (t0 + u) * 16 + sub];
          acc[c] = fmaf(v[u].x, w.x, acc[c]); acc[c] = fmaf(v[u].y, w.y, acc[c]); acc[c] = fmaf(v[u].z, w.z, acc[c]); acc[c] = fmaf(v[u].w, w.w, acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < QB; ++c) {
      float sum = acc[c];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      if (sub == 0 && live) out[(long)c * n + row] = sum;
    }
  }
}

template <int QB> void launch_scan(cc_index* h, const float* q, float* out, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>((h->n + 15) / 16, 256 * 8);
  const size_t lds = (size_t)QB * h->dim * 4;                     // <= kScanLdsFloats * 4: compute_scores cuts the passes by scan_pass_width
  if (lds > 65536) ensure_max_lds(scan_kernel<QB>, (size_t)kScanLdsFloats * 4);
  hipLaunchKernelGGL(scan_kernel<QB>, dim3(blocks), dim3(256), lds, s, h->emb, q, out, (long)h->n, h->dim);
}

// bf16-stored rows: 16 lanes x 8 halfs per step, two independent groups of four rows per wave iteration (four 16-byte loads per
// lane in flight, like the f32 kernel); f32 queries from LDS, f32 fma accumulation in a fixed order.  dim % 256 == 0.
template <int QB>
__global__ __launch_bounds__(256) void scan_bf16_kernel(const uint16_t* __restrict__ emb, const float* __restrict__ q, float* __restrict__ out,
                                                         long n, int dim) {
  extern __shared__ float4 qs[];
  const int nchunk = dim >> 2;
  for (int i = threadIdx.x; i < QB * nchunk; i += 256) qs[i] = reinterpret_cast<const float4*>(q)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const int steps = dim >> 7;                                     // 16 lanes x 8 halfs per step; even
  for (long r0 = wave * 8; r0 < n; r0 += nwaves * 8) {
    const long rowa = r0 + grp, rowb = r0 + 4 + grp;
    const uint4* ea = reinterpret_cast<const uint4*>(emb + (rowa < n ? rowa : n - 1) * dim) + sub;
    const uint4* eb = reinterpret_cast<const uint4*>(emb + (rowb < n ? rowb : n - 1) * dim) + sub;
    float acca[QB], accb[QB];
#pragma unroll
    for (int c = 0; c < QB; ++c) { acca[c] = 0.f; accb[c] = 0.f; }
    for (int t0 = 0; t0 < steps; t0 += 2) {
      uint4 va[2], vb[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) { va[u] = ea[(t0 + u) * 16]; vb[u] = eb[(t0 + u) * 16]; }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const unsigned wa[4] = {va[u].x, va[u].y, va[u].z, va[u].w}, wb[4] = {vb[u].x, vb[u].y, vb[u].z, vb[u].w};
#pragma unroll
        for (int c = 0; c < QB; ++c) {
          const float4 q0 = qs[c * nchunk + ((t0 + u) * 16 + sub) * 2], q1 = qs[c * nchunk + ((t0 + u) * 16 + sub) * 2 + 1];
          const float qq[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acca[c] = fmaf(__uint_as_float(wa[e] << 16), qq[2 * e], acca[c]); acca[c] = fmaf(__uint_as_float(wa[e] & 0xffff0000u), qq[2 * e + 1], acca[c]);
            accb[c] = fmaf(__uint_as_float(wb[e] << 16), qq[2 * e], accb[c]); accb[c] = fmaf(__uint_as_float(wb[e] & 0xffff0000u), qq[2 * e + 1], accb[c]);
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < QB; ++c) {
      float sa = acca[c], sb = accb[c];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
      if (sub == 0 && rowa < n) out[(long)c * n + rowa] = sa;
      if (sub == 0 && rowb < n) out[(long)c * n + rowb] = sb;
    }
  }
}

template <int QB> void launch_scan_bf16(cc_index* h, const float* q, float* out, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>((h->n + 31) / 32, 256 * 8);
  const size_t lds = (size_t)QB * h->dim * 4;
  if (lds > 65536) ensure_max_lds(scan_bf16_kernel<QB>, (size_t)kScanLdsFloats * 4);
  hipLaunchKernelGGL(scan_bf16_kernel<QB>, dim3(blocks), dim3(256), lds, s, reinterpret_cast<const uint16_t*>(h->emb), q, out, (long)h->n, h->dim);
}

// f32 rows -> bf16 rows (round to nearest even), for cc_index_add on a bf16-stored index
__global__ void to_bf16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = f32_to_bf16_bits(in[i]);
}

// int8-stored rows (CC_INDEX_I8): dim codes, then dim / 32 f32 scales, one per group of 32 consecutive elements (row_bytes = dim + dim / 8,
// the rule is in include/clearcam_hip.h).  16 lanes x 16 codes per step of 256; a lane's 16 codes lie inside one group: 16 converts,
// 16 fma into a group partial per query, then one fma by the group's scale from the row's trailer.  A 16-byte load carries four times
// the elements of an f32 one, so a wave iteration takes FOUR groups of four rows (16 rows): four independent 16-byte loads per lane
// in flight like scan_kernel, and every query value read from LDS serves four rows.  Per query the order of the additions is fixed
// (steps ascending, codes ascending, then the 16-lane butterfly) and does not depend on QB: a batch scores the same however it is split.
constexpr int kI8Pass = 8;                                        // queries per pass over int8 rows (compute_scores): the fastest of 1..8 measured
constexpr int kI8Rows = 4;                                        // groups of four rows per wave iteration
// The smallest batch that leaves the scan passes for the MFMA kernel (index_i8_mfma.hip) by default.  Never below 18: a batch of up to
// 17 queries is promised bit-equal to single queries.  The sweep behind it (docs/measurement.md, "int8 rows": 1 M x 768, search(q, 100),
// p50 in ms, forced scan / MFMA kernel): Q = 8 0.43 / 0.35, 16 0.80 / 0.38, 24 1.18 / 0.48, 32 1.56 / 0.52, 48 2.33 / 0.65, 64 3.10 / 0.82,
// 128 6.18 / 1.54, 256 12.3 / 3.05: the MFMA kernel is never the slower one, so the threshold is the lowest the contract allows.
constexpr int kI8MfmaFrom = 18;

template <int QB>
__global__ __launch_bounds__(256) void scan_i8_kernel(const char* __restrict__ emb, const float* __restrict__ q, float* __restrict__ out,
                                                       long n, int dim) {
  extern __shared__ float4 qs[];                                  // QB x dim/4
  const int nchunk = dim >> 2;
  for (int i = threadIdx.x; i < QB * nchunk; i += 256) qs[i] = reinterpret_cast<const float4*>(q)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const int steps = dim >> 8;                                     // 16 lanes x 16 codes per step
  const size_t rb = (size_t)dim + (dim >> 3);
  for (long r0 = wave * (4 * kI8Rows); r0 < n; r0 += nwaves * (4 * kI8Rows)) {
    const char* e[kI8Rows];
    float acc[kI8Rows][QB];
#pragma unroll
    for (int r = 0; r < kI8Rows; ++r) {
      const long row = r0 + r * 4 + grp;
      e[r] = emb + (size_t)(row < n ? row : n - 1) * rb;
#pragma unroll
      for (int c = 0; c < QB; ++c) acc[r][c] = 0.f;
    }
    for (int t = 0; t < steps; ++t) {
      uint4 v[kI8Rows]; float sc[kI8Rows];
#pragma unroll
      for (int r = 0; r < kI8Rows; ++r) {
        v[r] = reinterpret_cast<const uint4*>(e[r])[t * 16 + sub];
        sc[r] = reinterpret_cast<const float*>(e[r] + dim)[t * 8 + (sub >> 1)];
      }
      float f[kI8Rows][16];
#pragma unroll
      for (int r = 0; r < kI8Rows; ++r) {
        const unsigned w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
        for (int i = 0; i < 16; ++i) f[r][i] = i8_code(w[i >> 2], i & 3);
      }
#pragma unroll
      for (int c = 0; c < QB; ++c) {
        const float4* qc = qs + c * nchunk + (t * 16 + sub) * 4;
        const float4 q0 = qc[0], q1 = qc[1], q2 = qc[2], q3 = qc[3];
        const float qq[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
        for (int r = 0; r < kI8Rows; ++r) {
          float p = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) p = fmaf(f[r][i], qq[i], p);
          acc[r][c] = fmaf(p, sc[r], acc[r][c]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kI8Rows; ++r) {
      const long row = r0 + r * 4 + grp;
#pragma unroll
      for (int c = 0; c < QB; ++c) {
        float sum = acc[r][c];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (sub == 0 && row < n) out[(long)c * n + row] = sum;
      }
    }
  }
}

template <int QB> void launch_scan_i8(cc_index* h, const float* q, float* out, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>((h->n + 16 * kI8Rows - 1) / (16 * kI8Rows), 256 * 8);
  hipLaunchKernelGGL(scan_i8_kernel<QB>, dim3(blocks), dim3(256), (size_t)QB * h->dim * 4, s, reinterpret_cast<const char*>(h->emb), q, out, (long)h->n, h->dim);
}

// f32 rows -> int8 rows, for cc_index_add on an i8-stored index: one lane per element, a group of 32 elements is one half-wave.
// dim % 256 == 0, so every wave is whole and a group never straddles two rows.  The rule (include/clearcam_hip.h): a = max |x| of the
// group, s = a / 127 (correctly rounded f32 division), s zero or subnormal -> s = 0 and codes 0, else code = clamp(rint(x / s), +-127).
__global__ __launch_bounds__(256) void quantise_i8_kernel(const float* __restrict__ in, char* __restrict__ out, size_t cnt, int dim) {
  const size_t rb = (size_t)dim + (dim >> 3);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (size_t)gridDim.x * 256) {
    const float x = in[i];
    float a = fabsf(x);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
    float s = a / 127.0f;
    if (!(s >= 1.17549435e-38f)) s = 0.f;                         // zero or subnormal: nothing depends on the denormal mode
    const float c = s > 0.f ? fminf(fmaxf(rintf(x / s), -127.f), 127.f) : 0.f;
    const size_t row = i / (size_t)dim; const int j = (int)(i - row * dim);
    char* o = out + row * rb;
    o[j] = (char)(int)c;
    if ((j & 31) == 0) reinterpret_cast<float*>(o + dim)[j >> 5] = s;
  }
}

__device__ __forceinline__ unsigned ordered(float f) {          // monotone float -> uint
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// Block-wide exact top-K of `count` unique 64-bit keys (key(i) for i in [0,count)): MSB-first radix select of the
// K-th largest key, then collection of every key >= it into `sel` (unsorted; K entries, zero padded).
// Padding keys (zero) are never selected and stay out of the histogram: with fewer than K real keys no bucket reaches the
// wanted count, the prefix stays zero and every real key is collected.  Counting them cost more than everything else in a
// track search, where 19 of 20 keys are padding: thousands of LDS atomics of one block on the one address hist[0].
template <class KeyFn>
__device__ void block_topk(KeyFn key, long count, int K, unsigned long long* sel, unsigned* hist,
                           unsigned long long* s_prefix, int* s_k, unsigned* s_cnt) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < K; i += nt) sel[i] = 0ull;
  __shared__ int s_done;
  if (tid == 0) { *s_prefix = 0ull; *s_k = (int)(count < K ? count : K); *s_cnt = 0; s_done = 0; }
  __syncthreads();
  if (count <= 0) return;
  for (int byte = 7; byte >= 0; --byte) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned long long prefix = *s_prefix;
    const int sh = 8 * (byte + 1);
    for (long i = tid; i < count; i += nt) {
      const unsigned long long k = key(i);
      if (k != 0ull && (byte == 7 || (k >> sh) == (prefix >> sh))) atomicAdd(&hist[(unsigned)(k >> (8 * byte)) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {
      const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
      const unsigned s = h0 + h1 + h2 + h3;
      unsigned suf = s;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const unsigned t = __shfl_down(suf, off, 64); if (tid + off < 64) suf += t; }
      const unsigned above = suf - s, kk = (unsigned)*s_k;
      if (above < kk && kk <= suf) {
        unsigned cum = above; int v = 4 * tid + 3;
        const unsigned hh[4] = {h0, h1, h2, h3};
        for (int qd = 3; qd >= 0; --qd) { if (cum + hh[qd] >= kk) { v = 4 * tid + qd; break; } cum += hh[qd]; }
        *s_prefix = prefix | ((unsigned long long)v << (8 * byte));
        *s_k = (int)(kk - cum);
        // the whole bucket is wanted: every key at or above the prefix (lower bytes zero) is selected and the remaining
        // passes would only confirm it.  With distinct scores this fires after the four score bytes (row-id bytes skipped).
        if (hist[v] == kk - cum) s_done = 1;
      }
    }
    __syncthreads();
    if (s_done) break;
  }
  const unsigned long long thr = *s_prefix;
  for (long i = tid; i < count; i += nt) {
    const unsigned long long k = key(i);
    if (k >= thr && k != 0ull) { const unsigned pos = atomicAdd(s_cnt, 1u); if (pos < (unsigned)K) sel[pos] = k; }   // zero = padding / filtered-out row
  }
  __syncthreads();
}

// row_allowed, RowWhere and row_passes (the one rule by which a row competes) stand in kernels.h: the day digest selects by them too.

// Track search, pass 1: every allowed row with a track slot t raises best[q][t] to ordered(score) << 32 | ~row (a 64-bit integer
// maximum: the best score, and among equal scores the lowest row, whatever the arrival order) and lowers first[t] to its row id.
// Thousands of rows of ONE track (a parked car: one crop every 10 s all day) would send thousands of atomics to one address, so a
// block first reduces its contiguous kTrkRows rows in an LDS table keyed by slot & (kTrkTab - 1) and tagged with the slot; a row
// whose entry belongs to another slot goes to global memory directly.  One global atomic per distinct track per block is left.
// Measured on 1 M rows with one track owning 10 % of them (docs/measurement.md): 75 us, against 1.15 ms with one global atomic
// per row (the scan of the same search: 0.50 ms).
constexpr int kTrkRows = 2048, kTrkTab = 1024;

__global__ __launch_bounds__(256) void track_reduce_kernel(const float* __restrict__ scores, long n, int T, const int* __restrict__ trk,
                                                           const int* __restrict__ grp, const unsigned char* __restrict__ allowed, int n_allowed,
                                                           const RowWhere where, unsigned long long* __restrict__ best, unsigned* __restrict__ first) {
  __shared__ int tag[kTrkTab]; __shared__ unsigned long long val[kTrkTab]; __shared__ unsigned fst[kTrkTab];
  const int q = blockIdx.y, tid = threadIdx.x;
  const bool want_first = q == 0;                                // first[] depends on the filter only: the blocks of query 0 fill it
  for (int i = tid; i < kTrkTab; i += 256) { tag[i] = -1; val[i] = 0ull; fst[i] = 0xffffffffu; }
  __syncthreads();
  const long base = (long)blockIdx.x * kTrkRows, end = min(n, base + kTrkRows);
  const float* s = scores + (long)q * n;
  unsigned long long* b = best + (size_t)q * T;
  for (long r = base + tid; r < end; r += 256) {
    const int t = trk[r];
    if (t < 0 || t >= T || !row_passes(grp, allowed, n_allowed, where, r)) continue;
    const unsigned long long key = ((unsigned long long)ordered(s[r]) << 32) | (unsigned)(~(unsigned)r);
    const int h = t & (kTrkTab - 1);
    const int owner = atomicCAS(&tag[h], -1, t);
    if (owner == -1 || owner == t) {
      atomicMax(&val[h], key);
      if (want_first) atomicMin(&fst[h], (unsigned)r);
    } else {
      atomicMax(&b[t], key);
      if (want_first) atomicMin(&first[t], (unsigned)r);
    }
  }
  __syncthreads();
  for (int i = tid; i < kTrkTab; i += 256) {
    const int t = tag[i];
    if (t < 0) continue;
    atomicMax(&b[t], val[i]);
    if (want_first) atomicMin(&first[t], fst[i]);
  }
}

// stage 1: per (query, chunk of rows) top-K keys -> cand[q][chunk][K]
// `allowed` (one byte per group) filters rows by their group id: a row of a group that is not allowed contributes the padding key.
// TRACKS (pass 2 of the track search): a row without a slot carries its own score with ~(n + row) below it; the FIRST allowed row
// of a track carries the track's best score with its own ~row; every other row is padding.  So one key per track is in the
// running, tracks of equal score order by first appearance, and slot-less rows follow every track of the same score.
// The select evaluates a key up to nine times and a block has only 16 waves to hide latency with, so the chain of dependent loads
// behind a key (slot -> first[slot] -> best[q][slot]) is walked once: the block writes the high words of its chunk's keys to `hi`
// (its own rows of a (Q, n) scratch, 0 = padding) and the select then reads one coalesced word per key, like the plain search
// (1 M rows, 50 k tracks: 60 us against 104 us with the chain inside the key function; the plain stage 1: 26 us).
template <bool TRACKS>
__global__ __launch_bounds__(1024) void topk_stage1(const float* __restrict__ scores, long n, int K, unsigned long long* __restrict__ cand,
                                                    const int* __restrict__ grp, const unsigned char* __restrict__ allowed, int n_allowed,
                                                    const int* __restrict__ trk, const unsigned long long* __restrict__ best,
                                                    const unsigned* __restrict__ first, int T, unsigned* hi) {
  __shared__ unsigned hist[256]; __shared__ unsigned long long s_prefix; __shared__ int s_k; __shared__ unsigned s_cnt;
  __shared__ unsigned long long sel[kMaxK];
  const int chunk = blockIdx.x, q = blockIdx.y;
  const long base = (long)chunk * kChunk, count = min((long)kChunk, n - base);
  const float* s = scores + (long)q * n + base;
  unsigned* h = TRACKS ? hi + (long)q * n + base : nullptr;
  if (TRACKS) {
#pragma unroll 4
    for (long i = threadIdx.x; i < count; i += blockDim.x) {
      unsigned u = 0;
      if (row_allowed(grp, allowed, n_allowed, base + i)) {
        const int t = trk[base + i];
        if (t < 0) u = ordered(s[i]);
        else if (t < T && first[t] == (unsigned)(base + i)) u = (unsigned)(best[(size_t)q * T + t] >> 32);
      }
      h[i] = u;
    }
    __syncthreads();                                               // h[] is read back by other threads of this block only
  }
  auto key = [&](long i) -> unsigned long long {
    if (TRACKS) {
      const unsigned u = h[i];
      if (u == 0u) return 0ull;
      return ((unsigned long long)u << 32) | (unsigned)(~(unsigned)((trk[base + i] < 0 ? n : 0) + base + i));
    }
    if (!row_allowed(grp, allowed, n_allowed, base + i)) return 0ull;
    return ((unsigned long long)ordered(s[i]) << 32) | (unsigned)(~(unsigned)(base + i));
  };
  block_topk(key, count, K, sel, hist, &s_prefix, &s_k, &s_cnt);
  unsigned long long* o = cand + ((size_t)q * gridDim.x + chunk) * K;
  for (int i = threadIdx.x; i < K; i += blockDim.x) o[i] = sel[i];
}

// stage 2: merge candidates of one query, sort descending, emit (row id, score)
// TRACKS: the low word is ~position; a position >= n is a slot-less row (position - n), any other the first row of a track,
// whose answer is the row kept in best[q][slot].
template <bool TRACKS>
__global__ __launch_bounds__(1024) void topk_stage2(const unsigned long long* __restrict__ cand, long ncand, int K, int* __restrict__ idx, float* __restrict__ score,
                                                    long n, const int* __restrict__ trk, const unsigned long long* __restrict__ best, int T) {
  __shared__ unsigned hist[256]; __shared__ unsigned long long s_prefix; __shared__ int s_k; __shared__ unsigned s_cnt;
  __shared__ unsigned long long sel[kMaxK];
  const int q = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* c = cand + (size_t)q * ncand;
  auto key = [&](long i) { return c[i]; };      // zero keys (padding) sort last and never beat a real key
  for (int i = tid; i < kMaxK; i += blockDim.x) sel[i] = 0ull;
  __syncthreads();
  block_topk(key, ncand, K, sel, hist, &s_prefix, &s_k, &s_cnt);
  int P = 2;                                                     // the K selected keys sit in sel[0..K): sort the next power of two
  while (P < K) P <<= 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int ixj = tid ^ j;
      if (ixj > tid && ixj < P) {
        const unsigned long long x = sel[tid], y = sel[ixj];
        const bool desc = (tid & k) == 0;
        if (desc ? (x < y) : (x > y)) { sel[tid] = y; sel[ixj] = x; }
      }
      __syncthreads();
    }
  if (tid < K) {
    const unsigned long long k = sel[tid];
    if (k == 0ull) { idx[(size_t)q * K + tid] = -1; score[(size_t)q * K + tid] = -INFINITY; }
    else {
      unsigned row = ~(unsigned)(k & 0xffffffffull);
      if (TRACKS) row = row >= (unsigned)n ? row - (unsigned)n : ~(unsigned)(best[(size_t)q * T + trk[row]] & 0xffffffffull);
      idx[(size_t)q * K + tid] = (int)row; score[(size_t)q * K + tid] = unordered((unsigned)(k >> 32));
    }
  }
}

// ---- ranking: any window of the whole descending order (cc_index_rank) ---------------------------------------------------------
// The answers' keys are those of topk_stage1 / topk_stage2: ordered(score) << 32 | ~position, position = the row (a track: its
// first allowed row; without CC_RANK_TRACKS every allowed row is its own answer) or n + row for a slot-less row of a track search,
// 0 = padding, so keys are distinct and their descending order is the reference's dict order + stable sort.  Only the high words
// are stored (key_hi, as in the track search); the low word follows from the row number and its slot.
// A window of at most kMaxK answers is cut out by two boundary keys, the keys of rank `start` and of rank `end`: everything below
// the first and at or above the second.  A boundary is found by an MSB-first radix select over ALL keys, the multi-block form of
// block_topk: per key byte one launch in which every block counts its rows in an LDS histogram and adds the non-empty bins to a
// 256-bin table in global memory (integer atomics: the sums do not depend on the arrival order), and a one-wave launch that picks
// the digit.  Up to kRankSel boundaries - 16 consecutive windows - go through the same launches side by side (blockIdx.y).
// No block ever waits for another block: there is no flag to spin on, no ticket and no look-back anywhere in these kernels.
constexpr int kRankSel = 17;      // boundaries per batch of launches
constexpr int kRankRows = 4096;   // rows per block of the multi-block passes

struct RankSel { unsigned long long prefix; unsigned k, done; };   // a select: the key bytes fixed so far, the rank left inside them, finished

__device__ __forceinline__ unsigned long long rank_key(unsigned hi, long r, long n, const int* __restrict__ trk) {
  return ((unsigned long long)hi << 32) | (unsigned)(~(unsigned)((trk && trk[r] < 0 ? n : 0) + r));
}

// hi[q][row] = the high word of the row's key (0: filtered out, not the first row of its track, or below the cut), and
// total[q] += the number of keys.  TRACKS: behind track_reduce_kernel, like the first loop of topk_stage1<true>.
template <bool TRACKS>
__global__ __launch_bounds__(256) void rank_keys_kernel(const float* __restrict__ scores, long n, const int* __restrict__ grp,
                                                        const unsigned char* __restrict__ allowed, int n_allowed, const int* __restrict__ trk,
                                                        const unsigned long long* __restrict__ best, const unsigned* __restrict__ first, int T,
                                                        float min_score, const RowWhere where, unsigned* __restrict__ hi, unsigned* __restrict__ total) {
  __shared__ unsigned s_cnt[4];
  const int q = blockIdx.y, tid = threadIdx.x;
  const long base = (long)blockIdx.x * kRankRows, end = min(n, base + kRankRows);
  const float* s = scores + (long)q * n;
  unsigned* h = hi + (long)q * n;
  unsigned cnt = 0;
  for (long r = base + tid; r < end; r += 256) {
    unsigned u = 0;
    if (row_passes(grp, allowed, n_allowed, where, r)) {
      if (TRACKS) {
        const int t = trk[r];
        if (t < 0) u = ordered(s[r]);
        else if (t < T && first[t] == (unsigned)r) u = (unsigned)(best[(size_t)q * T + t] >> 32);
      } else u = ordered(s[r]);
      if (u != 0u && unordered(u) < min_score) u = 0u;             // the cut: score >= min_score stays (-inf: everything)
    }
    h[r] = u;
    cnt += u != 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) { const unsigned c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]; if (c) atomicAdd(&total[q], c); }
}

// The selects of one batch: boundary j is the key of rank min(r0 + j * kMaxK, r_last) (rank 0: nothing to find, the window is
// open at the top).  Clears the batch's bin tables and window counters.  One block per query.
__global__ __launch_bounds__(256) void rank_init_kernel(long r0, long r_last, RankSel* __restrict__ sel, unsigned* __restrict__ ghist, unsigned* __restrict__ wcnt) {
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < kRankSel * 256; i += 256) ghist[(size_t)q * kRankSel * 256 + i] = 0u;
  if (tid < kRankSel) {
    const long r = min(r0 + (long)tid * kMaxK, r_last);
    RankSel st; st.prefix = 0ull; st.k = (unsigned)r; st.done = r == 0;
    sel[q * kRankSel + tid] = st;
    wcnt[q * kRankSel + tid] = 0u;
  }
}

// One byte of select (blockIdx.y) of query (blockIdx.z): the digits of the keys that agree with the prefix above that byte.
__global__ __launch_bounds__(256) void rank_hist_kernel(const unsigned* __restrict__ hi, long n, const int* __restrict__ trk, int byte,
                                                        const RankSel* __restrict__ sel, unsigned* __restrict__ ghist) {
  __shared__ unsigned hist[256];
  const int j = blockIdx.y, q = blockIdx.z, tid = threadIdx.x;
  const RankSel st = sel[q * kRankSel + j];
  if (st.done) return;                                             // the same for every thread of every block of this select
  hist[tid] = 0u;
  __syncthreads();
  const long base = (long)blockIdx.x * kRankRows, end = min(n, base + kRankRows);
  const unsigned* h = hi + (long)q * n;
  const int sh = 8 * (byte + 1);
  for (long r = base + tid; r < end; r += 256) {
    const unsigned u = h[r];
    if (u == 0u) continue;
    const unsigned long long k = byte >= 4 ? (unsigned long long)u << 32 : rank_key(u, r, n, trk);   // the score bytes need no slot
    if (byte == 7 || (k >> sh) == (st.prefix >> sh)) atomicAdd(&hist[(unsigned)(k >> (8 * byte)) & 255u], 1u);
  }
  __syncthreads();
  const unsigned c = hist[tid];
  if (c) atomicAdd(&ghist[((size_t)q * kRankSel + j) * 256 + tid], c);
}

// One wave per select: walk the 256 bins from the top as block_topk does, fix the digit that holds the wanted rank, clear the bins.
// A select is finished when the whole bucket is wanted (every key at or above the prefix, lower bytes zero, then has a rank of at
// most the wanted one, and nothing else has: the prefix is as good a boundary as the key itself) or when fewer keys exist than
// the rank asks for (the prefix stays 0: every key lies at or above the boundary).
__global__ __launch_bounds__(64) void rank_pick_kernel(int byte, RankSel* __restrict__ sel, unsigned* __restrict__ ghist) {
  const int j = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  RankSel* st = sel + q * kRankSel + j;
  if (st->done) return;
  const unsigned kk = st->k;
  const unsigned long long prefix = st->prefix;
  unsigned* g = ghist + ((size_t)q * kRankSel + j) * 256 + 4 * tid;
  const unsigned hh[4] = {g[0], g[1], g[2], g[3]};
  g[0] = g[1] = g[2] = g[3] = 0u;
  const unsigned s = hh[0] + hh[1] + hh[2] + hh[3];
  unsigned suf = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const unsigned t = __shfl_down(suf, off, 64); if (tid + off < 64) suf += t; }
  const unsigned all = __shfl(suf, 0, 64), above = suf - s;
  if (all < kk) { if (tid == 0) st->done = 1u; return; }
  if (above < kk && kk <= suf) {
    unsigned cum = above; int v = 0;
    for (int qd = 3; qd >= 0; --qd) { if (cum + hh[qd] >= kk) { v = qd; break; } cum += hh[qd]; }
    st->prefix = prefix | ((unsigned long long)(4 * tid + v) << (8 * byte));
    st->k = kk - cum;
    if (hh[v] == kk - cum) st->done = 1u;
  }
}

// Every key below boundary 0 (open_top: no upper end) and at or above boundary S - 1 goes to the buffer of its window w, the one
// with boundary w > key >= boundary w + 1.  The place inside the buffer comes from an integer counter; the emit kernel sorts, so the
// result does not depend on it.  A window holds at most kMaxK keys by construction; the bound check only guards the buffer.
__global__ __launch_bounds__(256) void rank_collect_kernel(const unsigned* __restrict__ hi, long n, const int* __restrict__ trk, int S, int open_top,
                                                           const RankSel* __restrict__ sel, unsigned* __restrict__ wcnt, unsigned long long* __restrict__ wbuf) {
  __shared__ unsigned long long thr[kRankSel];
  const int q = blockIdx.y, tid = threadIdx.x;
  if (tid < S) thr[tid] = sel[q * kRankSel + tid].prefix;
  __syncthreads();
  const unsigned long long lo = thr[S - 1], top = thr[0];
  const long base = (long)blockIdx.x * kRankRows, end = min(n, base + kRankRows);
  const unsigned* h = hi + (long)q * n;
  for (long r = base + tid; r < end; r += 256) {
    const unsigned u = h[r];
    if (u == 0u) continue;
    const unsigned long long k = rank_key(u, r, n, trk);
    if (k < lo || (!open_top && k >= top)) continue;
    int w = 0;
    while (w < S - 2 && k < thr[w + 1]) ++w;
    const unsigned pos = atomicAdd(&wcnt[q * kRankSel + w], 1u);
    if (pos < (unsigned)kMaxK) wbuf[((size_t)q * kRankSel + w) * kMaxK + pos] = k;
  }
}

// One block per window: sort its keys descending with the bitonic network of topk_stage2 and emit (row, score) as it does, at
// answers out0 + window * kMaxK ... of the (Q, count) result; what lies past the last key is padding.
template <bool TRACKS>
__global__ __launch_bounds__(1024) void rank_emit_kernel(const unsigned long long* __restrict__ wbuf, const unsigned* __restrict__ wcnt, long out0, long count,
                                                         int* __restrict__ idx, float* __restrict__ score, long n, const int* __restrict__ trk,
                                                         const unsigned long long* __restrict__ best, int T) {
  __shared__ unsigned long long sel[kMaxK];
  const int w = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int c = (int)min(wcnt[q * kRankSel + w], (unsigned)kMaxK);
  sel[tid] = tid < c ? wbuf[((size_t)q * kRankSel + w) * kMaxK + tid] : 0ull;
  __syncthreads();
  int P = 2;
  while (P < c) P <<= 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int ixj = tid ^ j;
      if (ixj > tid && ixj < P) {
        const unsigned long long x = sel[tid], y = sel[ixj];
        const bool desc = (tid & k) == 0;
        if (desc ? (x < y) : (x > y)) { sel[tid] = y; sel[ixj] = x; }
      }
      __syncthreads();
    }
  const long o = out0 + (long)w * kMaxK + tid;
  if (o >= count) return;
  const unsigned long long k = sel[tid];
  int row = -1; float sc = -INFINITY;
  if (k != 0ull) {
    unsigned r = ~(unsigned)(k & 0xffffffffull);
    if (TRACKS) r = r >= (unsigned)n ? r - (unsigned)n : ~(unsigned)(best[(size_t)q * T + trk[r]] & 0xffffffffull);
    row = (int)r; sc = unordered((unsigned)(k >> 32));
  }
  idx[(size_t)q * count + o] = row; score[(size_t)q * count + o] = sc;
}

__global__ void rank_pad_kernel(int* __restrict__ idx, float* __restrict__ score, size_t cnt) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (size_t)gridDim.x * blockDim.x) { idx[i] = -1; score[i] = -INFINITY; }
}

// cc_index_timeline, behind rank_keys_kernel: counts[q][bin] += the answers of the block's kRankRows rows whose time falls into the
// bin.  hi[q][r] != 0 says that row r carries an answer; its time is the ts of the row the emit kernel would name (a track: the low
// word of best[q][slot], its best passing crop).  bin = (ts - t0) / bin_seconds in 64 bits (t0 = -2^31 + 1, ts = 2^31 - 1 differ by
// 2^32 - 2); a negative difference is below bin 0 and is dropped before the division, so truncation and floor agree.  The block
// counts in an LDS table of n_bins words (dynamic: 96 bytes for a day of hours, 16 KB at the limit of 4096, which still leaves ten
// blocks a CU) and adds its non-empty bins to global memory: integer sums, no block waits for another, no order to depend on.
template <bool TRACKS>
__global__ __launch_bounds__(256) void timeline_kernel(const unsigned* __restrict__ hi, long n, const int* __restrict__ trk,
                                                       const unsigned long long* __restrict__ best, int T, const int* __restrict__ ts,
                                                       long long t0, unsigned bin_seconds, int n_bins, unsigned* __restrict__ counts) {
  extern __shared__ unsigned bins[];
  const int q = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < n_bins; i += 256) bins[i] = 0u;
  __syncthreads();
  const long base = (long)blockIdx.x * kRankRows, end = min(n, base + kRankRows);
  const unsigned* h = hi + (long)q * n;
  for (long r = base + tid; r < end; r += 256) {
    if (h[r] == 0u) continue;
    long row = r;
    if (TRACKS) {
      const int t = trk[r];
      if (t >= 0) row = (long)(~(unsigned)(best[(size_t)q * T + t] & 0xffffffffull));
    }
    if (row < 0 || row >= n) continue;                             // cannot happen behind rank_keys_kernel; keeps the load inside the column
    const int t = ts[row];
    if (t == CC_ROW_NO_TS) continue;
    const long long d = (long long)t - t0;
    if (d < 0) continue;
    const unsigned long long b = (unsigned long long)d / bin_seconds;
    if (b < (unsigned long long)n_bins) atomicAdd(&bins[(unsigned)b], 1u);
  }
  __syncthreads();
  unsigned* c = counts + (size_t)q * n_bins;
  for (int i = tid; i < n_bins; i += 256) { const unsigned v = bins[i]; if (v) atomicAdd(&c[i], v); }
}

// ---- query by stored rows (cc_index_fetch_rows / cc_index_rank_like) ------------------------------------------------------------
// The queries are rows of the matrix: a gather decodes them to f32 where upload_queries would have copied them, the scoring routes
// of compute_scores run as for any batch, one pass of terms_fold_kernel (below) folds the (Q, n) score matrix into one vector (the
// row-wise maximum) and marks the excluded rows, and the ranking of ONE query follows unchanged.  Ordered by the stream alone, like
// everything above.

// Up to CC_LIKE_MAX_ROWS row numbers by value, in the kernel arguments (-1 behind the last one): the query rows of a
// cc_index_rank_like, for the gather and for the fold.
struct LikeRows { int n; int r[CC_LIKE_MAX_ROWS]; };

// out[i] = row i of the list decoded to f32.  One wave (one block) per row, one 16-byte piece of the stored row per lane and load,
// like compact_kernel: f32 the bytes as they are, bf16 the 16 bits moved to the high half, int8 (float)code * s_g with s_g from the
// row's trailer (a piece of 16 codes lies inside one group of 32).  The list: `rows` (pinned host memory) or, when that is null,
// `few` in the arguments, indexed by the block number alone, so that the number comes from a scalar load.  The numbers were checked
// on the host; the test here keeps every load inside the matrix whatever the list holds.
__global__ __launch_bounds__(64) void fetch_rows_kernel(const char* __restrict__ emb, const long long* __restrict__ rows, const LikeRows few, long size, int dim,
                                                        int storage, float* __restrict__ out) {
  const int lane = threadIdx.x;
  const long i = blockIdx.x;
  const long long r = rows ? rows[i] : (long long)few.r[blockIdx.x & (CC_LIKE_MAX_ROWS - 1)];
  if ((unsigned long long)r >= (unsigned long long)size) return;
  float4* o = reinterpret_cast<float4*>(out + (size_t)i * dim);
  if (storage == F32) {
    const float4* e = reinterpret_cast<const float4*>(emb + (size_t)r * dim * 4);
    for (int c = lane; c < (dim >> 2); c += 64) o[c] = e[c];
  } else if (storage == BF16) {
    const uint4* e = reinterpret_cast<const uint4*>(emb + (size_t)r * dim * 2);
    for (int c = lane; c < (dim >> 3); c += 64)
      decode_bf16_piece(e[c], o + 2 * c);
  } else {
    const char* e = emb + (size_t)r * ((size_t)dim + (dim >> 3));
    for (int c = lane; c < (dim >> 4); c += 64)
      decode_i8_piece(reinterpret_cast<const uint4*>(e)[c], reinterpret_cast<const float*>(e + dim)[c >> 1], o + 4 * c);
  }
}

// ---- compound search (cc_index_rank_terms / cc_index_timeline_terms) -----------------------------------------------------------------
// The fold of every ranking whose ONE score vector comes from several: S (T, n) -> S[0][r] = the ranking value of row r from the RANK
// terms, dead[r] from the REQUIRE / REJECT terms and the exclude flags, which[r] = the RANK term that made the value.  What each term is
// travels by value in the arguments.  cc_index_rank_like is the case "every term a stored row, RANK, MAX": the row-wise maximum in
// the order of the ranking keys (+0 beats -0), the same bits whichever of equal scores is kept.
struct TermParam { float weight, cut; int role, pad; };                      // 16 bytes: one scalar load per term
struct TermSpec { int T, combine, pad0, pad1; TermParam t[CC_TERMS_MAX]; };

// One row's state while the terms go by: v the sum so far (SUM), k the best key so far - ordered(product) under SUM, ordered(score)
// under MAX, its complement under MIN, so that every rule keeps the LARGEST key and 0 stands for "none yet" -, wh the term that
// brought k (-1: no RANK term yet), dead (0 / 1).
struct TermAcc { float v; unsigned k; int wh; unsigned dead; };

// Term t (what it is: m) scores the R rows of a thread x[0..R).  The role is tested once for all of them.  The product and the sum of
// SUM are two roundings: contraction is off in this function, so the compiler emits a multiply and an add, never an fma, and float32
// arithmetic on the host reproduces v bit for bit.  flip: ~0 under MIN, else 0.
template <int R>
__device__ __forceinline__ void term_step(TermAcc (&a)[R], const TermParam m, bool sum, unsigned flip, const float (&x)[R], int t) {
#pragma clang fp contract(off)
  if (m.role == CC_TERM_RANK) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      unsigned k;
      if (sum) {
        const float p = m.weight * x[j];
        a[j].v = a[j].v + p;
        k = ordered(p);
      } else {
        k = ordered(x[j]) ^ flip;
      }
      const bool take = k > a[j].k || a[j].wh < 0;                           // strictly larger: equal keys stay with the lower term
      a[j].k = take ? k : a[j].k; a[j].wh = take ? t : a[j].wh;
    }
  } else if (m.role == CC_TERM_REQUIRE) {
#pragma unroll
    for (int j = 0; j < R; ++j) a[j].dead |= x[j] >= m.cut ? 0u : 1u;
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) a[j].dead |= x[j] >= m.cut ? 1u : 0u;
  }
}

__device__ __forceinline__ float term_value(const TermAcc& a, bool sum, unsigned flip) { return sum ? a.v : unordered(a.k ^ flip); }

// A thread reads S[.][r] of its own rows and writes S[0][r], dead[r] (dead != null) and which[r] (which != null) of those rows only,
// so no thread reads what another one writes: no atomics, no LDS, no second score buffer, in place over row 0.  VEC (n % 4 == 0: row
// t of S starts at byte 4 t n, a multiple of 16 only then): four consecutive rows per thread, one 16-byte load per term, dead / which
// written as one 32-bit word each.  Otherwise one row per thread and 4-byte loads.
// What a term is is the same for every thread (one 16-byte scalar load from the arguments, uniform branches).  mode 1: the rows of
// `excl` are dead too (the stored rows that are RANK terms); mode 2: every row of group G and slot Tk is.
template <bool VEC>
__global__ __launch_bounds__(256) void terms_fold_kernel(float* __restrict__ S, long n, const int* __restrict__ grp, const int* __restrict__ trk, const TermSpec spec,
                                                         const LikeRows excl, int mode, int G, int Tk, unsigned char* __restrict__ dead,
                                                         unsigned char* __restrict__ which) {
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, nt = (long)gridDim.x * 256;
  const int T = spec.T;
  const bool sum = spec.combine == CC_COMBINE_SUM;
  const unsigned flip = spec.combine == CC_COMBINE_MIN ? ~0u : 0u;
  if (VEC) {
    const long n4 = n >> 2;
    float4* S4 = reinterpret_cast<float4*>(S);
    for (long i = tid; i < n4; i += nt) {
      TermAcc a[4] = {{0.f, 0u, -1, 0u}, {0.f, 0u, -1, 0u}, {0.f, 0u, -1, 0u}, {0.f, 0u, -1, 0u}};
      int t = 0;
      for (; t + 4 <= T; t += 4) {                                           // four independent loads in flight, then the four terms in order
        float4 x4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x4[u] = S4[(long)(t + u) * n4 + i];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float x[4] = {x4[u].x, x4[u].y, x4[u].z, x4[u].w};
          term_step<4>(a, spec.t[t + u], sum, flip, x, t + u);
        }
      }
      for (; t < T; ++t) {
        const float4 x4 = S4[(long)t * n4 + i];
        const float x[4] = {x4.x, x4.y, x4.z, x4.w};
        term_step<4>(a, spec.t[t], sum, flip, x, t);
      }
      S4[i] = make_float4(term_value(a[0], sum, flip), term_value(a[1], sum, flip), term_value(a[2], sum, flip), term_value(a[3], sum, flip));
      if (dead) {
        unsigned d = a[0].dead | a[1].dead << 8 | a[2].dead << 16 | a[3].dead << 24;
        if (mode == 2) {
          const int4 g = reinterpret_cast<const int4*>(grp)[i], k = reinterpret_cast<const int4*>(trk)[i];
          d |= (g.x == G && k.x == Tk ? 1u : 0u) | (g.y == G && k.y == Tk ? 1u << 8 : 0u) | (g.z == G && k.z == Tk ? 1u << 16 : 0u) | (g.w == G && k.w == Tk ? 1u << 24 : 0u);
        } else if (mode == 1) {
          for (int j = 0; j < excl.n; ++j) {
            const long k = (long)excl.r[j] - 4 * i;
            if (k >= 0 && k < 4) d |= 1u << (8 * (int)k);
          }
        }
        reinterpret_cast<unsigned*>(dead)[i] = d;
      }
      if (which) reinterpret_cast<unsigned*>(which)[i] = ((unsigned)a[0].wh & 255u) | ((unsigned)a[1].wh & 255u) << 8 | ((unsigned)a[2].wh & 255u) << 16 | ((unsigned)a[3].wh & 255u) << 24;
    }
  } else {
    for (long r = tid; r < n; r += nt) {
      TermAcc a[1] = {{0.f, 0u, -1, 0u}};
      int t = 0;
      for (; t + 4 <= T; t += 4) {
        float x4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x4[u] = S[(long)(t + u) * n + r];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float x[1] = {x4[u]};
          term_step<1>(a, spec.t[t + u], sum, flip, x, t + u);
        }
      }
      for (; t < T; ++t) {
        const float x[1] = {S[(long)t * n + r]};
        term_step<1>(a, spec.t[t], sum, flip, x, t);
      }
      S[r] = term_value(a[0], sum, flip);
      if (dead) {
        bool d = a[0].dead != 0u;
        if (mode == 2) d = d || (grp[r] == G && trk[r] == Tk);
        else if (mode == 1) for (int j = 0; j < excl.n; ++j) d = d || (long)excl.r[j] == r;
        dead[r] = d ? 1 : 0;
      }
      if (which) which[r] = (unsigned char)a[0].wh;
    }
  }
}

// Behind the emit step: which[o] = the term byte of the row idx[o] names, -1 where idx[o] is -1 (padding).  idx may be pinned host
// memory (the zero-copy route); the test keeps the load inside the column whatever it holds.
__global__ __launch_bounds__(256) void which_gather_kernel(const int* __restrict__ idx, const unsigned char* __restrict__ which_row, long n, size_t cnt,
                                                           int* __restrict__ which) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (size_t)gridDim.x * 256) {
    const int r = idx[i];
    which[i] = (r >= 0 && (long)r < n) ? (int)which_row[r] : -1;
  }
}

// ---- removal: stable compaction in place -------------------------------------------------------------------------------------
// Row r moves to pos(r) = the survivors before it, and pos(r) <= r.  Positions come from three passes: keep flags and survivor
// counts per granule of kGran rows, an exclusive scan of the counts by ONE block (64-bit), and the place inside the granule from a
// ballot in the mover.  No block waits for another one anywhere: what orders the passes and the slabs is the stream.
constexpr int kGran = 64;                 // rows per granule = rows per mover block (four waves x 16 rows)
constexpr int kSlabRows = 32768;          // rows of a bounced slab (cc_dev_set("index_slab_rows") overrides; docs/measurement.md has the sweep)

// keep[r] = 1 where row r survives, gcnt[g] = survivors of granule g.  drop set: group removal (a row goes when drop[its group] is
// non-zero; groups >= n_groups stay); otherwise keep[] holds the caller's drop bytes on entry.  One wave per granule.
__global__ __launch_bounds__(256) void keep_count_kernel(unsigned char* __restrict__ keep, const int* __restrict__ grp, const unsigned char* __restrict__ drop,
                                                         int n_groups, long n, unsigned* __restrict__ gcnt) {
  const int lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6), r = g * kGran + lane;
  bool k = false;
  if (r < n) {
    if (drop) { const unsigned gi = (unsigned)grp[r]; k = !(gi < (unsigned)n_groups && drop[gi]); }
    else k = keep[r] == 0;
    keep[r] = k ? 1 : 0;
  }
  const unsigned long long m = __ballot(k);
  if (lane == 0 && g * kGran < n) gcnt[g] = (unsigned)__popcll(m);
}

// goff[g] = sum of gcnt[0..g), goff[nb] = the number of survivors.  One block of 1024 threads walks the counts 1024 at a time.
__global__ __launch_bounds__(1024) void granule_offsets_kernel(const unsigned* __restrict__ gcnt, long nb, unsigned long long* __restrict__ goff) {
  __shared__ unsigned long long wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long carry = 0;
  for (long base = 0; base < nb; base += 1024) {
    const long i = base + tid;
    const unsigned long long c = i < nb ? gcnt[i] : 0ull;
    unsigned long long inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) { const unsigned long long v = wsum[j]; if (j < w) before += v; total += v; }
    if (i < nb) goff[i] = carry + before + inc - c;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) goff[nb] = carry;
}

// The mover: block b takes granule g0 + b.  Every wave ballots the granule's 64 keep flags and moves the survivors among its own
// 16 rows to goff[granule] - dst_sub + (survivors before the row in the granule): whole rows, `chunks` 16-byte pieces each, one
// piece per lane and load, four rows in flight per wave (a pure HBM kernel, like scan_kernel: 16 waves per CU with four
// independent 16-byte loads each).  grp / trk ride along.  dst is the matrix itself (direct: the caller guarantees that the
// destinations of this launch lie below its first source row) or the bounce buffer (dst_sub = survivors before the slab); either
// way no byte is both read and written by one launch, which is what __restrict__ says.
__global__ __launch_bounds__(256) void compact_kernel(const uint4* __restrict__ src, const int* __restrict__ sgrp, const int* __restrict__ strk,
                                                      uint4* __restrict__ dst, int* __restrict__ dgrp, int* __restrict__ dtrk,
                                                      const unsigned char* __restrict__ keep, const unsigned long long* __restrict__ goff,
                                                      long g0, long n, long dst_sub, int chunks) {
  const long g = g0 + blockIdx.x, r0 = g * kGran;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(r0 + lane < n && keep[r0 + lane] != 0);
  const long dbase = (long)goff[g] - dst_sub;
  if (lane < 16) {
    const int row = 16 * w + lane;
    if ((m >> row) & 1ull) {
      const long d = dbase + __popcll(m & ((1ull << row) - 1ull));
      dgrp[d] = sgrp[r0 + row]; dtrk[d] = strk[r0 + row];
    }
  }
  unsigned mine = (unsigned)((m >> (16 * w)) & 0xffffull);                   // the survivors among this wave's rows (wave-uniform)
  long d = dbase + __popcll(m & ((1ull << (16 * w)) - 1ull));
  const long s0 = (r0 + 16 * w) * chunks;
  while (mine) {
    long so[4]; int k = 0;                                                    // piece offsets of the next (up to) four survivors
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      so[u] = s0;
      if (mine) { so[u] = s0 + (long)(__ffs((int)mine) - 1) * chunks; mine &= mine - 1; ++k; }
    }
    const long o = d * chunks;
    if (k == 4) {
      for (int c = lane; c < chunks; c += 64) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = src[so[u] + c];
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[o + (long)u * chunks + c] = v[u];
      }
    } else {
      for (int c = lane; c < chunks; c += 64)
        for (int u = 0; u < k; ++u) dst[o + (long)u * chunks + c] = src[so[u] + c];
    }
    d += k;
  }
}

// A bounced slab back into the matrix: rows (n16 16-byte pieces) and their groups / slots, four loads in flight per thread.
__global__ __launch_bounds__(256) void copy_down_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16,
                                                        const int* __restrict__ sgrp, int* __restrict__ dgrp, const int* __restrict__ strk, int* __restrict__ dtrk, long rows) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nt = (size_t)gridDim.x * 256;
  size_t i = tid;
  for (; i + 3 * nt < n16; i += 4 * nt) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[i + u * nt];
#pragma unroll
    for (int u = 0; u < 4; ++u) dst[i + u * nt] = v[u];
  }
  for (; i < n16; i += nt) dst[i] = src[i];
  for (size_t i = tid; i < (size_t)rows; i += nt) { dgrp[i] = sgrp[i]; dtrk[i] = strk[i]; }
}

// The ts and cls columns follow their rows in a pass of their own, which leaves the movers above as they are: the columns as they
// were (sts / scls, a copy in scratch) are scattered to pos(r) = goff[granule] + the survivors before the row in its granule.  One
// wave per granule, like keep_count_kernel.  Source and destination are different buffers, so the order of the blocks is free.
__global__ __launch_bounds__(256) void attr_compact_kernel(const int* __restrict__ sts, const int* __restrict__ scls, int* __restrict__ dts, int* __restrict__ dcls,
                                                           const unsigned char* __restrict__ keep, const unsigned long long* __restrict__ goff, long n) {
  const int lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6), r = g * kGran + lane;
  const bool k = r < n && keep[r] != 0;
  const unsigned long long m = __ballot(k);
  if (k) {
    const long d = (long)goff[g] + __popcll(m & ((1ull << lane) - 1ull));
    dts[d] = sts[r]; dcls[d] = scls[r];
  }
}

__global__ void fill_i32_kernel(int* __restrict__ p, int v, size_t cnt) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

void ensure(void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return;
  if (*p) hipFree(*p);
  CC_HIP(hipMalloc(p, bytes + 256));
  *cap = bytes;
}

constexpr size_t kPinResultBytes = 1 << 20;      // results up to this size are written by the kernel straight into pinned host memory

void ensure_pinned(cc_index* h, size_t bytes) {
  if (h->pin_cap >= bytes) return;
  if (h->pin) hipHostFree(h->pin);
  h->pin = nullptr; h->pin_cap = 0;
  CC_HIP(hipHostMalloc((void**)&h->pin, bytes, hipHostMallocDefault));
  h->pin_cap = bytes;
}

// Host queries go through the pinned buffer (a pageable source makes the runtime stage and block; 3 KB per query).
void ensure_queries(cc_index* h, int Q) {
  if (h->q_cap < Q) { if (h->q_dev) hipFree(h->q_dev); h->q_dev = nullptr; h->q_cap = 0; CC_HIP(hipMalloc((void**)&h->q_dev, (size_t)Q * h->dim * 4 + 256)); h->q_cap = Q; }
}

void upload_queries(cc_index* h, const float* q, int Q, int on_device, hipStream_t s) {
  ensure_queries(h, Q);
  const size_t bytes = (size_t)Q * h->dim * 4;
  if (!on_device && bytes <= h->pin_cap) {
    memcpy(h->pin, q, bytes);
    CC_HIP(hipMemcpyAsync(h->q_dev, h->pin, bytes, hipMemcpyHostToDevice, s));
  } else {
    CC_HIP(hipMemcpyAsync(h->q_dev, q, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  }
}

void compute_scores(cc_index* h, int Q, hipStream_t s) {
  ensure((void**)&h->scores, &h->scores_cap, (size_t)Q * h->n * 4);
  // More than four queries: one pass over the matrix as a GEMM on the exact-f32 MFMA path (queries = the 128-row tile,
  // index rows = output channels, so every embedding is read from HBM once and scores come out (Q, N) row-major).
  // Sixteen GEMV passes for 64 queries become one.  Products are exact f32 either way; only the summation order differs
  // from the GEMV kernel (last-bit differences between the two paths).
  static const bool wide = [] { const char* e = getenv("CLEARCAM_SCAN"); return e ? atoi(e) != 0 : true; }();
  if (h->storage == BF16 && Q > 16 && h->n % 8 == 0 && h->n < (1L << 31)) {
    // many queries against bf16 rows: ONE pass as a bf16 MFMA GEMM (queries rounded to bf16 as well: scores within ~2e-3 of f32)
    if (h->q16_cap < Q) { if (h->q16) hipFree(h->q16); CC_HIP(hipMalloc((void**)&h->q16, (size_t)Q * h->dim * 2 + 256)); h->q16_cap = Q; }
    const size_t cnt = (size_t)Q * h->dim;
    hipLaunchKernelGGL(to_bf16_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, h->q_dev, h->q16, cnt);
    const ConvP g = gemm_params(h->q16, h->dim, Q, h->dim, h->emb, h->dim, nullptr, (int)h->n, h->scores, (int)h->n, 1, 0, nullptr, 0, 0);
    if (conv_mfma_supported(BF16, g)) { launch_conv_mfma(BF16, g, s); h->last_path = 1; return; }
  }
  h->last_path = 0;
  if (h->storage == CC_INDEX_I8) {
    // A batch of at least T queries goes to the MFMA kernel of index_i8_mfma.hip: one launch, every row read from HBM once, the same
    // exact products as the scan summed in another order (last-bit differences, like the f32 GEMM below).  T: cc_dev_set
    // ("index_i8_mfma"), 0 = never, -1 = kI8MfmaFrom.  Rows wider than kIndexI8MfmaMaxDim stay with the scan.
    const int key = g_index_i8_mfma.load(), T = key < 0 ? kI8MfmaFrom : key;
    if (T > 0 && Q >= T && index_i8_mfma_supported(h->dim, (long)h->n)) {
      ensure(&h->q_planes, &h->q_planes_cap, index_i8_mfma_plane_bytes(h->dim, Q));
      launch_index_i8_mfma(h->emb, h->q_dev, h->q_planes, h->scores, (long)h->n, h->dim, Q, s);
      h->last_path = 2;
      return;
    }
    // Smaller batches go through repeated scan passes, bit-identical to single queries.  The pass width is a
    // measured choice (docs/measurement.md, "int8 rows"): one convert and QB fma per code keep a pass at HBM speed only while QB is
    // small.  cc_dev_set("index_i8_pass") overrides it (1..8); the LDS copy of the queries caps it at 64 KB / (dim * 4).
    int W = g_index_i8_pass.load();
    W = std::max(1, std::min(std::min(W > 0 ? W : kI8Pass, 8), 16384 / h->dim));
    for (int q0 = 0; q0 < Q; q0 += W) {
      const float* q = h->q_dev + (size_t)q0 * h->dim; float* out = h->scores + (size_t)q0 * h->n;
      switch (std::min(W, Q - q0)) {
        case 1: launch_scan_i8<1>(h, q, out, s); break;  case 2: launch_scan_i8<2>(h, q, out, s); break;
        case 3: launch_scan_i8<3>(h, q, out, s); break;  case 4: launch_scan_i8<4>(h, q, out, s); break;
        case 5: launch_scan_i8<5>(h, q, out, s); break;  case 6: launch_scan_i8<6>(h, q, out, s); break;
        case 7: launch_scan_i8<7>(h, q, out, s); break;  default: launch_scan_i8<8>(h, q, out, s); break;
      }
    }
    CC_HIP(hipGetLastError());
    return;
  }
  const int W = scan_pass_width(h->dim);            // 8 unless the rows are wider than 5120
  if (h->storage == BF16) {                         // bf16 rows: W queries per pass over half the bytes (dim % 256 == 0 is checked at create)
    for (int q0 = 0; q0 < Q; q0 += W) {
      const float* q = h->q_dev + (size_t)q0 * h->dim; float* out = h->scores + (size_t)q0 * h->n;
      switch (std::min(W, Q - q0)) {
        case 1: launch_scan_bf16<1>(h, q, out, s); break;  case 2: launch_scan_bf16<2>(h, q, out, s); break;
        case 3: launch_scan_bf16<3>(h, q, out, s); break;  case 4: launch_scan_bf16<4>(h, q, out, s); break;
        case 5: launch_scan_bf16<5>(h, q, out, s); break;  case 6: launch_scan_bf16<6>(h, q, out, s); break;
        case 7: launch_scan_bf16<7>(h, q, out, s); break;  default: launch_scan_bf16<8>(h, q, out, s); break;
      }
    }
    CC_HIP(hipGetLastError());
    return;
  }
  const bool scan8 = wide && h->dim % 256 == 0 && h->dim <= 4096;   // scan_kernel: up to 8 queries per pass at HBM speed
  // measured on a 125 k x 768 shard: a scan pass costs ~65 us whatever its query count (1..8), the GEMM ~220 us flat up to 128 queries
  if (Q > (scan8 ? 16 : 4) && h->n % 4 == 0 && h->dim % 32 == 0) {
    const ConvP g = gemm_params(h->q_dev, h->dim, Q, h->dim, h->emb, h->dim, nullptr, (int)h->n, h->scores, (int)h->n, 1, 0, nullptr, 0, 0);
    if (h->n < (1L << 31) && conv_mfma_supported(F32, g)) { launch_conv_mfma(F32, g, s); h->last_path = 1; return; }
  }
  if (scan8) {                                      // dim <= 4096: W is 8
    for (int q0 = 0; q0 < Q; q0 += W) {
      const float* q = h->q_dev + (size_t)q0 * h->dim; float* out = h->scores + (size_t)q0 * h->n;
      switch (std::min(W, Q - q0)) {
        case 1: launch_scan<1>(h, q, out, s); break;  case 2: launch_scan<2>(h, q, out, s); break;
        case 3: launch_scan<3>(h, q, out, s); break;  case 4: launch_scan<4>(h, q, out, s); break;
        case 5: launch_scan<5>(h, q, out, s); break;  case 6: launch_scan<6>(h, q, out, s); break;
        case 7: launch_scan<7>(h, q, out, s); break;  default: launch_scan<8>(h, q, out, s); break;
      }
    }
    CC_HIP(hipGetLastError());
    return;
  }
  const int blocks = (int)std::min<int64_t>((h->n + 3) / 4, 256 * 16);
  for (int q0 = 0; q0 < Q; q0 += 4) {
    const int nq = std::min(4, Q - q0);
    hipLaunchKernelGGL(scores_kernel<4>, dim3(blocks), dim3(256), 0, s, h->emb, h->q_dev + (size_t)q0 * h->dim, h->scores + (size_t)q0 * h->n,
                       (long)h->n, h->dim, nq);
  }
  CC_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

int cc_index_create_ex(cc_index** h, int dim, int64_t capacity, int device, int storage) {
  CC_API_BEGIN
  CC_CHECK(h && dim > 0 && dim % 4 == 0 && capacity > 0, "bad argument (dim must be a multiple of 4)");
  CC_CHECK(storage == F32 || storage == BF16 || storage == CC_INDEX_I8, "index storage must be 0 (f32), 2 (bf16) or 8 (int8 with group scales)");
  // one query of a scan pass has to fit into the LDS of a CU (kScanLdsFloats): a wider bf16 row is refused here, not at the first search
  CC_CHECK(storage != BF16 || (dim % 256 == 0 && dim <= kScanLdsFloats), "a bf16 index needs dim % 256 == 0 (and dim <= 40960)");
  CC_CHECK(storage != CC_INDEX_I8 || (dim % 256 == 0 && dim <= 16384), "an int8 index needs dim % 256 == 0 (and dim <= 16384)");
  int n = 0; CC_HIP(hipGetDeviceCount(&n));
  CC_CHECK(n > 0 && device >= 0 && device < n, "no such HIP device");
  CC_HIP(hipSetDevice(device));
  std::unique_ptr<cc_index> x(new cc_index());
  x->dim = dim; x->capacity = capacity; x->device = device; x->storage = storage;
  CC_HIP(hipMalloc((void**)&x->emb, (size_t)capacity * x->row_bytes() + 256));
  CC_HIP(hipMalloc((void**)&x->grp, (size_t)capacity * 4 + 256));
  CC_HIP(hipMalloc((void**)&x->trk, (size_t)capacity * 4 + 256));
  CC_HIP(hipMalloc((void**)&x->ts, (size_t)capacity * 4 + 256));
  CC_HIP(hipMalloc((void**)&x->cls, (size_t)capacity * 4 + 256));
  x->stream = pool_stream_get(device);
  *h = x.release();
  CC_API_END
}

int cc_index_create(cc_index** h, int dim, int64_t capacity, int device) { return cc_index_create_ex(h, dim, capacity, device, F32); }

// Append n rows (f32 in; rounded to bf16 for a bf16 index, quantised for an int8 one) with their group ids (null: group 0) and track slots (null: -1, no
// track).  The matrix grows geometrically when it is full (new allocation, device-to-device copy, swap), so callers never see a
// capacity error.  ts / cls: the two per-row attributes (null: none), which grow and move with the rows.
int cc_index_add_described(cc_index* h, const float* emb, int64_t n, int on_device, const int32_t* groups, const int32_t* tracks,
                           const int32_t* ts, const int32_t* cls) {
  CC_API_BEGIN
  CC_CHECK(h && (emb || n == 0) && n >= 0, "bad argument");
  if (cls)
    for (int64_t i = 0; i < n; ++i) CC_CHECK(cls[i] >= -1 && cls[i] <= 255, "row classes must be in [0, 255] or -1");
  int n_slots = h->n_slots;
  if (tracks)
    for (int64_t i = 0; i < n; ++i) {
      CC_CHECK(tracks[i] >= -1 && tracks[i] < (1 << 24), "track slots must be in [0, 2^24) or -1");
      n_slots = std::max(n_slots, tracks[i] + 1);
    }
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));            // a search on our stream may still be reading the matrix
  if (h->n + n > h->capacity) {
    int64_t cap = h->capacity;
    while (cap < h->n + n) cap *= 2;
    CC_CHECK((size_t)cap * h->row_bytes() < ((size_t)1 << 40), "index would exceed 1 TiB");
    float* emb2 = nullptr; int* col2[4] = {nullptr, nullptr, nullptr, nullptr};      // grp, trk, ts, cls
    CC_HIP(hipMalloc((void**)&emb2, (size_t)cap * h->row_bytes() + 256));
    for (int c = 0; c < 4; ++c)
      if (hipMalloc((void**)&col2[c], (size_t)cap * 4 + 256) != hipSuccess) {
        hipFree(emb2);
        for (int d = 0; d < c; ++d) hipFree(col2[d]);
        throw cc::Error(-12, "out of device memory growing the index");
      }
    int** col[4] = {&h->grp, &h->trk, &h->ts, &h->cls};
    CC_HIP(hipMemcpy(emb2, h->emb, (size_t)h->n * h->row_bytes(), hipMemcpyDeviceToDevice));
    for (int c = 0; c < 4; ++c) CC_HIP(hipMemcpy(col2[c], *col[c], (size_t)h->n * 4, hipMemcpyDeviceToDevice));
    hipFree(h->emb); h->emb = emb2; h->capacity = cap;
    for (int c = 0; c < 4; ++c) { hipFree(*col[c]); *col[c] = col2[c]; }
  }
  if (n) {
    char* dst = reinterpret_cast<char*>(h->emb) + (size_t)h->n * h->row_bytes();
    if (h->storage == F32) {
      CC_HIP(hipMemcpy(dst, emb, (size_t)n * h->dim * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    } else {
      const size_t cnt = (size_t)n * h->dim;
      const float* src = emb; float* tmp = nullptr;
      if (!on_device) { CC_HIP(hipMalloc((void**)&tmp, cnt * 4)); CC_HIP(hipMemcpy(tmp, emb, cnt * 4, hipMemcpyHostToDevice)); src = tmp; }
      // Device-resident rows may still be being written by the caller's stream (torch's, not ours): the conversion kernel runs on
      // the index's private non-blocking stream, which nothing orders behind that producer.  The f32 path is ordered by its
      // blocking hipMemcpy; here the producer is waited for explicitly (add is not a hot path).
      else CC_HIP(hipDeviceSynchronize());
      const dim3 grid((unsigned)std::min<size_t>((cnt + 255) / 256, 65535));
      if (h->storage == CC_INDEX_I8) hipLaunchKernelGGL(quantise_i8_kernel, grid, dim3(256), 0, h->stream, src, dst, cnt, h->dim);
      else hipLaunchKernelGGL(to_bf16_kernel, grid, dim3(256), 0, h->stream, src, reinterpret_cast<uint16_t*>(dst), cnt);
      CC_HIP(hipGetLastError());
      CC_HIP(hipStreamSynchronize(h->stream));
      if (tmp) hipFree(tmp);
    }
    if (groups) CC_HIP(hipMemcpy(h->grp + h->n, groups, (size_t)n * 4, hipMemcpyHostToDevice));
    else CC_HIP(hipMemset(h->grp + h->n, 0, (size_t)n * 4));
    if (tracks) CC_HIP(hipMemcpy(h->trk + h->n, tracks, (size_t)n * 4, hipMemcpyHostToDevice));
    else CC_HIP(hipMemset(h->trk + h->n, 0xff, (size_t)n * 4));
    if (ts) CC_HIP(hipMemcpy(h->ts + h->n, ts, (size_t)n * 4, hipMemcpyHostToDevice));
    else {
      hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, h->stream, h->ts + h->n, (int)CC_ROW_NO_TS, (size_t)n);
      CC_HIP(hipGetLastError());
      CC_HIP(hipStreamSynchronize(h->stream));
    }
    if (cls) CC_HIP(hipMemcpy(h->cls + h->n, cls, (size_t)n * 4, hipMemcpyHostToDevice));
    else CC_HIP(hipMemset(h->cls + h->n, 0xff, (size_t)n * 4));
    h->grp_host.resize((size_t)h->n); h->trk_host.resize((size_t)h->n);      // what an add that failed half way may have left behind
    if (groups) h->grp_host.insert(h->grp_host.end(), groups, groups + n); else h->grp_host.insert(h->grp_host.end(), (size_t)n, 0);
    if (tracks) h->trk_host.insert(h->trk_host.end(), tracks, tracks + n); else h->trk_host.insert(h->trk_host.end(), (size_t)n, -1);
  }
  h->n += n;
  h->n_slots = n_slots;
  CC_API_END
}

int cc_index_add_tracked(cc_index* h, const float* emb, int64_t n, int on_device, const int32_t* groups, const int32_t* tracks) {
  return cc_index_add_described(h, emb, n, on_device, groups, tracks, nullptr, nullptr);
}

int cc_index_row_info(cc_index* h, int64_t row0, int64_t n, int32_t* ts_out, int32_t* cls_out) {
  CC_API_BEGIN
  CC_CHECK(h, "null index");
  CC_CHECK(row0 >= 0 && n >= 0 && row0 <= h->n && n <= h->n - row0, "rows outside the index");
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  if (n && ts_out) CC_HIP(hipMemcpy(ts_out, h->ts + row0, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (n && cls_out) CC_HIP(hipMemcpy(cls_out, h->cls + row0, (size_t)n * 4, hipMemcpyDeviceToHost));
  CC_API_END
}

int cc_index_add_grouped(cc_index* h, const float* emb, int64_t n, int on_device, const int32_t* groups) {
  return cc_index_add_tracked(h, emb, n, on_device, groups, nullptr);
}

int cc_index_add(cc_index* h, const float* emb, int64_t n, int on_device) { return cc_index_add_grouped(h, emb, n, on_device, nullptr); }

int cc_index_info(cc_index* h, int64_t* capacity, int* storage, int* dim) {
  CC_API_BEGIN
  CC_CHECK(h, "null argument");
  if (capacity) *capacity = h->capacity;
  if (storage) *storage = h->storage;
  if (dim) *dim = h->dim;
  CC_API_END
}

int cc_index_size(cc_index* h, int64_t* n) {
  CC_API_BEGIN
  CC_CHECK(h && n, "null argument");
  *n = h->n;
  CC_API_END
}

int cc_index_last_path(cc_index* h, int* path) {
  CC_API_BEGIN
  CC_CHECK(h && path, "null argument");
  *path = h->last_path;
  CC_API_END
}

int cc_index_scores(cc_index* h, const float* q, int Q, float* scores, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && q && scores && Q > 0, "bad argument");
  CC_HIP(hipSetDevice(h->device));
  if (h->n == 0) return 0;
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  upload_queries(h, q, Q, on_device, s);
  compute_scores(h, Q, s);
  CC_HIP(hipMemcpyAsync(scores, h->scores, (size_t)Q * h->n * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  if (!on_device) CC_HIP(hipStreamSynchronize(s));
  CC_API_END
}

}  // extern "C"

namespace cc { std::atomic<int> g_index_slab_rows{-1}; std::atomic<int> g_index_i8_pass{-1}; std::atomic<int> g_index_i8_mfma{-1}; }

namespace {

// Removal behind cc_index_remove_rows (by_rows; drop: one byte per row) and cc_index_remove_groups (drop: one byte per group id).
// The launches, all on the index's stream:
//   keep flags + granule counts, the scan, and the granule offsets back to the host (8 bytes per 64 rows), which cuts the slabs;
//   nothing for the granules before the first removed row (they stay where they are);
//   from there on, with a = the first row not yet moved and gap = a - pos(a) the rows removed before it:
//     gap >= T / 4: a DIRECT slab [a, b), b the last granule boundary with pos(b) <= a.  It writes [pos(a), pos(b)), all below a,
//       so neither its own sources nor those of any later slab; everything before a has been moved by earlier launches.
//     otherwise a BOUNCED slab of T rows: survivors gathered into the handle's bounce buffer, then copied down to
//       [pos(a), pos(a) + survivors), which ends at or below a + T, the start of the next slab.
// Direct slabs grow with the gap, so once the removed rows before a slab outnumber T / 4 no row is moved twice.
int remove_impl(cc_index* h, bool by_rows, const uint8_t* drop, int64_t n_rows, int n_groups, int64_t* removed) {
  CC_API_BEGIN
  CC_CHECK(h, "null index");
  if (removed) *removed = 0;
  if (by_rows) CC_CHECK(n_rows == h->n, "the drop mask must have one byte per row of the index");
  else CC_CHECK(n_groups > 0 && n_groups <= (1 << 24), "bad group count");
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));            // a search on our stream may still be reading the matrix
  const int64_t n = h->n;
  if (n == 0) return 0;
  CC_CHECK(drop, "null drop table");
  if (std::all_of(drop, drop + (by_rows ? (size_t)n : (size_t)n_groups), [](uint8_t b) { return b == 0; })) return 0;
  hipStream_t s = h->stream;
  const int64_t nb = (n + kGran - 1) / kGran;
  ensure((void**)&h->keep, &h->keep_cap, (size_t)n);
  ensure((void**)&h->gcnt, &h->gcnt_cap, (size_t)nb * 4);
  ensure((void**)&h->goff, &h->goff_cap, (size_t)(nb + 1) * 8);
  const unsigned char* drop_dev = nullptr;
  if (by_rows) CC_HIP(hipMemcpyAsync(h->keep, drop, (size_t)n, hipMemcpyHostToDevice, s));
  else {
    ensure((void**)&h->drop_grp, &h->drop_grp_cap, (size_t)n_groups);
    CC_HIP(hipMemcpyAsync(h->drop_grp, drop, (size_t)n_groups, hipMemcpyHostToDevice, s));
    drop_dev = h->drop_grp;
  }
  hipLaunchKernelGGL(keep_count_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, h->keep, h->grp, drop_dev, n_groups, (long)n, h->gcnt);
  hipLaunchKernelGGL(granule_offsets_kernel, dim3(1), dim3(1024), 0, s, h->gcnt, (long)nb, h->goff);
  CC_HIP(hipGetLastError());
  std::vector<unsigned long long> off((size_t)nb + 1);
  CC_HIP(hipMemcpyAsync(off.data(), h->goff, off.size() * 8, hipMemcpyDeviceToHost, s));
  CC_HIP(hipStreamSynchronize(s));
  const int64_t total = (int64_t)off[nb];
  if (total == n) return 0;                          // group removal that met no row
  int64_t T = g_index_slab_rows.load();
  T = T > 0 ? (T + kGran - 1) / kGran * kGran : kSlabRows;
  // ts / cls: the columns to scratch, then scattered by keep / goff (attr_compact_kernel); neither is touched by the movers below
  ensure((void**)&h->attr_tmp, &h->attr_tmp_cap, (size_t)n * 8);
  CC_HIP(hipMemcpyAsync(h->attr_tmp, h->ts, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  CC_HIP(hipMemcpyAsync(h->attr_tmp + n, h->cls, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(attr_compact_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, h->attr_tmp, h->attr_tmp + n, h->ts, h->cls, h->keep, h->goff, (long)n);
  const int64_t direct_min = std::max<int64_t>(kGran, T / 4);
  const size_t rb = h->row_bytes();
  const int chunks = (int)(rb / 16);                 // dim % 4 == 0 (f32) / dim % 256 == 0 (bf16; int8: dim + dim / 8 bytes, a multiple of 32): whole 16-byte pieces
  char* emb = reinterpret_cast<char*>(h->emb);
  int64_t ga = 0;                                    // granules before the first removed row stay where they are
  while (ga < nb && (int64_t)off[ga + 1] - (int64_t)off[ga] == std::min<int64_t>(kGran, n - ga * kGran)) ++ga;
  while (ga < nb) {
    const int64_t a = ga * kGran, pa = (int64_t)off[ga];
    int64_t gb;
    if (a - pa >= direct_min) {
      // the last boundary whose position is <= a; the next granule qualifies because it holds at most kGran <= gap survivors
      gb = (std::upper_bound(off.begin() + ga + 1, off.end(), (unsigned long long)a) - off.begin()) - 1;
      CC_CHECK(gb > ga, "index compaction made no progress");
      if ((int64_t)off[gb] > pa)
        hipLaunchKernelGGL(compact_kernel, dim3((unsigned)(gb - ga)), dim3(256), 0, s, reinterpret_cast<const uint4*>(emb), h->grp, h->trk,
                           reinterpret_cast<uint4*>(emb), h->grp, h->trk, h->keep, h->goff, (long)ga, (long)n, 0L, chunks);
    } else {
      gb = std::min<int64_t>(nb, ga + T / kGran);
      const int64_t ns = (int64_t)off[gb] - pa;
      if (ns > 0) {
        const size_t emb_bytes = ((size_t)T * rb + 255) & ~(size_t)255, ids_bytes = ((size_t)T * 4 + 255) & ~(size_t)255;
        ensure((void**)&h->bounce, &h->bounce_cap, emb_bytes + 2 * ids_bytes);
        int* bgrp = reinterpret_cast<int*>(h->bounce + emb_bytes); int* btrk = reinterpret_cast<int*>(h->bounce + emb_bytes + ids_bytes);
        hipLaunchKernelGGL(compact_kernel, dim3((unsigned)(gb - ga)), dim3(256), 0, s, reinterpret_cast<const uint4*>(emb), h->grp, h->trk,
                           reinterpret_cast<uint4*>(h->bounce), bgrp, btrk, h->keep, h->goff, (long)ga, (long)n, (long)pa, chunks);
        const size_t n16 = (size_t)ns * chunks;
        const unsigned blocks = (unsigned)std::min<size_t>((n16 + 1023) / 1024, 256 * 16);
        hipLaunchKernelGGL(copy_down_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(h->bounce),
                           reinterpret_cast<uint4*>(emb + (size_t)pa * rb), n16, bgrp, h->grp + pa, btrk, h->trk + pa, (long)ns);
      }
    }
    ga = gb;
  }
  CC_HIP(hipGetLastError());
  CC_HIP(hipStreamSynchronize(s));
  {                                                  // the host copies of grp / trk follow: the same keep rule, the same stable order
    int64_t d = 0;
    for (int64_t r = 0; r < n; ++r) {
      const bool gone = by_rows ? drop[r] != 0 : ((unsigned)h->grp_host[r] < (unsigned)n_groups && drop[h->grp_host[r]] != 0);
      if (!gone) { h->grp_host[d] = h->grp_host[r]; h->trk_host[d] = h->trk_host[r]; ++d; }
    }
    CC_CHECK(d == total, "the host columns and the device disagree about the survivors");
    h->grp_host.resize((size_t)d); h->trk_host.resize((size_t)d);
  }
  h->n = total;
  if (removed) *removed = n - total;
  CC_API_END
}

// The per-group filter of a call on the device (h->allowed, zero beyond n_groups), or null without one.
const unsigned char* upload_allowed(cc_index* h, const uint8_t* allowed, int n_groups, hipStream_t s) {
  if (!allowed) return nullptr;
  if (h->allowed_cap < n_groups) {
    if (h->allowed) hipFree(h->allowed);
    h->allowed = nullptr; h->allowed_cap = 0;
    int cap = 1024; while (cap < n_groups) cap *= 2;
    CC_HIP(hipMalloc((void**)&h->allowed, (size_t)cap)); h->allowed_cap = cap;
  }
  CC_HIP(hipMemsetAsync(h->allowed, 0, (size_t)h->allowed_cap, s));
  CC_HIP(hipMemcpyAsync(h->allowed, allowed, (size_t)n_groups, hipMemcpyHostToDevice, s));
  return h->allowed;
}

// The caller's row filter, checked, as the kernels take it.
RowWhere make_where(const cc_index* h, const cc_row_filter* where) {
  RowWhere w{};
  if (!where) return w;
  if (where->use_ts) {
    CC_CHECK(where->ts_min <= where->ts_max, "empty time window (ts_min > ts_max)");
    w.ts = h->ts; w.ts_min = where->ts_min; w.ts_max = where->ts_max;
  }
  if (where->use_cls) {
    CC_CHECK((where->cls_mask[0] | where->cls_mask[1] | where->cls_mask[2] | where->cls_mask[3]) != 0, "empty class set (all-zero mask)");
    w.cls = h->cls; w.m0 = where->cls_mask[0]; w.m1 = where->cls_mask[1]; w.m2 = where->cls_mask[2]; w.m3 = where->cls_mask[3];
  }
  return w;
}

// Room for (Q, k) answers in h->idx_dev / h->sc_dev: where search() and rank() leave what a copy then takes to the caller.
void ensure_out(cc_index* h, size_t ob) {
  if (h->out_cap >= ob) return;
  if (h->idx_dev) hipFree(h->idx_dev);
  if (h->sc_dev) hipFree(h->sc_dev);
  h->idx_dev = nullptr; h->sc_dev = nullptr; h->out_cap = 0;
  CC_HIP(hipMalloc((void**)&h->idx_dev, ob * 4 + 256)); CC_HIP(hipMalloc((void**)&h->sc_dev, ob * 4 + 256)); h->out_cap = ob;
}

// The track reduction of search() and rank_keys() over the (Q, n) scores: h->best and h->first made and cleared, then the launch.  n > 0.
void track_reduce(cc_index* h, int Q, const unsigned char* allowed_dev, const RowWhere& w, hipStream_t s) {
  const long n = (long)h->n;
  const int T = std::max(h->n_slots, 1);
  ensure((void**)&h->best, &h->best_cap, (size_t)Q * T * 8);
  ensure((void**)&h->first, &h->first_cap, (size_t)T * 4);
  CC_HIP(hipMemsetAsync(h->best, 0, (size_t)Q * T * 8, s));
  CC_HIP(hipMemsetAsync(h->first, 0xff, (size_t)T * 4, s));
  hipLaunchKernelGGL(track_reduce_kernel, dim3((unsigned)((n + kTrkRows - 1) / kTrkRows), Q), dim3(256), 0, s, h->scores, n, T, h->trk, h->grp,
                     allowed_dev, h->allowed_cap, w, h->best, h->first);
}

// Top-k among the rows whose group is allowed (allowed: n_groups bytes on the HOST, one per group id, non-zero = keep;
// null = every row).  Rows of a group id >= n_groups are filtered out.  tracks: the answers are tracks (their best row) and
// slot-less rows instead of rows - one more pass over scores + trk between the scan and the selection.
int search(cc_index* h, const float* q, int Q, int k, const uint8_t* allowed, int n_groups, int32_t* idx, float* score,
           int on_device, void* stream, bool tracks) {
  CC_API_BEGIN
  CC_CHECK(h && q && idx && score && Q > 0, "bad argument");
  CC_CHECK(k > 0 && k <= kMaxK, "k must be in [1, 1024]");
  CC_CHECK(!tracks || h->n < (1LL << 31), "a track search needs fewer than 2^31 rows");   // keys hold ~row and ~(n + row) in 32 bits
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const size_t ob = (size_t)Q * k;
  ensure_out(h, ob);
  const int nchunk = (int)std::max<int64_t>(1, (h->n + kChunk - 1) / kChunk);
  ensure((void**)&h->cand, &h->cand_cap, (size_t)Q * nchunk * k * 8);
  // Host caller with a small result (the interactive case: one query, k = 100): the merge kernel writes (id, score) into
  // pinned host memory and the only host-side wait is the stream synchronize - no pageable copies in either direction.
  const size_t qbytes = ((size_t)Q * h->dim * 4 + 255) & ~(size_t)255;
  const bool zero_copy = !on_device && ob * 8 <= kPinResultBytes;
  if (zero_copy) ensure_pinned(h, qbytes + ob * 8);
  int* idx_out = zero_copy ? reinterpret_cast<int*>(h->pin + qbytes) : h->idx_dev;
  float* sc_out = zero_copy ? reinterpret_cast<float*>(h->pin + qbytes + ob * 4) : h->sc_dev;
  CC_CHECK(!allowed || (n_groups > 0 && n_groups <= (1 << 24)), "bad group count");
  // the kernel indexes the bitmap with the row's group id: upload_allowed sizes it for every id the caller may have used (ids are < 2^24)
  const unsigned char* allowed_dev = upload_allowed(h, allowed, n_groups, s);
  if (h->n > 0) {
    upload_queries(h, q, Q, on_device, s);
    compute_scores(h, Q, s);
    if (tracks) {
      const int T = std::max(h->n_slots, 1);
      ensure((void**)&h->key_hi, &h->key_hi_cap, (size_t)Q * h->n * 4);
      track_reduce(h, Q, allowed_dev, RowWhere{}, s);
      hipLaunchKernelGGL(topk_stage1<true>, dim3(nchunk, Q), dim3(1024), 0, s, h->scores, (long)h->n, k, h->cand, h->grp, allowed_dev, h->allowed_cap,
                         h->trk, h->best, h->first, T, h->key_hi);
    } else {
      hipLaunchKernelGGL(topk_stage1<false>, dim3(nchunk, Q), dim3(1024), 0, s, h->scores, (long)h->n, k, h->cand, h->grp, allowed_dev, h->allowed_cap,
                         nullptr, nullptr, nullptr, 0, nullptr);
    }
  } else {
    CC_HIP(hipMemsetAsync(h->cand, 0, (size_t)Q * nchunk * k * 8, s));
  }
  if (tracks) hipLaunchKernelGGL(topk_stage2<true>, dim3(Q), dim3(1024), 0, s, h->cand, (long)nchunk * k, k, idx_out, sc_out, (long)h->n, h->trk, h->best, std::max(h->n_slots, 1));
  else hipLaunchKernelGGL(topk_stage2<false>, dim3(Q), dim3(1024), 0, s, h->cand, (long)nchunk * k, k, idx_out, sc_out, (long)h->n, nullptr, nullptr, 0);
  CC_HIP(hipGetLastError());
  if (zero_copy) {
    CC_HIP(hipStreamSynchronize(s));
    memcpy(idx, idx_out, ob * 4);
    memcpy(score, sc_out, ob * 4);
  } else {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    CC_HIP(hipMemcpyAsync(idx, h->idx_dev, ob * 4, kind, s));
    CC_HIP(hipMemcpyAsync(score, h->sc_dev, ob * 4, kind, s));
    if (!on_device) CC_HIP(hipStreamSynchronize(s));
  }
  CC_API_END
}

// What cc_index_rank_where and cc_index_timeline share behind the scan: (track reduction,) keys + totals.  n > 0.
void rank_keys(cc_index* h, int Q, bool tracks, float min_score, const unsigned char* allowed_dev, const RowWhere& w, unsigned* tot_dev, hipStream_t s) {
  const long n = (long)h->n;
  ensure((void**)&h->key_hi, &h->key_hi_cap, (size_t)Q * n * 4);
  const unsigned nblk = (unsigned)((n + kRankRows - 1) / kRankRows);
  const int T = std::max(h->n_slots, 1);
  if (tracks) {
    track_reduce(h, Q, allowed_dev, w, s);
    hipLaunchKernelGGL(rank_keys_kernel<true>, dim3(nblk, Q), dim3(256), 0, s, h->scores, n, h->grp, allowed_dev, h->allowed_cap, h->trk, h->best, h->first, T,
                       min_score, w, h->key_hi, tot_dev);
  } else {
    hipLaunchKernelGGL(rank_keys_kernel<false>, dim3(nblk, Q), dim3(256), 0, s, h->scores, n, h->grp, allowed_dev, h->allowed_cap, nullptr, nullptr, nullptr, 0,
                       min_score, w, h->key_hi, tot_dev);
  }
}

void check_rows(const cc_index* h, const int64_t* rows, int n) {
  for (int i = 0; i < n; ++i) CC_CHECK(rows[i] >= 0 && rows[i] < h->n, "a row number outside the index");
}

LikeRows like_rows(const int64_t* rows, int n) {
  LikeRows lr; lr.n = n;
  for (int i = 0; i < CC_LIKE_MAX_ROWS; ++i) lr.r[i] = i < n ? (int)rows[i] : -1;
  return lr;
}

// rows -> h->rows_pin, once the last launch that read it is through.  The caller launches its reader and records h->rows_ev behind it.
void pin_rows(cc_index* h, const int64_t* rows, int n) {
  if (!h->rows_ev) CC_HIP(hipEventCreateWithFlags(&h->rows_ev, hipEventDisableTiming));
  CC_HIP(hipEventSynchronize(h->rows_ev));
  const size_t bytes = (size_t)n * 8;
  if (h->rows_pin_cap < bytes) {
    if (h->rows_pin) hipHostFree(h->rows_pin);
    h->rows_pin = nullptr; h->rows_pin_cap = 0;
    size_t cap = 4096;
    while (cap < bytes) cap *= 2;
    CC_HIP(hipHostMalloc((void**)&h->rows_pin, cap, hipHostMallocDefault));
    h->rows_pin_cap = cap;
  }
  for (int i = 0; i < n; ++i) h->rows_pin[i] = rows[i];
}

// rows (checked by the caller) -> out (n, dim) f32 on the device, one launch of fetch_rows_kernel.  Up to CC_LIKE_MAX_ROWS numbers
// (every cc_index_rank_like) travel in the kernel arguments: copied at the launch, nothing to keep alive.  A longer list goes
// through pinned memory.  A call that returns without waiting for the stream (device results) leaves a gather behind that has yet
// to read it, so that buffer is this function's alone and is rewritten only behind the event recorded after the last such gather.
void gather_rows(cc_index* h, const int64_t* rows, int n, float* out, hipStream_t s) {
  if (n <= CC_LIKE_MAX_ROWS && h->n < (1LL << 31)) {
    hipLaunchKernelGGL(fetch_rows_kernel, dim3((unsigned)n), dim3(64), 0, s, reinterpret_cast<const char*>(h->emb), (const long long*)nullptr, like_rows(rows, n),
                       (long)h->n, h->dim, h->storage, out);
    CC_HIP(hipGetLastError());
    return;
  }
  pin_rows(h, rows, n);
  hipLaunchKernelGGL(fetch_rows_kernel, dim3((unsigned)n), dim3(64), 0, s, reinterpret_cast<const char*>(h->emb), (const long long*)h->rows_pin, LikeRows{}, (long)h->n,
                     h->dim, h->storage, out);
  CC_HIP(hipGetLastError());
  CC_HIP(hipEventRecord(h->rows_ev, s));
}

// The query side of a folded ranking (cc_index_rank_terms / cc_index_timeline_terms, cc_index_rank_like), checked: the vectors, the rows, what each term is (spec), which
// rows the exclude bits kill (mode 0 nothing, 1 the rows of excl, 2 group G + slot Tk), whether any term or flag can kill a row, and
// where the caller wants `which` (null: not asked for).
struct TermsQuery { const float* q; int n_vec; const int64_t* rows; int n_rows; TermSpec spec; LikeRows excl; int mode, G, Tk; bool kills; int32_t* which; };

// The query side of cc_index_rank_like, checked by its own rules, as the compound question it is: no vector, every row a RANK term of
// weight 1 under MAX, the exclude bits as they are, no `which`.
int like_check(cc_index* h, const int64_t* rows, int n_rows, int flags, TermsQuery* tq) {
  CC_API_BEGIN
  CC_CHECK(h && rows, "null argument");
  CC_CHECK(n_rows >= 1 && n_rows <= CC_LIKE_MAX_ROWS, "n_rows must be in [1, CC_LIKE_MAX_ROWS]");
  CC_CHECK((flags & ~(CC_RANK_TRACKS | CC_LIKE_EXCLUDE_ROWS | CC_LIKE_EXCLUDE_TRACK)) == 0, "unknown flag bits");
  check_rows(h, rows, n_rows);
  *tq = TermsQuery{};
  tq->rows = rows; tq->n_rows = n_rows;
  tq->spec.T = n_rows; tq->spec.combine = CC_COMBINE_MAX;
  for (int t = 0; t < n_rows; ++t) tq->spec.t[t] = TermParam{1.f, 0.f, CC_TERM_RANK, 0};
  tq->excl = like_rows(rows, n_rows);                // n < 2^31 (checked by rank())
  tq->mode = (flags & CC_LIKE_EXCLUDE_TRACK) ? 2 : (flags & CC_LIKE_EXCLUDE_ROWS) ? 1 : 0;
  tq->G = 0; tq->Tk = -1;
  tq->kills = tq->mode != 0;
  if (tq->mode == 2) {
    CC_CHECK(h->grp_host.size() == (size_t)h->n && h->trk_host.size() == (size_t)h->n, "the host columns are out of step with the index");
    tq->G = h->grp_host[(size_t)rows[0]]; tq->Tk = h->trk_host[(size_t)rows[0]];
    CC_CHECK(tq->Tk >= 0, "CC_LIKE_EXCLUDE_TRACK needs query rows with a track slot");
    for (int i = 1; i < n_rows; ++i)
      CC_CHECK(h->grp_host[(size_t)rows[i]] == tq->G && h->trk_host[(size_t)rows[i]] == tq->Tk, "CC_LIKE_EXCLUDE_TRACK needs query rows of one group and one track slot");
  }
  CC_API_END
}

int terms_check(cc_index* h, const float* q, int n_vec, const int64_t* rows, int n_rows, const cc_term* terms, int combine, int flags, int32_t* which,
                TermsQuery* tq) {
  CC_API_BEGIN
  CC_CHECK(h && terms, "null argument");
  CC_CHECK(n_vec >= 0 && n_rows >= 0 && n_vec <= CC_TERMS_MAX && n_rows <= CC_TERMS_MAX && n_vec + n_rows >= 1 && n_vec + n_rows <= CC_TERMS_MAX,
           "n_vec and n_rows must not be negative and n_vec + n_rows must be in [1, CC_TERMS_MAX]");
  CC_CHECK((q || !n_vec) && (rows || !n_rows), "null argument");
  CC_CHECK(combine == CC_COMBINE_MAX || combine == CC_COMBINE_MIN || combine == CC_COMBINE_SUM, "unknown combine rule");
  CC_CHECK((flags & ~(CC_RANK_TRACKS | CC_LIKE_EXCLUDE_ROWS | CC_LIKE_EXCLUDE_TRACK)) == 0, "unknown flag bits");
  check_rows(h, rows, n_rows);
  const int T = n_vec + n_rows;
  *tq = TermsQuery{};
  tq->q = q; tq->n_vec = n_vec; tq->rows = rows; tq->n_rows = n_rows; tq->which = which;
  tq->spec.T = T; tq->spec.combine = combine;
  tq->mode = (flags & CC_LIKE_EXCLUDE_TRACK) ? 2 : (flags & CC_LIKE_EXCLUDE_ROWS) ? 1 : 0;
  tq->G = 0; tq->Tk = -1;
  for (int i = 0; i < CC_LIKE_MAX_ROWS; ++i) tq->excl.r[i] = -1;
  int n_rank = 0;
  for (int t = 0; t < T; ++t) {
    const cc_term& m = terms[t];
    CC_CHECK(m.role == CC_TERM_RANK || m.role == CC_TERM_REQUIRE || m.role == CC_TERM_REJECT, "unknown term role");
    tq->spec.t[t] = TermParam{m.weight, m.cut, m.role, 0};
    if (m.role == CC_TERM_RANK) {
      ++n_rank;
      CC_CHECK(combine != CC_COMBINE_SUM || (m.weight - m.weight == 0.f), "the weight of a RANK term must be finite under CC_COMBINE_SUM");
      if (t >= n_vec) tq->excl.r[tq->excl.n++] = (int)std::min<int64_t>(rows[t - n_vec], INT32_MAX);   // n < 2^31 is checked by rank() / timeline()
    } else {
      CC_CHECK(m.cut == m.cut, "the cut of a REQUIRE / REJECT term is NaN");
      tq->kills = true;
    }
  }
  CC_CHECK(n_rank >= 1, "no RANK term");
  if (tq->mode) {
    CC_CHECK(tq->excl.n >= 1, "an exclude bit needs a stored row that is a RANK term");
    tq->kills = true;
  }
  if (tq->mode == 2) {
    CC_CHECK(h->grp_host.size() == (size_t)h->n && h->trk_host.size() == (size_t)h->n, "the host columns are out of step with the index");
    tq->G = h->grp_host[(size_t)tq->excl.r[0]]; tq->Tk = h->trk_host[(size_t)tq->excl.r[0]];
    CC_CHECK(tq->Tk >= 0, "CC_LIKE_EXCLUDE_TRACK needs RANK rows with a track slot");
    for (int i = 1; i < tq->excl.n; ++i)
      CC_CHECK(h->grp_host[(size_t)tq->excl.r[i]] == tq->G && h->trk_host[(size_t)tq->excl.r[i]] == tq->Tk, "CC_LIKE_EXCLUDE_TRACK needs RANK rows of one group and one track slot");
  }
  CC_API_END
}

// What cc_index_rank_terms and cc_index_rank_like run where cc_index_rank_where uploads and scores its queries: the vectors copied and
// the rows gathered into ONE batch of T queries, scored by the route of that batch, folded.  Leaves v in row 0 of h->scores, w.dead set
// when a term or a flag can kill a row, and h->which_row written when `which` is asked for.  One RANK term under MAX / MIN and nothing
// else: no fold.
void terms_scores(cc_index* h, const TermsQuery& tq, RowWhere& w, int on_device, hipStream_t s) {
  const long n = (long)h->n;
  const int T = tq.spec.T;
  ensure_queries(h, T);
  if (tq.n_vec) upload_queries(h, tq.q, tq.n_vec, on_device, s);
  if (tq.n_rows) gather_rows(h, tq.rows, tq.n_rows, h->q_dev + (size_t)tq.n_vec * h->dim, s);
  compute_scores(h, T, s);
  if (T == 1 && tq.spec.combine != CC_COMBINE_SUM && !tq.kills && !tq.which) return;
  unsigned char *dead = nullptr, *which = nullptr;
  if (tq.kills) { ensure((void**)&h->dead, &h->dead_cap, (size_t)n); w.dead = dead = h->dead; }
  if (tq.which) { ensure((void**)&h->which_row, &h->which_row_cap, (size_t)n); which = h->which_row; }
  if (n % 4 == 0)
    hipLaunchKernelGGL(terms_fold_kernel<true>, dim3((unsigned)std::min<long>((n / 4 + 255) / 256, 256 * 8)), dim3(256), 0, s, h->scores, n, h->grp, h->trk, tq.spec,
                       tq.excl, tq.mode, tq.G, tq.Tk, dead, which);
  else
    hipLaunchKernelGGL(terms_fold_kernel<false>, dim3((unsigned)std::min<long>((n + 255) / 256, 256 * 8)), dim3(256), 0, s, h->scores, n, h->grp, h->trk, tq.spec,
                       tq.excl, tq.mode, tq.G, tq.Tk, dead, which);
  CC_HIP(hipGetLastError());
}

// The selection of rank() over the keys in h->key_hi (Q, n): per batch of up to 16 windows of kMaxK answers init, eight times (histogram,
// pick), collect, emit into idx_out / sc_out (Q, count).  sel / ghist / wcnt: the selects, bin tables and window counters of one batch
// (kRankSel per query).  avail: the answers from `start` on that are not padding whatever the scores are.
void rank_select(cc_index* h, int Q, bool tracks, int64_t start, int64_t avail, int64_t count, RankSel* sel, unsigned* ghist, unsigned* wcnt,
                 int* idx_out, float* sc_out, hipStream_t s) {
  const long n = (long)h->n;
  const unsigned nblk = (unsigned)((n + kRankRows - 1) / kRankRows);
  const int T = std::max(h->n_slots, 1);
  const int* trk = tracks ? h->trk : nullptr;
  const int64_t nwin = (avail + kMaxK - 1) / kMaxK;
  if (nwin) ensure((void**)&h->cand, &h->cand_cap, (size_t)Q * kRankSel * kMaxK * 8);
  for (int64_t w0 = 0; w0 < nwin; w0 += kRankSel - 1) {
    const int nw = (int)std::min<int64_t>(kRankSel - 1, nwin - w0), S = nw + 1;
    const long r0 = (long)(start + w0 * kMaxK), r_last = (long)(start + std::min<int64_t>(avail, (w0 + nw) * kMaxK));
    hipLaunchKernelGGL(rank_init_kernel, dim3(Q), dim3(256), 0, s, r0, r_last, sel, ghist, wcnt);
    for (int byte = 7; byte >= 0; --byte) {
      hipLaunchKernelGGL(rank_hist_kernel, dim3(nblk, S, Q), dim3(256), 0, s, h->key_hi, n, trk, byte, sel, ghist);
      hipLaunchKernelGGL(rank_pick_kernel, dim3(S, Q), dim3(64), 0, s, byte, sel, ghist);
    }
    hipLaunchKernelGGL(rank_collect_kernel, dim3(nblk, Q), dim3(256), 0, s, h->key_hi, n, trk, S, r0 == 0 ? 1 : 0, sel, wcnt, h->cand);
    if (tracks) hipLaunchKernelGGL(rank_emit_kernel<true>, dim3(nw, Q), dim3(1024), 0, s, h->cand, wcnt, (long)(w0 * kMaxK), (long)count, idx_out, sc_out, n, h->trk, h->best, T);
    else hipLaunchKernelGGL(rank_emit_kernel<false>, dim3(nw, Q), dim3(1024), 0, s, h->cand, wcnt, (long)(w0 * kMaxK), (long)count, idx_out, sc_out, n, nullptr, nullptr, 0);
  }
}

// The query side of cc_index_rank_near / cc_index_timeline_near, checked: the two sides (a vector, or a stored row beside a null vector),
// the join, B's filter as the kernels take it (rows with a ts only), and where the caller wants the partners and the list's full length.
struct NearQuery { const float* qa; int64_t row_a; const float* qb; int64_t row_b; int within, cap, value; float cut_b; RowWhere wb;
                   int32_t* partner; float* partner_score; int64_t* n_partners; };

int near_check(cc_index* h, const float* qa, int64_t row_a, const float* qb, int64_t row_b, int32_t within, int max_partners, float cut_b, int value, int flags,
               const cc_row_filter* where_b, int32_t* partner, float* partner_score, int64_t* n_partners, NearQuery* nq) {
  CC_API_BEGIN
  CC_CHECK(h, "null argument");
  CC_CHECK((qa != nullptr) != (row_a >= 0) && (qb != nullptr) != (row_b >= 0), "each side needs exactly one of a vector and a stored row");
  CC_CHECK((qa || row_a < h->n) && (qb || row_b < h->n), "a row number outside the index");
  CC_CHECK(within >= 0, "within must not be negative");
  CC_CHECK(max_partners >= 1 && max_partners <= CC_NEAR_MAX_PARTNERS, "max_partners must be in [1, CC_NEAR_MAX_PARTNERS]");
  CC_CHECK(cut_b == cut_b, "cut_b is NaN");
  CC_CHECK(value == CC_NEAR_VALUE_A || value == CC_NEAR_VALUE_MIN, "unknown value rule");
  CC_CHECK((flags & ~CC_RANK_TRACKS) == 0, "unknown flag bits");
  *nq = NearQuery{qa, row_a, qb, row_b, within, max_partners, value, cut_b, make_where(h, where_b), partner, partner_score, n_partners};
  if (!nq->wb.ts) { nq->wb.ts = h->ts; nq->wb.ts_min = INT32_MIN; nq->wb.ts_max = INT32_MAX; }   // no window: still only rows that have a ts
  CC_API_END
}

// The scratch of a together call that is its own (h->near_ws): the list, the state of its selection, its total.
struct NearWs { NearList L; RankSel* sel; unsigned* ghist; unsigned* wcnt; unsigned* total; };

NearWs near_ws(cc_index* h) {
  const size_t list_bytes = near_list_bytes(), sel_bytes = (kRankSel * sizeof(RankSel) + 255) & ~(size_t)255, hist_bytes = (size_t)kRankSel * 256 * 4,
               cnt_bytes = (size_t)kRankSel * 4;
  ensure((void**)&h->near_ws, &h->near_ws_cap, list_bytes + sel_bytes + hist_bytes + cnt_bytes + 4);
  NearWs ws;
  ws.L = near_list(h->near_ws);
  ws.sel = reinterpret_cast<RankSel*>(h->near_ws + list_bytes);
  ws.ghist = reinterpret_cast<unsigned*>(h->near_ws + list_bytes + sel_bytes);
  ws.wcnt = reinterpret_cast<unsigned*>(h->near_ws + list_bytes + sel_bytes + hist_bytes);
  ws.total = reinterpret_cast<unsigned*>(h->near_ws + list_bytes + sel_bytes + hist_bytes + cnt_bytes);
  return ws;
}

// What cc_index_rank_near runs where cc_index_rank_where uploads and scores its queries: both sides where queries stand, ONE scoring
// call, the ungrouped selection of cc_index_rank_where on B's score row (cut_b, B's filter, rows with a ts) into the list, the pack and
// the fold.  Leaves v in row 0 of h->scores, w.dead set, h->near_pos written and the list's full length in ws.total (cleared by the
// caller).  w comes in as A's filter without dead bytes; min_score / tracks: what the ranking behind will cut and reduce by.  n > 0.
void near_scores(cc_index* h, const NearQuery& nq, RowWhere& w, bool tracks, float min_score, const unsigned char* allowed_dev, int on_device, hipStream_t s) {
  const long n = (long)h->n;
  const NearWs ws = near_ws(h);
  ensure_queries(h, 2);
  const float* vec[2] = {nq.qa, nq.qb};
  const int64_t row[2] = {nq.row_a, nq.row_b};
  const size_t qb = (size_t)h->dim * 4;
  for (int i = 0; i < 2; ++i) {
    float* dst = h->q_dev + (size_t)i * h->dim;
    if (!vec[i]) gather_rows(h, &row[i], 1, dst, s);              // one number: it travels in the kernel arguments
    else if (on_device) CC_HIP(hipMemcpyAsync(dst, vec[i], qb, hipMemcpyDeviceToDevice, s));
    else {                                                        // through the pinned block, as upload_queries does
      memcpy(h->pin + i * qb, vec[i], qb);
      CC_HIP(hipMemcpyAsync(dst, h->pin + i * qb, qb, hipMemcpyHostToDevice, s));
    }
  }
  compute_scores(h, 2, s);
  ensure((void**)&h->key_hi, &h->key_hi_cap, (size_t)n * 4);
  hipLaunchKernelGGL(rank_keys_kernel<false>, dim3((unsigned)((n + kRankRows - 1) / kRankRows), 1), dim3(256), 0, s, h->scores + n, n, h->grp, allowed_dev,
                     h->allowed_cap, nullptr, nullptr, nullptr, 0, nq.cut_b, nq.wb, h->key_hi, ws.total);
  const int64_t avail = std::min<int64_t>(nq.cap, n);
  if (avail < nq.cap) hipLaunchKernelGGL(rank_pad_kernel, dim3((unsigned)((nq.cap + 255) / 256)), dim3(256), 0, s, ws.L.row, ws.L.score, (size_t)nq.cap);
  rank_select(h, 1, false, 0, avail, nq.cap, ws.sel, ws.ghist, ws.wcnt, ws.L.row, ws.L.score, s);
  CC_HIP(hipGetLastError());
  launch_near_pack(ws.L, nq.cap, n, h->grp, h->ts, h->trk, s);
  ensure((void**)&h->dead, &h->dead_cap, (size_t)n);
  ensure((void**)&h->near_pos, &h->near_pos_cap, (size_t)n * 4);
  launch_near_fold(h->scores, n, h->grp, h->trk, h->ts, allowed_dev, h->allowed_cap, w, min_score, tracks ? 0 : 1, ws.L, ws.total, nq.cap, nq.within, nq.value,
                   h->dead, h->near_pos, s);
  w.dead = h->dead;
}

// Where the ONE score vector of a ranking comes from when it is not a caller's query: the fold of a cc_index_rank_like / cc_index_rank_terms /
// cc_index_timeline_terms or the join of a cc_index_rank_near / cc_index_timeline_near.  Exactly one of the two is set.
struct FoldQuery { const TermsQuery* terms; const NearQuery* near; };

void fold_scores(cc_index* h, const FoldQuery& f, RowWhere& w, bool tracks, float min_score, const unsigned char* allowed_dev, int on_device, hipStream_t s) {
  if (f.terms) terms_scores(h, *f.terms, w, on_device, s);
  else near_scores(h, *f.near, w, tracks, min_score, allowed_dev, on_device, s);
}

// What rank() and timeline() share around their own selection.  rank_begin: the call as checked - the stream, the row filter, whether
// tracks answer, the together question behind a fold, and qbytes, the head of the pinned block that the queries go through.  The caller
// sizes the pinned block and its scratch behind that and says where the totals stand (tot_host, tot_dev).
struct RankCall {
  bool tracks; RowWhere w; hipStream_t s; long n; const NearQuery* near; size_t qbytes;
  NearWs nws;                                     // a together call: its own scratch, whose total rank_scores clears
  unsigned* tot_host; unsigned* tot_dev;          // (Q) the totals, and on the host behind them the full length of a together call's list
};

RankCall rank_begin(cc_index* h, const float* q, int Q, float min_score, int flags, const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                    bool outputs, void* stream, const FoldQuery* fold) {
  CC_CHECK(h && (q || fold) && outputs, "null argument");
  CC_CHECK(Q >= 1 && Q <= 65535, "Q must be in [1, 65535]");
  CC_CHECK(min_score == min_score, "min_score is NaN");
  CC_CHECK((flags & ~CC_RANK_TRACKS) == 0, "unknown flag bits");
  CC_CHECK(!allowed || (n_groups > 0 && n_groups <= (1 << 24)), "bad group count");
  CC_CHECK(h->n < (1LL << 31), "ranking needs fewer than 2^31 rows");       // keys hold ~row and ~(n + row) in 32 bits
  RankCall c{};
  c.tracks = (flags & CC_RANK_TRACKS) != 0;
  c.w = make_where(h, where);
  CC_HIP(hipSetDevice(h->device));
  c.s = stream ? (hipStream_t)stream : h->stream;
  c.n = (long)h->n;
  c.near = fold ? fold->near : nullptr;
  const int nq = c.near ? 2 : fold && fold->terms ? std::max(fold->terms->n_vec, 1) : Q;  // the queries that go through the pinned block
  c.qbytes = ((size_t)nq * h->dim * 4 + 255) & ~(size_t)255;
  return c;
}

// The ONE score vector per query and its keys: the together scratch total cleared, then (n > 0) the group filter, the scores - a
// fold's, or the caller's queries uploaded and scored -, (track reduction,) keys + totals.
void rank_scores(cc_index* h, RankCall& c, const float* q, int Q, float min_score, const uint8_t* allowed, int n_groups, int on_device, const FoldQuery* fold) {
  if (c.near) { c.nws = near_ws(h); CC_HIP(hipMemsetAsync(c.nws.total, 0, 4, c.s)); }
  if (c.n <= 0) return;
  const unsigned char* allowed_dev = upload_allowed(h, allowed, n_groups, c.s);
  if (fold) fold_scores(h, *fold, c.w, c.tracks, min_score, allowed_dev, on_device, c.s);
  else {
    upload_queries(h, q, Q, on_device, c.s);
    compute_scores(h, Q, c.s);
  }
  rank_keys(h, Q, c.tracks, min_score, allowed_dev, c.w, c.tot_dev, c.s);
}

// Behind everything a call has put on the stream: the totals (and a together call's list length) to the host, when asked for.  A host
// caller waits for the stream whatever it asked for: its results come by the same stream.
void rank_totals(const RankCall& c, int Q, int64_t* total, int on_device) {
  if (total) CC_HIP(hipMemcpyAsync(c.tot_host, c.tot_dev, (size_t)Q * 4, hipMemcpyDeviceToHost, c.s));
  const bool want_np = c.near && c.near->n_partners;
  if (want_np) CC_HIP(hipMemcpyAsync(c.tot_host + Q, c.nws.total, 4, hipMemcpyDeviceToHost, c.s));
  if (!on_device || total || want_np) CC_HIP(hipStreamSynchronize(c.s));
  if (total) for (int i = 0; i < Q; ++i) total[i] = (int64_t)c.tot_host[i];
  if (want_np) *c.near->n_partners = (int64_t)c.tot_host[Q];
}

// cc_index_rank / cc_index_rank_where.  Launches on one stream: scan, (track reduction,) keys + totals, then per batch of up to 16 windows of kMaxK answers:
// init, eight times (histogram, pick), collect, emit.  Answers past the last row the index could give are padded by one fill.
// fold (cc_index_rank_like, cc_index_rank_terms; Q is 1 and q unused): the score vector comes from fold_scores instead, everything behind
// it is the same; a cc_index_rank_terms that asks for `which` adds one gather of `count` entries behind the last emit, and so does a
// cc_index_rank_near for its partners.
int rank(cc_index* h, const float* q, int Q, int64_t start, int64_t count, float min_score, int flags, const uint8_t* allowed, int n_groups,
         const cc_row_filter* where, int32_t* idx, float* score, int64_t* total, int on_device, void* stream, const FoldQuery* fold = nullptr) {
  CC_API_BEGIN
  RankCall c = rank_begin(h, q, Q, min_score, flags, allowed, n_groups, where, idx && score, stream, fold);
  CC_CHECK(start >= 0, "start must not be negative");
  CC_CHECK(count >= 1 && count <= (1LL << 40) / Q, "count must be positive (and Q * count below 2^40)");
  const hipStream_t s = c.s;
  const long n = c.n;
  const NearQuery* near = c.near;
  const size_t qbytes = c.qbytes, ob = (size_t)Q * (size_t)count;
  int32_t* which = fold && fold->terms ? fold->terms->which : nullptr;
  const bool zero_copy = !on_device && ob * 8 <= kPinResultBytes;            // small host results: written into pinned memory, as search() does
  // idx, score and, asked for, `which` in a slot of its own; a together call: partner and partner_score in two slots behind score
  const size_t res_bytes = zero_copy ? (ob * (near ? 16 : which ? 12 : 8) + 255) & ~(size_t)255 : 0;
  ensure_pinned(h, qbytes + res_bytes + (size_t)(Q + (near ? 1 : 0)) * 4);   // the totals, and behind them the full length of a together call's list
  c.tot_host = reinterpret_cast<unsigned*>(h->pin + qbytes + res_bytes);
  int* idx_out = idx; float* sc_out = score;
  int* which_out = which;
  int* partner_out = near ? near->partner : nullptr; float* pscore_out = near ? near->partner_score : nullptr;
  const bool want_partner = partner_out || pscore_out;
  if (zero_copy) {
    idx_out = reinterpret_cast<int*>(h->pin + qbytes); sc_out = reinterpret_cast<float*>(h->pin + qbytes + ob * 4); which_out = reinterpret_cast<int*>(h->pin + qbytes + ob * 8);
    if (want_partner) { partner_out = reinterpret_cast<int*>(h->pin + qbytes + ob * 8); pscore_out = reinterpret_cast<float*>(h->pin + qbytes + ob * 12); }
  } else if (!on_device) {
    if (which) { ensure((void**)&h->which_dev, &h->which_dev_cap, ob * 4); which_out = h->which_dev; }
    if (want_partner) { ensure((void**)&h->near_dev, &h->near_dev_cap, ob * 8); partner_out = h->near_dev; pscore_out = reinterpret_cast<float*>(h->near_dev + ob); }
    ensure_out(h, ob);
    idx_out = h->idx_dev; sc_out = h->sc_dev;
  }
  const size_t sel_bytes = (size_t)Q * kRankSel * sizeof(RankSel), hist_bytes = (size_t)Q * kRankSel * 256 * 4, cnt_bytes = (size_t)Q * kRankSel * 4;
  ensure((void**)&h->rank_ws, &h->rank_ws_cap, sel_bytes + hist_bytes + cnt_bytes + (size_t)Q * 4);
  RankSel* sel = reinterpret_cast<RankSel*>(h->rank_ws);
  unsigned* ghist = reinterpret_cast<unsigned*>(h->rank_ws + sel_bytes);
  unsigned* wcnt = reinterpret_cast<unsigned*>(h->rank_ws + sel_bytes + hist_bytes);
  c.tot_dev = reinterpret_cast<unsigned*>(h->rank_ws + sel_bytes + hist_bytes + cnt_bytes);
  CC_HIP(hipMemsetAsync(c.tot_dev, 0, (size_t)Q * 4, s));
  // answers the index can give from `start` on: at most one per row.  What lies behind them is padding whatever the scores are.
  const int64_t avail = std::max<int64_t>(0, std::min<int64_t>(count, (int64_t)n - start));
  if (avail < count)
    hipLaunchKernelGGL(rank_pad_kernel, dim3((unsigned)std::min<size_t>((ob + 255) / 256, 4096)), dim3(256), 0, s, idx_out, sc_out, ob);
  rank_scores(h, c, q, Q, min_score, allowed, n_groups, on_device, fold);
  if (n > 0) rank_select(h, Q, c.tracks, start, avail, count, sel, ghist, wcnt, idx_out, sc_out, s);
  if (which)   // every entry of idx is written by now (an emit or the padding): one term byte per answer, -1 behind the last one
    hipLaunchKernelGGL(which_gather_kernel, dim3((unsigned)std::min<size_t>((ob + 255) / 256, 4096)), dim3(256), 0, s, idx_out, h->which_row, n, ob, which_out);
  CC_HIP(hipGetLastError());
  if (want_partner)   // the same for a together call: the partner of the row each answer names, from the fold's places (an empty index: all padding)
    launch_near_gather(idx_out, h->near_pos, c.nws.L, n, ob, near->cap, partner_out, pscore_out, s);
  if (!on_device && !zero_copy) {
    CC_HIP(hipMemcpyAsync(idx, h->idx_dev, ob * 4, hipMemcpyDeviceToHost, s));
    CC_HIP(hipMemcpyAsync(score, h->sc_dev, ob * 4, hipMemcpyDeviceToHost, s));
    if (which) CC_HIP(hipMemcpyAsync(which, h->which_dev, ob * 4, hipMemcpyDeviceToHost, s));
    if (near && near->partner) CC_HIP(hipMemcpyAsync(near->partner, partner_out, ob * 4, hipMemcpyDeviceToHost, s));
    if (near && near->partner_score) CC_HIP(hipMemcpyAsync(near->partner_score, pscore_out, ob * 4, hipMemcpyDeviceToHost, s));
  }
  rank_totals(c, Q, total, on_device);
  if (zero_copy) {
    memcpy(idx, idx_out, ob * 4); memcpy(score, sc_out, ob * 4); if (which) memcpy(which, which_out, ob * 4);
    if (near && near->partner) memcpy(near->partner, partner_out, ob * 4);
    if (near && near->partner_score) memcpy(near->partner_score, pscore_out, ob * 4);
  }
  CC_API_END
}

// cc_index_timeline.  Launches on one stream: scan, (track reduction,) keys + totals as in rank(), then the histogram kernel.
// fold (cc_index_timeline_terms; Q is 1 and q unused): the score vector comes from fold_scores, as in rank().
int timeline(cc_index* h, const float* q, int Q, float min_score, int flags, const uint8_t* allowed, int n_groups, const cc_row_filter* where,
             int32_t t0, int32_t bin_seconds, int n_bins, uint32_t* counts, int64_t* total, int on_device, void* stream, const FoldQuery* fold = nullptr) {
  CC_API_BEGIN
  RankCall c = rank_begin(h, q, Q, min_score, flags, allowed, n_groups, where, counts != nullptr, stream, fold);
  CC_CHECK(bin_seconds >= 1, "bin_seconds must be at least 1");
  CC_CHECK(n_bins >= 1 && n_bins <= 4096, "n_bins must be in [1, 4096]");
  const hipStream_t s = c.s;
  const long n = c.n;
  const size_t cbytes = (size_t)Q * n_bins * 4;
  ensure_pinned(h, c.qbytes + (size_t)(Q + (c.near ? 1 : 0)) * 4);           // the totals, and behind them the full length of a together call's list
  c.tot_host = reinterpret_cast<unsigned*>(h->pin + c.qbytes);
  ensure((void**)&h->rank_ws, &h->rank_ws_cap, (size_t)Q * 4 + cbytes);     // per query the total, then (host caller) the bins
  c.tot_dev = reinterpret_cast<unsigned*>(h->rank_ws);
  unsigned* cnt_dev = on_device ? counts : c.tot_dev + Q;
  CC_HIP(hipMemsetAsync(c.tot_dev, 0, (size_t)Q * 4, s));
  CC_HIP(hipMemsetAsync(cnt_dev, 0, cbytes, s));
  rank_scores(h, c, q, Q, min_score, allowed, n_groups, on_device, fold);
  if (n > 0) {
    const dim3 grid((unsigned)((n + kRankRows - 1) / kRankRows), Q);
    const size_t lds = (size_t)n_bins * 4;
    if (c.tracks) hipLaunchKernelGGL(timeline_kernel<true>, grid, dim3(256), lds, s, h->key_hi, n, h->trk, h->best, std::max(h->n_slots, 1), h->ts,
                                     (long long)t0, (unsigned)bin_seconds, n_bins, cnt_dev);
    else hipLaunchKernelGGL(timeline_kernel<false>, grid, dim3(256), lds, s, h->key_hi, n, nullptr, nullptr, 0, h->ts,
                            (long long)t0, (unsigned)bin_seconds, n_bins, cnt_dev);
  }
  CC_HIP(hipGetLastError());
  if (!on_device) CC_HIP(hipMemcpyAsync(counts, cnt_dev, cbytes, hipMemcpyDeviceToHost, s));
  rank_totals(c, Q, total, on_device);
  CC_API_END
}

}  // namespace

extern "C" {

int cc_index_search_groups(cc_index* h, const float* q, int Q, int k, const uint8_t* allowed, int n_groups, int32_t* idx, float* score,
                           int on_device, void* stream) {
  return search(h, q, Q, k, allowed, n_groups, idx, score, on_device, stream, false);
}

int cc_index_search_tracks(cc_index* h, const float* q, int Q, int k, const uint8_t* allowed, int n_groups, int32_t* idx, float* score,
                           int on_device, void* stream) {
  return search(h, q, Q, k, allowed, n_groups, idx, score, on_device, stream, true);
}

int cc_index_search(cc_index* h, const float* q, int Q, int k, int32_t* idx, float* score, int on_device, void* stream) {
  return cc_index_search_groups(h, q, Q, k, nullptr, 0, idx, score, on_device, stream);
}

int cc_index_rank(cc_index* h, const float* q, int Q, int64_t start, int64_t count, float min_score, int flags, const uint8_t* allowed, int n_groups,
                  int32_t* idx, float* score, int64_t* total, int on_device, void* stream) {
  return rank(h, q, Q, start, count, min_score, flags, allowed, n_groups, nullptr, idx, score, total, on_device, stream);
}

int cc_index_rank_where(cc_index* h, const float* q, int Q, int64_t start, int64_t count, float min_score, int flags, const uint8_t* allowed, int n_groups,
                        const cc_row_filter* where, int32_t* idx, float* score, int64_t* total, int on_device, void* stream) {
  return rank(h, q, Q, start, count, min_score, flags, allowed, n_groups, where, idx, score, total, on_device, stream);
}

int cc_index_timeline(cc_index* h, const float* q, int Q, float min_score, int flags, const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                      int32_t t0, int32_t bin_seconds, int n_bins, uint32_t* counts, int64_t* total, int on_device, void* stream) {
  return timeline(h, q, Q, min_score, flags, allowed, n_groups, where, t0, bin_seconds, n_bins, counts, total, on_device, stream);
}

int cc_index_fetch_rows(cc_index* h, const int64_t* rows, int n, float* out, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && rows && out, "null argument");
  CC_CHECK(n >= 1 && n <= 65535, "n must be in [1, 65535]");
  check_rows(h, rows, n);
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (on_device) gather_rows(h, rows, n, out, s);
  else {                                             // a host caller: gathered where queries stand, then one copy down
    ensure_queries(h, n);
    gather_rows(h, rows, n, h->q_dev, s);
    CC_HIP(hipMemcpyAsync(out, h->q_dev, (size_t)n * h->dim * 4, hipMemcpyDeviceToHost, s));
    CC_HIP(hipStreamSynchronize(s));
  }
  CC_API_END
}

int cc_index_rank_like(cc_index* h, const int64_t* rows, int n_rows, int64_t start, int64_t count, float min_score, int flags,
                       const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                       int32_t* idx, float* score, int64_t* total, int on_device, void* stream) {
  TermsQuery tq{};
  if (const int rc = like_check(h, rows, n_rows, flags, &tq)) return rc;
  const FoldQuery fold{&tq, nullptr};
  return rank(h, nullptr, 1, start, count, min_score, flags & CC_RANK_TRACKS, allowed, n_groups, where, idx, score, total, on_device, stream, &fold);
}

int cc_index_rank_terms(cc_index* h, const float* q, int n_vec, const int64_t* rows, int n_rows, const cc_term* terms, int combine,
                        int64_t start, int64_t count, float min_score, int flags, const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                        int32_t* idx, float* score, int32_t* which, int64_t* total, int on_device, void* stream) {
  TermsQuery tq{};
  if (const int rc = terms_check(h, q, n_vec, rows, n_rows, terms, combine, flags, which, &tq)) return rc;
  const FoldQuery fold{&tq, nullptr};
  return rank(h, nullptr, 1, start, count, min_score, flags & CC_RANK_TRACKS, allowed, n_groups, where, idx, score, total, on_device, stream, &fold);
}

int cc_index_timeline_terms(cc_index* h, const float* q, int n_vec, const int64_t* rows, int n_rows, const cc_term* terms, int combine, float min_score, int flags,
                            const uint8_t* allowed, int n_groups, const cc_row_filter* where, int32_t t0, int32_t bin_seconds, int n_bins,
                            uint32_t* counts, int64_t* total, int on_device, void* stream) {
  TermsQuery tq{};
  if (const int rc = terms_check(h, q, n_vec, rows, n_rows, terms, combine, flags, nullptr, &tq)) return rc;
  const FoldQuery fold{&tq, nullptr};
  return timeline(h, nullptr, 1, min_score, flags & CC_RANK_TRACKS, allowed, n_groups, where, t0, bin_seconds, n_bins, counts, total, on_device, stream, &fold);
}

// Together: the kernels that are new are index_near.hip's (its head tells how they fit together); the checks of the two sides and the join stand
// in near_check, everything else is rank() / timeline() with the join as the fold.
int cc_index_rank_near(cc_index* h, const float* qa, int64_t row_a, const float* qb, int64_t row_b, int32_t within, int max_partners, float cut_b, int value,
                       int64_t start, int64_t count, float min_score, int flags, const uint8_t* allowed, int n_groups, const cc_row_filter* where_a,
                       const cc_row_filter* where_b, int32_t* idx, float* score, int32_t* partner, float* partner_score, int64_t* total, int64_t* n_partners,
                       int on_device, void* stream) {
  NearQuery nq{};
  if (const int rc = near_check(h, qa, row_a, qb, row_b, within, max_partners, cut_b, value, flags, where_b, partner, partner_score, n_partners, &nq)) return rc;
  const FoldQuery fold{nullptr, &nq};
  return rank(h, nullptr, 1, start, count, min_score, flags, allowed, n_groups, where_a, idx, score, total, on_device, stream, &fold);
}

int cc_index_timeline_near(cc_index* h, const float* qa, int64_t row_a, const float* qb, int64_t row_b, int32_t within, int max_partners, float cut_b, int value,
                           float min_score, int flags, const uint8_t* allowed, int n_groups, const cc_row_filter* where_a, const cc_row_filter* where_b,
                           int32_t t0, int32_t bin_seconds, int n_bins, uint32_t* counts, int64_t* total, int64_t* n_partners, int on_device, void* stream) {
  NearQuery nq{};
  if (const int rc = near_check(h, qa, row_a, qb, row_b, within, max_partners, cut_b, value, flags, where_b, nullptr, nullptr, n_partners, &nq)) return rc;
  const FoldQuery fold{nullptr, &nq};
  return timeline(h, nullptr, 1, min_score, flags, allowed, n_groups, where_a, t0, bin_seconds, n_bins, counts, total, on_device, stream, &fold);
}

// Distinct ranking: the kernels are index_distinct.hip's (its head tells how they fit together); here the checks, the scratch and the copies.
int cc_index_gram(cc_index* h, const int64_t* rows, int n, float* out, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && rows && out, "null argument");
  CC_CHECK(n >= 1 && n <= CC_DISTINCT_MAX_DEPTH, "n must be in [1, CC_DISTINCT_MAX_DEPTH]");
  check_rows(h, rows, n);
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  float* dst = out;
  if (!on_device) { ensure((void**)&h->dist_io, &h->dist_io_cap, (size_t)n * n * 4); dst = reinterpret_cast<float*>(h->dist_io); }
  pin_rows(h, rows, n);
  launch_index_gram(h->emb, (long)h->n, h->dim, h->storage, (const long long*)h->rows_pin, n, dst, s);
  CC_HIP(hipEventRecord(h->rows_ev, s));
  if (!on_device) {
    CC_HIP(hipMemcpyAsync(out, dst, (size_t)n * n * 4, hipMemcpyDeviceToHost, s));
    CC_HIP(hipStreamSynchronize(s));
  }
  CC_API_END
}

int cc_index_distinct(cc_index* h, const int32_t* idx, const float* score, int Q, int depth, float same_at, int64_t start, int64_t count,
                      int32_t* out_idx, float* out_score, int32_t* out_dups, int64_t* total, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && idx && out_idx && (out_score || !score), "null argument");
  CC_CHECK(same_at == same_at, "same_at is NaN");
  CC_CHECK(depth >= 1 && depth <= CC_DISTINCT_MAX_DEPTH, "depth must be in [1, CC_DISTINCT_MAX_DEPTH]");
  CC_CHECK(Q >= 1 && Q <= CC_DISTINCT_MAX_Q, "Q must be in [1, CC_DISTINCT_MAX_Q]");
  CC_CHECK(start >= 0, "start must not be negative");
  CC_CHECK(count >= 1 && count <= (1LL << 40) / Q, "count must be positive (and Q * count below 2^40)");
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  ensure((void**)&h->dist_ws, &h->dist_ws_cap, distinct_ws_bytes(Q));
  const DistinctWs ws = distinct_ws(h->dist_ws, Q);
  const size_t in = (size_t)Q * depth, on = (size_t)Q * count;
  if (on_device) {
    launch_index_distinct(h->emb, (long)h->n, h->dim, h->storage, idx, score, Q, depth, same_at, start, count, ws, out_idx, out_score, out_dups, s);
  } else {                                           // a host caller: lists up, answers down, five equal-typed planes of one buffer
    ensure((void**)&h->dist_io, &h->dist_io_cap, (2 * in + 3 * on) * 4);
    int* d_idx = reinterpret_cast<int*>(h->dist_io); float* d_sc = reinterpret_cast<float*>(d_idx + in);
    int* o_idx = reinterpret_cast<int*>(d_sc + in); float* o_sc = reinterpret_cast<float*>(o_idx + on); int* o_dups = reinterpret_cast<int*>(o_sc + on);
    CC_HIP(hipMemcpyAsync(d_idx, idx, in * 4, hipMemcpyHostToDevice, s));
    if (score) CC_HIP(hipMemcpyAsync(d_sc, score, in * 4, hipMemcpyHostToDevice, s));
    launch_index_distinct(h->emb, (long)h->n, h->dim, h->storage, d_idx, score ? d_sc : nullptr, Q, depth, same_at, start, count, ws, o_idx, o_sc,
                          out_dups ? o_dups : nullptr, s);
    CC_HIP(hipMemcpyAsync(out_idx, o_idx, on * 4, hipMemcpyDeviceToHost, s));
    if (score) CC_HIP(hipMemcpyAsync(out_score, o_sc, on * 4, hipMemcpyDeviceToHost, s));
    if (out_dups) CC_HIP(hipMemcpyAsync(out_dups, o_dups, on * 4, hipMemcpyDeviceToHost, s));
  }
  if (total) CC_HIP(hipMemcpyAsync(total, ws.kept, (size_t)Q * 8, hipMemcpyDeviceToHost, s));
  if (total || !on_device) CC_HIP(hipStreamSynchronize(s));
  CC_API_END
}

// Day digest: the kernels are index_digest.hip's (its head tells how they fit together); here the checks, the scratch, the loop over the
// pieces and the copies.
int cc_index_digest(cc_index* h, float same_at, int max_leaders, int order, const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                    int64_t start, int64_t count, int32_t* out_row, int32_t* out_count, int32_t* out_ts_first, int32_t* out_ts_last,
                    int32_t* owner, int64_t* totals, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && out_row, "null argument");
  CC_CHECK(same_at == same_at, "same_at is NaN");
  CC_CHECK(max_leaders >= 1 && max_leaders <= CC_DIGEST_MAX_LEADERS, "max_leaders must be in [1, CC_DIGEST_MAX_LEADERS]");
  CC_CHECK(order == CC_DIGEST_BY_COUNT || order == CC_DIGEST_BY_FIRST, "unknown order");
  CC_CHECK(start >= 0, "start must not be negative");
  CC_CHECK(count >= 1, "count must be positive");
  CC_CHECK(!allowed || (n_groups > 0 && n_groups <= (1 << 24)), "bad group count");
  CC_CHECK(h->n < (1LL << 31), "a digest needs fewer than 2^31 rows");       // owner and the outputs hold row numbers in 32 bits
  const RowWhere w = make_where(h, where);
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const long n = (long)h->n;
  ensure((void**)&h->digest_ws, &h->digest_ws_cap, digest_ws_bytes(n));
  const DigestWs ws = digest_ws(h->digest_ws, n);
  if (!h->digest_pin) CC_HIP(hipHostMalloc((void**)&h->digest_pin, 64, hipHostMallocDefault));
  // a host caller: no leader stands past entry CC_DIGEST_MAX_LEADERS, so that many entries come down and the rest is padded here
  const int64_t wn = on_device ? count : std::min<int64_t>(count, CC_DIGEST_MAX_LEADERS);
  int *o_row = out_row, *o_cnt = out_count, *o_t0 = out_ts_first, *o_t1 = out_ts_last, *o_own = owner;
  if (!on_device) {
    ensure((void**)&h->digest_io, &h->digest_io_cap, ((size_t)4 * wn + (owner ? (size_t)n : 0)) * 4);
    o_row = reinterpret_cast<int*>(h->digest_io); o_cnt = o_row + wn; o_t0 = o_cnt + wn; o_t1 = o_t0 + wn;
    o_own = owner ? o_t1 + wn : nullptr;
  }
  const unsigned char* allowed_dev = n > 0 ? upload_allowed(h, allowed, n_groups, s) : nullptr;
  launch_digest_select(n, h->grp, allowed_dev, h->allowed_cap, w, ws, o_own, s);
  CC_HIP(hipMemcpyAsync(h->digest_pin, ws.m, 4, hipMemcpyDeviceToHost, s));
  CC_HIP(hipStreamSynchronize(s));                                           // the one readback: how many pieces to launch
  const long m = (long)h->digest_pin[0];
  for (long first = 0; first < m; first += kDigestChunk)
    launch_digest_piece(h->emb, n, h->dim, h->storage, first, (int)std::min<long>(kDigestChunk, m - first), same_at, max_leaders, h->ts, ws, o_own, s);
  launch_digest_finish(ws, order, start, wn, o_row, o_cnt, o_t0, o_t1, s);
  if (!on_device) {
    CC_HIP(hipMemcpyAsync(out_row, o_row, (size_t)wn * 4, hipMemcpyDeviceToHost, s));
    if (out_count) CC_HIP(hipMemcpyAsync(out_count, o_cnt, (size_t)wn * 4, hipMemcpyDeviceToHost, s));
    if (out_ts_first) CC_HIP(hipMemcpyAsync(out_ts_first, o_t0, (size_t)wn * 4, hipMemcpyDeviceToHost, s));
    if (out_ts_last) CC_HIP(hipMemcpyAsync(out_ts_last, o_t1, (size_t)wn * 4, hipMemcpyDeviceToHost, s));
    if (owner && n > 0) CC_HIP(hipMemcpyAsync(owner, o_own, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  }
  if (totals) CC_HIP(hipMemcpyAsync(totals, ws.totals, 3 * 8, hipMemcpyDeviceToHost, s));
  if (totals || !on_device) CC_HIP(hipStreamSynchronize(s));
  if (!on_device)
    for (int64_t p = wn; p < count; ++p) {
      out_row[p] = -1;
      if (out_count) out_count[p] = 0;
      if (out_ts_first) out_ts_first[p] = CC_ROW_NO_TS;
      if (out_ts_last) out_ts_last[p] = CC_ROW_NO_TS;
    }
  CC_API_END
}

// Seen before: the kernels are index_sightings.hip's (its head tells how they fit together) and the digest's selection; here the checks,
// the scratch, the zeroing and the copies.  Nothing is read back inside the call.
int cc_index_sightings(cc_index* h, const int64_t* rows, int n, float same_at, int flags, const uint8_t* allowed, int n_groups, const cc_row_filter* where,
                       int32_t* out_count, int32_t* out_best_row, float* out_best_score, uint32_t* out_group_counts, int n_group_counts,
                       int64_t* total, int on_device, void* stream) {
  CC_API_BEGIN
  CC_CHECK(h && rows && out_count, "null argument");
  CC_CHECK(same_at == same_at, "same_at is NaN");
  CC_CHECK(n >= 1 && n <= CC_SIGHT_MAX_OBJECTS, "n must be in [1, CC_SIGHT_MAX_OBJECTS]");
  CC_CHECK((flags & ~CC_SIGHT_SKIP_SELF) == 0, "unknown flag bits");
  CC_CHECK(out_group_counts ? (n_group_counts >= 1 && n_group_counts <= CC_SIGHT_MAX_GROUPS) : n_group_counts == 0,
           "n_group_counts must be in [1, CC_SIGHT_MAX_GROUPS] with out_group_counts and 0 without");
  CC_CHECK(!allowed || (n_groups > 0 && n_groups <= (1 << 24)), "bad group count");
  CC_CHECK(h->n < (1LL << 31), "sightings need fewer than 2^31 rows");       // out_best_row and the keys hold row numbers in 32 bits
  check_rows(h, rows, n);
  const RowWhere w = make_where(h, where);
  CC_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const long size = (long)h->n;                                              // > 0: a row passed check_rows
  ensure((void**)&h->digest_ws, &h->digest_ws_cap, digest_ws_bytes(size));
  const DigestWs ws = digest_ws(h->digest_ws, size);
  ensure((void**)&h->sight_ws, &h->sight_ws_cap, (size_t)CC_SIGHT_MAX_OBJECTS * 16);
  long long* obj = reinterpret_cast<long long*>(h->sight_ws);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(h->sight_ws) + CC_SIGHT_MAX_OBJECTS;
  const size_t gcn = (size_t)n * n_group_counts;
  int* o_cnt = out_count; int* o_row = out_best_row; float* o_sc = out_best_score; unsigned* o_gc = out_group_counts;
  if (!on_device) {
    ensure((void**)&h->sight_io, &h->sight_io_cap, ((size_t)3 * n + gcn) * 4);
    o_cnt = reinterpret_cast<int*>(h->sight_io); o_row = o_cnt + n; o_sc = reinterpret_cast<float*>(o_row + n);
    o_gc = out_group_counts ? reinterpret_cast<unsigned*>(o_sc + n) : nullptr;
    if (!out_best_row && !out_best_score) { o_row = nullptr; o_sc = nullptr; }
  }
  pin_rows(h, rows, n);
  CC_HIP(hipMemcpyAsync(obj, h->rows_pin, (size_t)n * 8, hipMemcpyHostToDevice, s));
  CC_HIP(hipEventRecord(h->rows_ev, s));
  const unsigned char* allowed_dev = upload_allowed(h, allowed, n_groups, s);
  launch_digest_select(size, h->grp, allowed_dev, h->allowed_cap, w, ws, nullptr, s);
  CC_HIP(hipMemsetAsync(o_cnt, 0, (size_t)n * 4, s));
  CC_HIP(hipMemsetAsync(best, 0, (size_t)n * 8, s));
  if (o_gc) CC_HIP(hipMemsetAsync(o_gc, 0, gcn * 4, s));
  launch_sightings(h->emb, size, h->dim, h->storage, ws.sel, ws.m, obj, n, same_at, flags & CC_SIGHT_SKIP_SELF, h->grp, n_group_counts, o_cnt, best, o_gc,
                   o_row, o_sc, s);
  if (!on_device) {
    CC_HIP(hipMemcpyAsync(out_count, o_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_best_row) CC_HIP(hipMemcpyAsync(out_best_row, o_row, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_best_score) CC_HIP(hipMemcpyAsync(out_best_score, o_sc, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (o_gc) CC_HIP(hipMemcpyAsync(out_group_counts, o_gc, gcn * 4, hipMemcpyDeviceToHost, s));
  }
  if (total) CC_HIP(hipMemcpyAsync(total, ws.totals + 1, 8, hipMemcpyDeviceToHost, s));
  if (total || !on_device) CC_HIP(hipStreamSynchronize(s));
  CC_API_END
}

int cc_index_remove_rows(cc_index* h, const uint8_t* drop, int64_t n, int64_t* removed) { return remove_impl(h, true, drop, n, 0, removed); }

int cc_index_remove_groups(cc_index* h, const uint8_t* drop, int n_groups, int64_t* removed) { return remove_impl(h, false, drop, 0, n_groups, removed); }

void cc_index_destroy(cc_index* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->emb, (void*)h->grp, (void*)h->trk, (void*)h->ts, (void*)h->cls, (void*)h->attr_tmp, (void*)h->best, (void*)h->first, (void*)h->key_hi, (void*)h->allowed, (void*)h->q16, (void*)h->q_planes, (void*)h->q_dev, (void*)h->scores, (void*)h->cand, (void*)h->idx_dev, (void*)h->sc_dev,
                  (void*)h->keep, (void*)h->drop_grp, (void*)h->gcnt, (void*)h->goff, (void*)h->bounce, (void*)h->rank_ws, (void*)h->dead, (void*)h->which_row, (void*)h->which_dev, (void*)h->near_ws, (void*)h->near_pos, (void*)h->near_dev, (void*)h->dist_ws, (void*)h->dist_io, (void*)h->digest_ws, (void*)h->digest_io, (void*)h->sight_ws, (void*)h->sight_io}) if (p) hipFree(p);
  if (h->digest_pin) hipHostFree(h->digest_pin);
  if (h->pin) hipHostFree(h->pin);
  if (h->rows_ev) { hipEventSynchronize(h->rows_ev); hipEventDestroy(h->rows_ev); }
  if (h->rows_pin) hipHostFree(h->rows_pin);
  pool_stream_put(h->device, h->stream);                  // parked, never destroyed (kernels.h)
  delete h;
}

}  // extern "C"
