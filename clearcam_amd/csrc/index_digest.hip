// Day digest on the embedding index (cc_index_digest): leader clustering of the competing rows in row order.  The C entry point stands
// with the handle in index.hip; this file holds the kernels.
//
// Walking the competing rows in ascending row number, a row joins the first-created leader it is at least same_at similar to, else it
// becomes a leader while fewer than max_leaders exist, else it is left over.  The similarity is the float cc_index_gram returns for the
// pair: the tiles here run gram_tile_accumulate of gram_tile.h, the accumulation of gram_kernel.
//
//   select           digest_count_kernel (competing rows per block of 1024 rows, row_passes of kernels.h: the rule of rank_keys_kernel),
//                    digest_offsets_kernel (one block: the exclusive scan of the counts, the number of competing rows, and the leader
//                    tables and counters cleared), digest_scatter_kernel (the competing row numbers, in order, into one list).
//   per piece of up to 1024 competing rows, three launches in stream order:
//     digest_leaders_kernel   64 x 64 tiles of the piece's rows against the leaders so far, compared with same_at into a bit matrix.  The
//                    leader list and its length live on the device; a block whose leader tile lies past the length exits.
//     gram_kernel    (launch_index_gram_bits of index_distinct.hip) the piece against itself, the tiles at and above the diagonal.
//     digest_walk_kernel      one block.  Every thread reduces its row's leader words to "first old leader or none"; the piece's own bit
//                    matrix goes to LDS, cleared where the walk must not look.  One wave walks the rows in order, lane w holding word w
//                    of the claimed set, which starts as the rows that have an old leader: a row whose bit is set is skipped (it neither
//                    leads nor claims; the walk steps from one clear bit to the next, so a piece of known objects costs 16 steps), a
//                    row whose bit is clear leads while the leader count is below the cap and then claims the unclaimed rows behind it
//                    that match it, else it and every unclaimed row behind it is left over and claims nothing.  Old leaders precede every leader
//                    of the piece in creation order, so "first old leader, else first claimant of the piece" is the sequential rule,
//                    and the answer does not depend on where the pieces are cut.  All threads then find their leader, add counts and
//                    ts extremes to tables in LDS (integer sums, min and max: order-free), write `owner`, and one thread per leader
//                    folds the tables into the global ones and appends the new leaders.
//   finish           digest_finish_kernel: one block sorts at most 1024 (count, row) keys (bitonic, in LDS), writes the window, the
//                    padding and the three totals.
#include <climits>
#include "gram_tile.h"
#include "../../include/clearcam_hip.h"

namespace cc {

namespace {

static_assert(CC_DIGEST_MAX_LEADERS == kDigestMaxLeaders && CC_ROW_NO_TS == kRowNoTs, "the header and kernels.h disagree");
static_assert(kDigestChunk == kDistinctMaxDepth && kDigestMaxLeaders == 1024, "one thread per row of a piece and per leader; launch_index_gram_bits makes the piece's matrix");

constexpr int kSelRows = 1024;                                            // rows per block of the selection
constexpr size_t kWalkLds = (size_t)kDigestChunk * kDistinctWords * 8;    // the piece's own bit matrix

// this thread's place among the block's threads with `ok` set, and their number: ballot per wave, the wave sums through LDS
__device__ __forceinline__ int block_place(bool ok, int* wcnt, int* all) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long b = __ballot(ok);
  if (lane == 0) wcnt[wave] = __popcll(b);
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) { before += w < wave ? wcnt[w] : 0; sum += wcnt[w]; }
  *all = sum;
  return before + __popcll(b & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(1024) void digest_count_kernel(long n, const int* __restrict__ grp, const unsigned char* __restrict__ allowed, int n_allowed,
                                                            const RowWhere where, unsigned* __restrict__ bcnt, int* __restrict__ owner) {
  __shared__ int wcnt[16];
  const long r = (long)blockIdx.x * kSelRows + threadIdx.x;
  const bool ok = r < n && row_passes(grp, allowed, n_allowed, where, r);
  int all;
  block_place(ok, wcnt, &all);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = (unsigned)all;
  if (owner && r < n && !ok) owner[r] = -1;
}

__global__ __launch_bounds__(1024) void digest_offsets_kernel(const unsigned* __restrict__ bcnt, long nb, unsigned* __restrict__ boff, DigestWs ws) {
  __shared__ unsigned wsum[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  ws.lead_cnt[t] = 0; ws.lead_ts_min[t] = INT_MAX; ws.lead_ts_max[t] = INT_MIN; ws.lead_row[t] = -1;
  unsigned run = 0;
  for (long base = 0; base < nb; base += 1024) {
    const long i = base + t;
    const unsigned v = i < nb ? bcnt[i] : 0u;
    unsigned x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { before += w < wave ? wsum[w] : 0u; all += wsum[w]; }
    if (i < nb) boff[i] = run + before + x - v;
    run += all;
    __syncthreads();
  }
  if (t == 0) { *ws.m = (int)run; *ws.n_lead = 0; ws.totals[0] = 0; ws.totals[1] = (long long)run; ws.totals[2] = 0; }
}

__global__ __launch_bounds__(1024) void digest_scatter_kernel(long n, const int* __restrict__ grp, const unsigned char* __restrict__ allowed, int n_allowed,
                                                              const RowWhere where, const unsigned* __restrict__ boff, long long* __restrict__ sel) {
  __shared__ int wcnt[16];
  const long r = (long)blockIdx.x * kSelRows + threadIdx.x;
  const bool ok = r < n && row_passes(grp, allowed, n_allowed, where, r);
  int all;
  const int p = block_place(ok, wcnt, &all);
  if (ok) sel[(size_t)boff[blockIdx.x] + p] = r;                // boff + p < the number of competing rows <= n
}

// grid (16 leader tiles, tiles of the piece), 256 threads: tile rows = rows of the piece, tile columns = leaders.
template <int STORAGE>
__global__ __launch_bounds__(256) void digest_leaders_kernel(const char* __restrict__ emb, long size, int dim, const long long* __restrict__ rows, int len,
                                                             const long long* __restrict__ lead_row, const int* __restrict__ n_lead,
                                                             unsigned long long* __restrict__ bits, float same_at) {
  __shared__ __attribute__((aligned(16))) float As[kGramTile * kGramLd];
  __shared__ __attribute__((aligned(16))) float Bs[kGramTile * kGramLd];
  __shared__ long long srow[2 * kGramTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = blockIdx.y, tj = blockIdx.x, L = *n_lead;
  if (ti * kGramTile >= len || tj * kGramTile >= L) return;     // the whole block: past the piece, or past the leaders
  if (tid < 2 * kGramTile) {
    if (tid < kGramTile) { const int li = ti * kGramTile + tid; srow[tid] = li < len ? rows[li] : -1; }
    else { const int lj = tj * kGramTile + tid - kGramTile; srow[tid] = lj < L ? lead_row[lj] : -1; }
  }
  __syncthreads();
  f32x4 acc[2][2];
  gram_tile_accumulate<STORAGE>(emb, size, dim, srow, As, Bs, tid, acc);
  const unsigned long long mine = gram_tile_bits(acc, same_at, reinterpret_cast<unsigned char*>(As), tid);
  const int gi = ti * kGramTile + wave * 16 + lane;
  if (lane < 16 && gi < len) bits[(size_t)gi * kDistinctWords + tj] = mine;
}

__global__ __launch_bounds__(1024) void digest_walk_kernel(const unsigned long long* __restrict__ bits_lead, const unsigned long long* __restrict__ bits_self,
                                                           const long long* __restrict__ rows, int len, int cap, const int* __restrict__ ts, DigestWs ws,
                                                           int* __restrict__ owner) {
  extern __shared__ unsigned long long sb[];                    // [len][16]: the piece's bit matrix, then per new leader the rows it claimed
  __shared__ int scnt[kDigestMaxLeaders], smin[kDigestMaxLeaders], smax[kDigestMaxLeaders];
  __shared__ unsigned short snew[kDigestChunk];                 // the rows of the piece that became leaders, in order
  __shared__ unsigned long long shas[kDistinctWords], slead[kDistinctWords], sleft[kDistinctWords];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = *ws.n_lead, LW = (L + 63) >> 6;                 // L <= cap <= 1024
  int old = -1;
  if (tid < len) {
    for (int w = 0; w < LW; ++w) {                              // words past LW: nobody wrote them in this piece
      unsigned long long v = bits_lead[(size_t)tid * kDistinctWords + w];
      if (L - w * 64 < 64) v &= (1ull << (L - w * 64)) - 1;     // only leaders that exist
      if (v) { old = w * 64 + __ffsll(v) - 1; break; }
    }
  }
  scnt[tid] = 0; smin[tid] = INT_MAX; smax[tid] = INT_MIN;
  const unsigned long long hb = __ballot(old >= 0);
  if (lane == 0) shas[wave] = hb;
  for (int e = tid; e < len * kDistinctWords; e += 1024) {
    const int i = e >> 4, w = e & 15;
    unsigned long long v = 0;
    if (w >= (i >> 6) && w * 64 < len) {                        // a tile the Gram epilogue of THIS piece wrote
      v = bits_self[e];
      if (w == (i >> 6)) v &= ~((2ull << (i & 63)) - 1);        // only rows behind i
      if (len - w * 64 < 64) v &= (1ull << (len - w * 64)) - 1; // only rows of the piece
    }
    sb[e] = v;
  }
  __syncthreads();
  if (tid < 64) {                                               // lanes 16 .. 63 mirror lanes 0 .. 15
    const int lw = tid & 15;
    unsigned long long drop = shas[lw], lead = 0, left = 0;     // claimed: by an old leader, or by a leader of this piece
    int nl = L, j = 0;
    while (j < len) {                                           // j, nl and every branch are wave-uniform: they come from readlane
      const int w = j >> 6;
      const unsigned lo = __builtin_amdgcn_readlane((unsigned)drop, w), hi = __builtin_amdgcn_readlane((unsigned)(drop >> 32), w);   // the builtin returns int
      const unsigned long long dw = ((unsigned long long)hi << 32) | lo;
      unsigned long long open = ~dw & ~((1ull << (j & 63)) - 1);  // the unclaimed rows of word w from j on
      if (len - w * 64 < 64) open &= (1ull << (len - w * 64)) - 1;
      if (!open) { j = (w + 1) * 64; continue; }                // claimed rows are stepped over a word at a time
      j = w * 64 + __ffsll(open) - 1;
      if (nl >= cap) {                                          // the cap: every unclaimed row from j on is left over and claims nothing
        unsigned long long m = lw < w ? 0ull : lw == w ? ~((1ull << (j & 63)) - 1) : ~0ull;
        if (lw * 64 >= len) m = 0;
        else if (len - lw * 64 < 64) m &= (1ull << (len - lw * 64)) - 1;
        left = ~drop & m;
        break;
      }
      const unsigned long long newly = sb[j * kDistinctWords + lw] & ~drop;
      drop |= newly;
      if (lw == w) lead |= 1ull << (j & 63);
      if (tid < kDistinctWords) sb[j * kDistinctWords + lw] = newly;
      ++nl; ++j;
    }
    if (tid < kDistinctWords) { slead[tid] = lead; sleft[tid] = left; }
  }
  __syncthreads();
  int nnew = 0, before = 0, nleft = 0;
#pragma unroll
  for (int w = 0; w < kDistinctWords; ++w) { const int c = __popcll(slead[w]); nnew += c; before += w < wave ? c : 0; nleft += __popcll(sleft[w]); }
  const bool leads = tid < len && ((slead[wave] >> lane) & 1ull);
  const int k = before + __popcll(slead[wave] & ((1ull << lane) - 1));
  if (leads) snew[k] = (unsigned short)tid;
  __syncthreads();
  if (tid < len) {
    int slot = -2;                                              // left over
    if (old >= 0) slot = old;
    else if (leads) slot = L + k;
    else if (!((sleft[wave] >> lane) & 1ull)) {
      for (int c = 0; c < nnew && snew[c] < tid; ++c)           // the first leader of the piece that claimed this row (exactly one did)
        if ((sb[snew[c] * kDistinctWords + wave] >> lane) & 1ull) { slot = L + c; break; }
    }
    const long long row = rows[tid];
    if (slot >= 0) {
      atomicAdd(&scnt[slot], 1);
      const int t = ts[row];
      if (t != kRowNoTs) { atomicMin(&smin[slot], t); atomicMax(&smax[slot], t); }
    }
    if (owner) owner[row] = slot < 0 ? -2 : (int)(slot < L ? ws.lead_row[slot] : rows[snew[slot - L]]);
  }
  __syncthreads();
  if (tid < L + nnew) {                                         // L + nnew <= cap: one thread per leader, old and new
    if (tid >= L) ws.lead_row[tid] = rows[snew[tid - L]];
    if (scnt[tid]) {
      ws.lead_cnt[tid] += scnt[tid];
      ws.lead_ts_min[tid] = min(ws.lead_ts_min[tid], smin[tid]);
      ws.lead_ts_max[tid] = max(ws.lead_ts_max[tid], smax[tid]);
    }
  }
  if (tid == 0) { *ws.n_lead = L + nnew; ws.totals[2] += nleft; }
}

__global__ __launch_bounds__(1024) void digest_finish_kernel(DigestWs ws, int order, long long start, long long count, int* __restrict__ out_row,
                                                             int* __restrict__ out_count, int* __restrict__ out_ts_first, int* __restrict__ out_ts_last) {
  __shared__ unsigned long long skey[kDigestMaxLeaders];
  __shared__ unsigned short sslot[kDigestMaxLeaders];
  const int tid = threadIdx.x, L = *ws.n_lead;
  unsigned long long key = ~0ull;                               // past the leaders: sorts last
  if (tid < L) {
    const unsigned row = (unsigned)ws.lead_row[tid];            // below 2^31
    key = order == CC_DIGEST_BY_COUNT ? ((unsigned long long)(unsigned)(INT_MAX - ws.lead_cnt[tid]) << 32) | row : (unsigned long long)row;
  }
  skey[tid] = key; sslot[tid] = (unsigned short)tid;
  __syncthreads();
  for (int k = 2; k <= kDigestMaxLeaders; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int o = tid ^ j;
      if (o > tid) {
        const unsigned long long a = skey[tid], b = skey[o];
        if ((a > b) == ((tid & k) == 0)) {
          skey[tid] = b; skey[o] = a;
          const unsigned short s = sslot[tid]; sslot[tid] = sslot[o]; sslot[o] = s;
        }
      }
      __syncthreads();
    }
  const long long p = (long long)tid - start;
  if (tid < L && p >= 0 && p < count) {
    const int s = sslot[tid], lo = ws.lead_ts_min[s], hi = ws.lead_ts_max[s];
    out_row[p] = (int)ws.lead_row[s];
    if (out_count) out_count[p] = ws.lead_cnt[s];
    if (out_ts_first) out_ts_first[p] = lo > hi ? kRowNoTs : lo;
    if (out_ts_last) out_ts_last[p] = lo > hi ? kRowNoTs : hi;
  }
  const long long first = L > start ? (L - start < count ? L - start : count) : 0;
  for (long long q = first + tid; q < count; q += 1024) {
    out_row[q] = -1;
    if (out_count) out_count[q] = 0;
    if (out_ts_first) out_ts_first[q] = kRowNoTs;
    if (out_ts_last) out_ts_last[q] = kRowNoTs;
  }
  if (tid == 0) ws.totals[0] = L;
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline long sel_blocks(long n) { return (n + kSelRows - 1) / kSelRows; }

}  // namespace

size_t digest_ws_bytes(long n) {
  const size_t nb = (size_t)sel_blocks(n), bm = (size_t)kDigestChunk * kDistinctWords * 8;
  return up256((size_t)n * 8) + 2 * up256(nb * 4) + 2 * up256(bm) + up256((size_t)kDigestMaxLeaders * 8) + 3 * up256((size_t)kDigestMaxLeaders * 4) + 3 * 256;
}

DigestWs digest_ws(void* base, long n) {
  const size_t nb = (size_t)sel_blocks(n), bm = (size_t)kDigestChunk * kDistinctWords * 8;
  char* p = static_cast<char*>(base);
  DigestWs ws;
  ws.sel = reinterpret_cast<long long*>(p); p += up256((size_t)n * 8);
  ws.bcnt = reinterpret_cast<unsigned*>(p); p += up256(nb * 4);
  ws.boff = reinterpret_cast<unsigned*>(p); p += up256(nb * 4);
  ws.bits_lead = reinterpret_cast<unsigned long long*>(p); p += up256(bm);
  ws.bits_self = reinterpret_cast<unsigned long long*>(p); p += up256(bm);
  ws.lead_row = reinterpret_cast<long long*>(p); p += up256((size_t)kDigestMaxLeaders * 8);
  ws.lead_cnt = reinterpret_cast<int*>(p); p += up256((size_t)kDigestMaxLeaders * 4);
  ws.lead_ts_min = reinterpret_cast<int*>(p); p += up256((size_t)kDigestMaxLeaders * 4);
  ws.lead_ts_max = reinterpret_cast<int*>(p); p += up256((size_t)kDigestMaxLeaders * 4);
  ws.n_lead = reinterpret_cast<int*>(p); p += 256;
  ws.m = reinterpret_cast<int*>(p); p += 256;
  ws.totals = reinterpret_cast<long long*>(p);
  return ws;
}

void launch_digest_select(long n, const int* grp, const unsigned char* allowed, int n_allowed, const RowWhere& where, const DigestWs& ws, int* owner,
                          hipStream_t stream) {
  const long nb = sel_blocks(n);
  if (nb) hipLaunchKernelGGL(digest_count_kernel, dim3((unsigned)nb), dim3(1024), 0, stream, n, grp, allowed, n_allowed, where, ws.bcnt, owner);
  hipLaunchKernelGGL(digest_offsets_kernel, dim3(1), dim3(1024), 0, stream, ws.bcnt, nb, ws.boff, ws);
  if (nb) hipLaunchKernelGGL(digest_scatter_kernel, dim3((unsigned)nb), dim3(1024), 0, stream, n, grp, allowed, n_allowed, where, ws.boff, ws.sel);
  CC_HIP(hipGetLastError());
}

void launch_digest_piece(const void* emb, long size, int dim, int storage, long first, int len, float same_at, int max_leaders, const int* ts,
                         const DigestWs& ws, int* owner, hipStream_t stream) {
  const long long* rows = ws.sel + first;
  const dim3 grid(kDigestMaxLeaders / kGramTile, (len + kGramTile - 1) / kGramTile), block(256);
  const char* e = static_cast<const char*>(emb);
  if (storage == F32) hipLaunchKernelGGL(digest_leaders_kernel<F32>, grid, block, 0, stream, e, size, dim, rows, len, ws.lead_row, ws.n_lead, ws.bits_lead, same_at);
  else if (storage == BF16) hipLaunchKernelGGL(digest_leaders_kernel<BF16>, grid, block, 0, stream, e, size, dim, rows, len, ws.lead_row, ws.n_lead, ws.bits_lead, same_at);
  else hipLaunchKernelGGL(digest_leaders_kernel<CC_INDEX_I8>, grid, block, 0, stream, e, size, dim, rows, len, ws.lead_row, ws.n_lead, ws.bits_lead, same_at);
  CC_HIP(hipGetLastError());
  launch_index_gram_bits(emb, size, dim, storage, rows, len, ws.bits_self, same_at, stream);
  ensure_max_lds(digest_walk_kernel, kWalkLds);
  hipLaunchKernelGGL(digest_walk_kernel, dim3(1), dim3(1024), kWalkLds, stream, ws.bits_lead, ws.bits_self, rows, len, max_leaders, ts, ws, owner);
  CC_HIP(hipGetLastError());
}

void launch_digest_finish(const DigestWs& ws, int order, long long start, long long count, int* out_row, int* out_count, int* out_ts_first,
                          int* out_ts_last, hipStream_t stream) {
  hipLaunchKernelGGL(digest_finish_kernel, dim3(1), dim3(1024), 0, stream, ws, order, start, count, out_row, out_count, out_ts_first, out_ts_last);
  CC_HIP(hipGetLastError());
}

}  // namespace cc
