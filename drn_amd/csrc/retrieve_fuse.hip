// DENSE SCORES and FUSED SHORTLISTS (drn_amd/retrieve.py: Shortlister.scores / scores_late, shortlist_scores, FusedShortlister).
//   drn_shortlist_scores      the WHOLE (sentence, video) score matrix of a table -- plain or ragged, plain or block-scaled FP8, one
//                             vector a sentence or late interaction -- with the bits the matching *_topn entry lists, -inf where the
//                             video is no candidate;
//   drn_shortlist_fuse_topn   each sentence's best n videos under the weighted fold of M such matrices, one total order;
//   drn_shortlist_fuse_rank   the place of a named video in that order (drn_shortlist_rank's three fields);
//   drn_shortlist_fuse_rerank the same fold and order over M matrices of LISTED pairs' scores (drn_shortlist_rerank_scores), column j
//                             of a row belonging to the video candidates[s][j]: the fused second stage of a cascade.
#include "common.h"
#include "shortlist.h"
#include "fuse.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// THE SCORE KERNELS are new bodies beside the counting kernels of retrieve_rank.hip (rank_block_kernel, rank_segments_kernel,
// rank_late_kernel), which run the phase-one bodies of the shortlist kernels "up to their keys" and count: these run them up to the same
// point and WRITE.  The table operand's scores() (AlPlain / AlQ8 of shortlist.h) is the very chain, the segmented maximum is taken over
// the ordered words with the lowest row winning, the tokens are folded ((0 + sim_0) + sim_1) + ... in fp32: a written score has the
// bits the list would show.  What the list would not show -- a video without rows, a score that is not finite, a clear mask bit, a
// sentence without live tokens -- is written as -inf, so "finite <=> candidate" and no NaN leaves the kernel.  A score of -0 is written
// as +0 (x + 0.f), as sl_word folds it into the key.
// One launch each, no workspace, no atomics.  A workgroup writes the elements out[s][v] of its own (sentence tile, video block) and no
// others: s < S and v < V are checked at every store, and the blocks of a plan tile [0, V).  As in retrieve_seg.hip every index read
// from a device table is clamped.
#define FS_BLOCK 256        // = RK_BLOCK = AL_BLOCK = LT_BLOCK = _lib.SHORTLIST_BLOCK = _lib.SHORTLIST_SEG_BLOCK
#define FS_LD (FS_BLOCK + 1)
#define FS_WORDS 8          // mask words of a plain block: FS_BLOCK / 32
#define FS_SEG_WORDS 9      // of a ragged block, which starts at any video

__device__ __forceinline__ float fs_none() { return __uint_as_float(0xff800000u); }                        // -inf: no candidate
__device__ __forceinline__ float fs_value(const float score, const bool ok) { return ok && isfinite(score) ? score + 0.f : fs_none(); }

// may sentence s list video v (v < V: its word lies inside the mask's row)
__device__ __forceinline__ bool fs_allowed(const int* __restrict__ allow, const int stride, const int s, const int v) {
  return allow == nullptr || ((allow[(long)s * stride + (v >> 5)] >> (v & 31)) & 1);
}

// rk_load_mask of retrieve_rank.hip: the tile's mask words of the videos [v0, v1) into mw[sentence of the tile][word - (v0 >> 5)], bits
// outside [v0, v1) cleared (no mask: every video of [v0, v1) is allowed) -> does any bit remain (workgroup-uniform; ends in a barrier).
// A sentence slot past S reads the last sentence's row; v1 <= V.
template <int NW>
__device__ __forceinline__ bool fs_load_mask(const int* __restrict__ allow, const int stride, const int s0, const int S, const int v0,
                                             const int v1, int* mw, int* wany, const int tid) {
  const int w0 = v0 >> 5;
  unsigned word = 0u;
  if (tid < 16 * NW) {
    const int sl = tid / NW, w = tid - sl * NW;
    const int lo = max(v0, (w0 + w) * 32), hi = min(v1, (w0 + w) * 32 + 32), bits = hi - lo;
    if (bits > 0) {
      const unsigned in = (bits == 32 ? 0xffffffffu : (1u << bits) - 1u) << (lo & 31);
      word = allow == nullptr ? in : (unsigned)allow[(long)min(s0 + sl, S - 1) * stride + w0 + w] & in;
    }
    mw[tid] = (int)word;
  }
  const bool any = __ballot(word != 0u) != 0ull;
  if ((tid & 63) == 0) wany[tid >> 6] = any;
  __syncthreads();
  return (wany[0] | wany[1] | wany[2] | wany[3]) != 0;
}

// a dark block: -inf for the tile's `rows` sentences from s0 and the nv videos from v0 (nv <= FS_BLOCK); no table row is read
__device__ __forceinline__ void fs_write_none(float* __restrict__ out, const long ld, const int s0, const int rows, const int v0, const int nv,
                                              const int tid) {
  for (int p = tid; p < rows * FS_BLOCK; p += 256) {
    const int sl = p / FS_BLOCK, vi = p - sl * FS_BLOCK;
    if (vi < nv) out[(long)(s0 + sl) * ld + v0 + vi] = fs_none();
  }
}

// The plain table.  shortlist_block_allow_kernel (retrieve_allow.hip) up to its keys, as rank_block_kernel runs it: lane (r, g) holds
// the scores of the videos v0 + 16 j + r for the sentences 4 g + i, and stores them where a key would be made.
template <typename Op>
__global__ __launch_bounds__(256) void scores_block_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ allow,
                                                           const int allow_stride, const int V, const int E, const int S,
                                                           float* __restrict__ out, const long ld) {
  __shared__ int mw[16 * FS_WORDS];                           // [sentence of the tile][mask word of the block]
  __shared__ int wany[4];                                     // each wave's "a bit is set"
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, vb = b * FS_BLOCK, v0 = vb + wave * 64;
  const int r = lane & 15, g = lane >> 4;
  const int rows = min(16, S - s0), ve = min(vb + FS_BLOCK, V);
  if (!fs_load_mask<FS_WORDS>(allow, allow_stride, s0, S, vb, ve, mw, wany, tid)) {
    fs_write_none(out, ld, s0, rows, vb, ve - vb, tid);       // (workgroup-uniform: a dark block)
    return;
  }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the wave's 64 videos are the words 2 wave and 2 wave + 1 of the 16 rows: lane -> (row lane & 15, word (lane >> 4) & 1)
  if (__ballot(mw[r * FS_WORDS + 2 * wave + (g & 1)] != 0) != 0ull) {
    // (a row past S or V reads the last row instead: its scores are not stored below)
    const typename Op::Q* qrow = q + (long)min(s0 + r, S - 1) * E;
    long row[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) row[j] = min(v0 + 16 * j + r, V - 1);
    op.scores(qrow, row, E, g, acc);
  }
  // C/D: column (video) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = v0 + 16 * j + r, sl = 4 * g + i, at = wave * 64 + 16 * j + r;
      const bool may = (mw[sl * FS_WORDS + (at >> 5)] >> (at & 31)) & 1;
      if (v < V && s0 + sl < S) out[(long)(s0 + sl) * ld + v] = fs_value(acc[j][i], may);
    }
}

// The ragged table, one vector a sentence.  shortlist_segments_allow_kernel (retrieve_allow.hip) up to where its states become keys, as
// rank_segments_kernel runs it: each state is stored where that kernel makes its key.
template <typename Op>
__global__ __launch_bounds__(256) void scores_segments_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ offsets,
                                                              const int* __restrict__ blk_vid, const int* __restrict__ allow,
                                                              const int allow_stride, const int R, const int V, const int E, const int S,
                                                              float* __restrict__ out, const long ld) {
  __shared__ sl_key_t keys[16 * FS_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block] states
  __shared__ float sc[16 * FS_LD];                            // [sentence of the tile][row of the pass]
  __shared__ int voff[FS_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ int wlong[4];                                    // each wave's longest run
  __shared__ int mw[16 * FS_SEG_WORDS];                       // [sentence of the tile][mask word from the block's first]
  __shared__ int wany[4];                                     // each wave's "a bit is set"
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16;
  const int r = lane & 15, g = lane >> 4;
  const int rows = min(16, S - s0);
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + FS_BLOCK, V)), nv = v1 - v0;
  if (!fs_load_mask<FS_SEG_WORDS>(allow, allow_stride, s0, S, v0, v1, mw, wany, tid)) {
    fs_write_none(out, ld, s0, rows, v0, nv, tid);            // (workgroup-uniform; a block without videos writes nothing)
    return;
  }
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // states per sentence: 16, 64 or 256 >= nv
  for (int i = tid; i <= nv; i += 256) voff[i] = min(max(offsets[v0 + i], 0), R);
  for (int p = tid; p < 16 * len; p += 256) keys[p] = 0ull;
  __syncthreads();
  {
    int mine = tid < nv ? voff[tid + 1] - voff[tid] : 0;      // (nv <= 256: one video per thread)
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) mine = max(mine, __shfl_xor(mine, w, 64));
    if (lane == 0) wlong[wave] = mine;
  }
  __syncthreads();
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), FS_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (sentence, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  // (a sentence past S reads the last one instead: its states are not stored below)
  const typename Op::Q* qrow = q + (long)min(s0 + r, S - 1) * E;
  for (int p0 = r0; p0 < r1; p0 += FS_BLOCK) {
    const int p1 = min(p0 + FS_BLOCK, r1), rw = p0 + wave * 64;
    if (rw < p1) {                                            // (wave-uniform: a wave whose 64 rows lie past the block reads nothing)
      // (a row past the block reads the table's last row instead: nobody folds its score)
      long row[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = min(rw + 16 * j + r, R - 1);
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      op.scores(qrow, row, E, g, acc);
      // C/D: column (row of the table) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[(4 * g + i) * FS_LD + wave * 64 + 16 * j + r] = acc[j][i];
    }
    __syncthreads();
    // the segmented maximum: item p = (pair p >> plg, part p & (P - 1)), pair = (sentence pair / nv, video pair % nv).  The P lanes of
    // a pair are adjacent and aligned, and 256 is a multiple of P: they leave the loop together, the same lanes in every pass
    const int items = (16 * nv) << plg;
    for (int p = tid; p < items; p += 256) {
      const int pair = p >> plg, part = p & (P - 1);
      const int sl = pair / nv, vi = pair - sl * nv;
      const int base = voff[vi], lo = max(base, p0), hi = min(voff[vi + 1], p1);
      const int share = (max(hi - lo, 0) + P - 1) >> plg;
      const int from = lo + part * share, to = min(from + share, hi);
      const float* mine = sc + sl * FS_LD;
      sl_key_t best = 0ull;
      for (int x = from; x < to; ++x) {
        const float s = mine[x - p0];
        const unsigned o = s != s ? 0xffffffffu : sl_word(s);
        const sl_key_t cand = ((sl_key_t)o << 32) | (sl_key_t)(~(unsigned)(x - base));
        best = cand > best ? cand : best;
      }
      for (int d = 1; d < P; d <<= 1) {
        const sl_key_t other = __shfl_xor(best, d, 64);
        best = other > best ? other : best;
      }
      if (part == 0 && best != 0ull) {
        const sl_key_t had = keys[sl * len + vi];
        keys[sl * len + vi] = best > had ? best : had;
      }
    }
    __syncthreads();
  }
  // states -> scores: a state's upper word is the ordered word of the video's best row (0: no row; all ones: a NaN among them; the
  // words of -inf and +inf bound the finite ones), and sl_score of it is the listed score
  for (int p = tid; p < 16 * len; p += 256) {
    const int sl = p >> lenlg, vi = p & (len - 1);
    if (vi >= nv || s0 + sl >= S) continue;
    const sl_key_t state = keys[p];
    const unsigned o = (unsigned)(state >> 32);
    const int v = v0 + vi;                                    // (v - 32 (v0 >> 5) < 32 FS_SEG_WORDS: inside mw)
    const bool may = (mw[sl * FS_SEG_WORDS + (v >> 5) - (v0 >> 5)] >> (v & 31)) & 1;
    const bool ok = o > 0x007fffffu && o < 0xff800000u && may;
    out[(long)(s0 + sl) * ld + v] = ok ? sl_score(state) : fs_none();
  }
}

// Late interaction.  shortlist_late_kernel (retrieve_late.hip) up to where its sums become keys, as rank_late_kernel runs it: thread vi
// stores video vi's sum.  A block none of whose videos the sentence may list is left before the offsets are read.
template <typename Op>
__global__ __launch_bounds__(256) void scores_late_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ lengths,
                                                          const int* __restrict__ offsets, const int* __restrict__ blk_vid,
                                                          const int* __restrict__ allow, const int allow_stride, const int R, const int V,
                                                          const int E, const int L, float* __restrict__ out, const long ld) {
  __shared__ sl_key_t keys[16 * FS_BLOCK];                    // 32 KiB: [token of the tile][video of the block] states
  __shared__ float sc[16 * FS_LD];                            // [token of the tile][row of the pass]
  __shared__ int voff[FS_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ float sums[FS_BLOCK];                            // each video's running sum over the tokens
  __shared__ int wlong[4];                                    // each wave's longest run
  __shared__ int wany[4];                                     // each wave's "a video is allowed"
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s = blockIdx.y;
  const int r = lane & 15, g = lane >> 4;
  const int Lt = min(max(lengths[s], 0), L);
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + FS_BLOCK, V)), nv = v1 - v0;
  const bool may = tid < nv && fs_allowed(allow, allow_stride, s, v0 + tid);    // (nv <= 256: one video per thread)
  {
    const bool any = __ballot(may) != 0ull;
    if (lane == 0) wany[wave] = any;
  }
  __syncthreads();
  if (Lt == 0 || !(wany[0] | wany[1] | wany[2] | wany[3])) {  // (workgroup-uniform: no live token, or a dark block)
    if (tid < nv) out[(long)s * ld + v0 + tid] = fs_none();
    return;
  }
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // states per token: 16, 64 or 256 >= nv
  for (int i = tid; i <= nv; i += 256) voff[i] = min(max(offsets[v0 + i], 0), R);
  for (int p = tid; p < 16 * len; p += 256) keys[p] = 0ull;
  sums[tid] = 0.f;
  __syncthreads();
  {
    int mine = tid < nv ? voff[tid + 1] - voff[tid] : 0;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) mine = max(mine, __shfl_xor(mine, w, 64));
    if (lane == 0) wlong[wave] = mine;
  }
  __syncthreads();
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), FS_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (token, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  for (int t0 = 0; t0 < Lt; t0 += 16) {                       // (workgroup-uniform: Lt is the sentence's)
    const int live = min(16, Lt - t0);
    // (a token slot past Lt reads the last live token instead: nobody folds its scores)
    const typename Op::Q* qrow = q + ((long)s * L + min(t0 + r, Lt - 1)) * E;
    for (int p0 = r0; p0 < r1; p0 += FS_BLOCK) {
      const int p1 = min(p0 + FS_BLOCK, r1), rw = p0 + wave * 64;
      if (rw < p1) {                                          // (wave-uniform: a wave whose 64 rows lie past the block reads nothing)
        // (a row past the block reads the table's last row instead: nobody folds its score)
        long row[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) row[j] = min(rw + 16 * j + r, R - 1);
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        op.scores(qrow, row, E, g, acc);
        // C/D: column (row of the table) lane & 15, row (token) 4 (lane >> 4) + i
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) sc[(4 * g + i) * FS_LD + wave * 64 + 16 * j + r] = acc[j][i];
      }
      __syncthreads();
      // the segmented maximum of retrieve_seg.hip over the tile's LIVE tokens: item p = (pair p >> plg, part p & (P - 1)), pair =
      // (token pair / nv, video pair % nv); the P lanes of a pair are adjacent and aligned and leave the loop together
      const int items = (live * nv) << plg;
      for (int p = tid; p < items; p += 256) {
        const int pair = p >> plg, part = p & (P - 1);
        const int tl = pair / nv, vi = pair - tl * nv;
        const int base = voff[vi], lo = max(base, p0), hi = min(voff[vi + 1], p1);
        const int share = (max(hi - lo, 0) + P - 1) >> plg;
        const int from = lo + part * share, to = min(from + share, hi);
        const float* mine = sc + tl * FS_LD;
        sl_key_t best = 0ull;
        for (int x = from; x < to; ++x) {
          const float d = mine[x - p0];
          const unsigned o = d != d ? 0xffffffffu : sl_word(d);
          const sl_key_t cand = ((sl_key_t)o << 32) | (sl_key_t)(~(unsigned)(x - base));
          best = cand > best ? cand : best;
        }
        for (int d = 1; d < P; d <<= 1) {
          const sl_key_t other = __shfl_xor(best, d, 64);
          best = other > best ? other : best;
        }
        if (part == 0 && best != 0ull) {
          const sl_key_t had = keys[tl * len + vi];
          keys[tl * len + vi] = best > had ? best : had;
        }
      }
      __syncthreads();
    }
    // the fold: the video's thread adds the tile's live tokens in ascending t and clears their states
    if (tid < nv) {
      float sum = sums[tid];
      for (int tl = 0; tl < live; ++tl) {
        sum += sl_score(keys[tl * len + tid]);
        keys[tl * len + tid] = 0ull;
      }
      sums[tid] = sum;
    }
    __syncthreads();
  }
  // sums -> scores, one per thread; a video without rows or with a clear mask bit has none
  if (tid < nv) out[(long)s * ld + v0 + tid] = fs_value(sums[tid], may && voff[tid + 1] > voff[tid]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// THE FUSED SCORE of (sentence s, video v) over M stacked matrices, and its key.  The order is the definition's
// (drn_amd.retrieve.fuse_scores_reference): acc = +0, then for m ascending acc = acc + (w[m] * x_m), every product and every sum rounded
// on its own, by fu_mul and fu_add of fuse.h, which keep hipcc from contracting the two into one FMA.

// `at` = s * ld + v.  Key 0 where the pair is no candidate: the fold is not finite, the mask bit is clear, or (drop) a term is not
// finite / (skip) none is.
__device__ __forceinline__ sl_key_t fu_key(const float* __restrict__ scores, const long stride_m, const float* __restrict__ weights,
                                           const int M, const int mode, const long at, const int v, const bool allowed) {
  float acc = 0.f;
  bool all = true, some = false;
  for (int m = 0; m < M; ++m) {
    const float x = scores[m * stride_m + at];
    const bool present = isfinite(x);
    const float term = fu_mul(weights[m], x);
    if (mode == DRN_FUSE_DROP || present) acc = fu_add(acc, term);
    all = all && present;
    some = some || present;
  }
  const bool ok = allowed && (mode == DRN_FUSE_DROP ? all : some);
  return ok ? sl_key(acc, v) : 0ull;
}

// Phase one of drn_shortlist_fuse_topn: workgroup (block of 256 videos, sentence) makes its 256 keys, sorts them and writes the best
// m = min(n, 256) to ws[s][b][0..m): the lists sl_launch_merge / sl_launch_merge_deep take.
#define FU_BLOCK 256
__global__ __launch_bounds__(256) void fuse_block_kernel(const float* __restrict__ scores, const long stride_m, const long ld,
                                                         const float* __restrict__ weights, const int M, const int mode,
                                                         const int* __restrict__ allow, const int allow_stride, const int V, const int m,
                                                         const int nblocks, sl_key_t* __restrict__ ws) {
  __shared__ sl_key_t keys[FU_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x, s = blockIdx.y, v = b * FU_BLOCK + tid;
  sl_key_t key = 0ull;
  if (v < V) key = fu_key(scores, stride_m, weights, M, mode, (long)s * ld + v, v, fs_allowed(allow, allow_stride, s, v));
  keys[tid] = key;
  __syncthreads();
  sl_sort_desc<FU_BLOCK, 256>(keys, 1, tid);
  if (tid < m) ws[((long)s * nblocks + b) * m + tid] = keys[tid];
}

// Phase one of drn_shortlist_fuse_rerank: fuse_block_kernel with candidate SLOTS in the place of store positions.  Workgroup (block of
// 256 slots, sentence) reads the sentence's whole row of candidates into LDS (C <= 1024 words, 4 KiB).  Slot j is LISTED when its id lies
// in [0, V), no EARLIER slot of the whole row holds the same id (the rule of shortlist_rerank_kernel: of a repeated position the first
// occurrence counts) and the mask bit is set -- the rule is applied HERE, from the row, and not trusted to the -inf of the matrices, so
// the merge's premise that no video reaches it twice holds on any matrices.  A mask word is read only for an id already known to lie in
// [0, V).  The key is fu_key's with the REAL store position: the order among the listed is the full fused shortlist's and the place in
// the list means nothing.  The block's 256 keys are sorted and the best m = min(n, 256) go to ws[s][b][0..m).
__global__ __launch_bounds__(256) void fuse_slots_kernel(const float* __restrict__ scores, const long stride_m, const long ld,
                                                         const float* __restrict__ weights, const int M, const int mode,
                                                         const int* __restrict__ candidates, const int* __restrict__ allow,
                                                         const int allow_stride, const int V, const int C, const int m, const int nblocks,
                                                         sl_key_t* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) int cand[DRN_RERANK_MAX_CANDIDATES];          // 4 KiB: the sentence's row of the list
  __shared__ sl_key_t keys[FU_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x, s = blockIdx.y, j = b * FU_BLOCK + tid;
  for (int i = tid; i < C; i += 256) cand[i] = candidates[(long)s * C + i];
  __syncthreads();
  sl_key_t key = 0ull;
  if (j < C) {
    const int id = cand[j];
    if (id >= 0 && id < V) {
      // the scan of the EARLIER slots, four words a read (a wave's lanes read the same words: a broadcast), then the last j & 3
      int dup = 0;
      const int4* c4 = (const int4*)cand;
      for (int i = 0; i < (j >> 2); ++i) {
        const int4 c = c4[i];
        dup |= (c.x == id) | (c.y == id) | (c.z == id) | (c.w == id);
      }
      for (int i = j & ~3; i < j; ++i) dup |= cand[i] == id;
      if (!dup && fs_allowed(allow, allow_stride, s, id)) key = fu_key(scores, stride_m, weights, M, mode, (long)s * ld + j, id, true);
    }
  }
  keys[tid] = key;
  __syncthreads();
  sl_sort_desc<FU_BLOCK, 256>(keys, 1, tid);
  if (tid < m) ws[((long)s * nblocks + b) * m + tid] = keys[tid];
}

// drn_shortlist_fuse_rank: one workgroup per sentence makes the target's key (every thread, from the same M loads) and walks the V
// videos; the keys of a sentence are distinct and the target's own equals tk, so nothing is counted twice and the target is not counted.
#define FU_RANK_THREADS 1024
__global__ __launch_bounds__(FU_RANK_THREADS) void fuse_rank_kernel(const float* __restrict__ scores, const long stride_m, const long ld,
                                                                    const float* __restrict__ weights, const int M, const int mode,
                                                                    const int* __restrict__ targets, const int* __restrict__ allow,
                                                                    const int allow_stride, const int V, int* __restrict__ rank,
                                                                    float* __restrict__ score, int* __restrict__ total) {
  __shared__ int wa[FU_RANK_THREADS / 64], wn[FU_RANK_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x;
  const int t = targets[s], tc = min(max(t, 0), V - 1);       // (clamped for every read)
  const sl_key_t own = fu_key(scores, stride_m, weights, M, mode, (long)s * ld + tc, tc, fs_allowed(allow, allow_stride, s, tc));
  const sl_key_t tk = t == tc ? own : 0ull;
  int above = 0, any = 0;
  for (int v = tid; v < V; v += FU_RANK_THREADS) {
    const sl_key_t key = fu_key(scores, stride_m, weights, M, mode, (long)s * ld + v, v, fs_allowed(allow, allow_stride, s, v));
    above += key > tk;
    any += key != 0ull;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    above += __shfl_xor(above, w, 64);
    any += __shfl_xor(any, w, 64);
  }
  if (lane == 0) {
    wa[wave] = above;
    wn[wave] = any;
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0, c = 0;
    for (int w = 0; w < FU_RANK_THREADS / 64; ++w) {
      a += wa[w];
      c += wn[w];
    }
    rank[s] = tk != 0ull ? a : -1;
    score[s] = tk != 0ull ? sl_score(tk) : 0.f;
    total[s] = c;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The entries.

struct FsArgs {
  const void* table;                                          // emb, or the codes where scales is given
  const uint8_t* scales;                                      // (null: a plain table)
  const void* queries;
  const int32_t *lengths, *offsets, *blk_vid, *allow;
  int allow_stride, R, V, nblocks, E, S, L, dtype;
  float* out;
  int ld_out;
};

// RAGGED is a compile-time switch: an operand instantiates only the kernels it is launched on
template <bool RAGGED, typename Op>
static void fs_launch(const Op op, const FsArgs& a, hipStream_t stream) {
  typedef typename Op::Q Q;
  const Q* q = (const Q*)a.queries;
  const int stride = a.allow ? a.allow_stride : 0;
  if constexpr (!RAGGED)
    scores_block_kernel<Op><<<dim3(cdiv(a.V, FS_BLOCK), cdiv(a.S, 16)), 256, 0, stream>>>(op, q, a.allow, stride, a.V, a.E, a.S, a.out, a.ld_out);
  else if (!a.lengths)
    scores_segments_kernel<Op><<<dim3(a.nblocks, cdiv(a.S, 16)), 256, 0, stream>>>(op, q, a.offsets, a.blk_vid, a.allow, stride, a.R, a.V, a.E,
                                                                                  a.S, a.out, a.ld_out);
  else
    scores_late_kernel<Op><<<dim3(a.nblocks, a.S), 256, 0, stream>>>(op, q, a.lengths, a.offsets, a.blk_vid, a.allow, stride, a.R, a.V, a.E, a.L,
                                                                     a.out, a.ld_out);
}

extern "C" int drn_shortlist_scores(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths,
                                    const int32_t* offsets, const int32_t* blk_vid, const int32_t* allow, int allow_stride, int R, int V,
                                    int nblocks, int E, int S, int L, int dtype, float* out, int ld_out, void* stream) {
  const char* what = "drn_shortlist_scores";
  drn_clear_status();
  const FsArgs a = {table, scales, queries, lengths, offsets, blk_vid, allow, allow_stride, R, V, nblocks, E, S, L, dtype, out, ld_out};
  const bool ragged = offsets != nullptr, late = lengths != nullptr;
  DRN_CHECK_ARG(table && queries && out, "%s: null pointer", what);
  DRN_CHECK_ARG(ragged == (blk_vid != nullptr), "%s: offsets and blk_vid are given together (a ragged table) or not at all", what);
  DRN_CHECK_ARG(!late || ragged, "%s: lengths (late interaction) need a ragged table: offsets and blk_vid", what);
  if (ragged)
    DRN_CHECK_ARG(R >= 1 && V >= 1 && E >= 1 && S >= 1, "%s: bad args (R = %d rows, V = %d videos, E = %d columns, S = %d sentences)", what, R,
                  V, E, S);
  else
    DRN_CHECK_ARG(V >= 1 && E >= 1 && S >= 1, "%s: bad args (V = %d videos, E = %d columns, S = %d sentences)", what, V, E, S);
  if (late) DRN_CHECK_ARG(L >= 1 && L <= DRN_LATE_MAX_TOKENS, "%s: L = %d tokens outside [1, %d]", what, L, DRN_LATE_MAX_TOKENS);
  else DRN_CHECK_ARG(L == 1, "%s: L = %d without lengths (one vector a sentence: L must be 1)", what, L);
  if (scales) DRN_CHECK_ARG(E % MX8_BLOCK == 0, "%s: E = %d is not a multiple of the block of %d columns", what, E, MX8_BLOCK);
  if (ragged)
    DRN_CHECK_ARG(nblocks >= 1 && nblocks <= V && (long)nblocks * FS_BLOCK >= V, "%s: %d blocks outside [ceil(V / %d), V] for V = %d videos", what,
                  nblocks, FS_BLOCK, V);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "%s: dtype %d (float32 / bfloat16 only)", what, dtype);
  DRN_CHECK_ARG(ld_out >= V, "%s: ld_out = %d below V = %d", what, ld_out, V);
  DRN_CHECK_ARG(((uintptr_t)table & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)out & 3) == 0,
                "%s: the table and the queries must be 16-byte aligned, out 4-byte aligned", what);
  DRN_CHECK_ARG(((uintptr_t)lengths & 3) == 0 && ((uintptr_t)offsets & 3) == 0 && ((uintptr_t)blk_vid & 3) == 0,
                "%s: lengths, offsets and blk_vid must be 4-byte aligned", what);
  if (const int rc = fu_check_allow(what, allow, allow_stride, V)) return rc;
  if (late) DRN_CHECK_ARG(S <= 65535, "%s: S = %d, more than 65535 sentences", what, S);
  else DRN_CHECK_ARG(cdiv(S, 16) <= 65535, "%s: S = %d, more than 65535 tiles of 16 sentences", what, S);
  const uint8_t* codes = (const uint8_t*)table;
  const bool bf16 = dtype == DRN_BF16;
  // (a quantised bf16 chain keeps two scale blocks of loads in flight on the plain table, one on the ragged: retrieve_q8.hip says why)
  hipStream_t st = (hipStream_t)stream;
  if (!ragged) {
    if (!scales && bf16) fs_launch<false>(AlPlain<bf16_t>{(const bf16_t*)table}, a, st);
    else if (!scales) fs_launch<false>(AlPlain<float>{(const float*)table}, a, st);
    else if (bf16) fs_launch<false>(AlQ8<bf16_t, 2>{codes, scales}, a, st);
    else fs_launch<false>(AlQ8<float, 1>{codes, scales}, a, st);
  } else {
    if (!scales && bf16) fs_launch<true>(AlPlain<bf16_t>{(const bf16_t*)table}, a, st);
    else if (!scales) fs_launch<true>(AlPlain<float>{(const float*)table}, a, st);
    else if (bf16) fs_launch<true>(AlQ8<bf16_t, 1>{codes, scales}, a, st);
    else fs_launch<true>(AlQ8<float, 1>{codes, scales}, a, st);
  }
  return drn_launch_status(what);
}

// (`cols` columns a matrix, named `col` in the refusals: the V videos, or the C slots of drn_shortlist_fuse_rerank)
static int fu_check(const char* what, const float* scores, long long stride_m, int ld, const float* weights, int M, int mode,
                    const int32_t* allow, int allow_stride, int V, int S, const char col, const int cols) {
  DRN_CHECK_ARG(scores && weights, "%s: null pointer", what);
  DRN_CHECK_ARG(V >= 1 && S >= 1, "%s: bad args (V = %d videos, S = %d sentences)", what, V, S);
  DRN_CHECK_ARG(M >= 1 && M <= DRN_FUSE_MAX_TABLES, "%s: M = %d tables outside [1, %d]", what, M, DRN_FUSE_MAX_TABLES);
  DRN_CHECK_ARG(mode == DRN_FUSE_DROP || mode == DRN_FUSE_SKIP, "%s: mode = %d is neither %d (drop) nor %d (skip)", what, mode, DRN_FUSE_DROP,
                DRN_FUSE_SKIP);
  DRN_CHECK_ARG(ld >= cols, "%s: ld = %d below %c = %d", what, ld, col, cols);
  DRN_CHECK_ARG(M == 1 || stride_m >= (long long)(S - 1) * ld + cols,
                "%s: stride_m = %lld below the (S - 1) * ld + %c = %lld elements of one matrix", what, stride_m, col,
                (long long)(S - 1) * ld + cols);
  DRN_CHECK_ARG(((uintptr_t)scores & 3) == 0 && ((uintptr_t)weights & 3) == 0, "%s: scores and weights must be 4-byte aligned", what);
  DRN_CHECK_ARG(S <= 65535, "%s: S = %d, more than 65535 sentences", what, S);
  return fu_check_allow(what, allow, allow_stride, V);
}

extern "C" int drn_shortlist_fuse_topn(const float* scores, long long stride_m, int ld, const float* weights, int M, int mode,
                                       const int32_t* allow, int allow_stride, int V, int S, int n, void* ws, int ws_keys, int32_t* ids,
                                       float* out_scores, int32_t* counts, void* stream) {
  const char* what = "drn_shortlist_fuse_topn";
  drn_clear_status();
  if (const int rc = fu_check(what, scores, stride_m, ld, weights, M, mode, allow, allow_stride, V, S, 'V', V)) return rc;
  DRN_CHECK_ARG(ws && ids && out_scores && counts, "%s: null pointer", what);
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_DEEP_MAX, "%s: n = %d outside [1, %d]", what, n, DRN_SHORTLIST_DEEP_MAX);
  DRN_CHECK_ARG(((uintptr_t)ws & 7) == 0, "%s: the workspace must be 8-byte aligned", what);
  const int m = n < FU_BLOCK ? n : FU_BLOCK, nblocks = cdiv(V, FU_BLOCK);
  const long need = (long)S * nblocks * m;
  DRN_CHECK_ARG(ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (S * ceil(V / %d) * min(n, %d))", what, ws_keys, need, FU_BLOCK,
                FU_BLOCK);
  const int stride = allow ? allow_stride : 0;
  fuse_block_kernel<<<dim3(nblocks, S), 256, 0, (hipStream_t)stream>>>(scores, (long)stride_m, (long)ld, weights, M, mode, allow, stride, V, m,
                                                                      nblocks, (sl_key_t*)ws);
  if (n <= DRN_SHORTLIST_MAX) sl_launch_merge((const sl_key_t*)ws, S, n, m, nblocks, ids, out_scores, counts, (hipStream_t)stream);
  else sl_launch_merge_deep((const sl_key_t*)ws, S, n, m, nblocks, ids, out_scores, counts, (hipStream_t)stream);
  return drn_launch_status(what);
}

extern "C" int drn_shortlist_fuse_rank(const float* scores, long long stride_m, int ld, const float* weights, int M, int mode,
                                       const int32_t* targets, const int32_t* allow, int allow_stride, int V, int S, int32_t* rank,
                                       float* score, int32_t* total, void* stream) {
  const char* what = "drn_shortlist_fuse_rank";
  drn_clear_status();
  if (const int rc = fu_check(what, scores, stride_m, ld, weights, M, mode, allow, allow_stride, V, S, 'V', V)) return rc;
  DRN_CHECK_ARG(targets && rank && score && total, "%s: null pointer", what);
  DRN_CHECK_ARG(((uintptr_t)targets & 3) == 0, "%s: targets must be 4-byte aligned", what);
  const int stride = allow ? allow_stride : 0;
  fuse_rank_kernel<<<S, FU_RANK_THREADS, 0, (hipStream_t)stream>>>(scores, (long)stride_m, (long)ld, weights, M, mode, targets, allow, stride, V,
                                                                  rank, score, total);
  return drn_launch_status(what);
}

extern "C" int drn_shortlist_fuse_rerank(const float* scores, long long stride_m, int ld, const float* weights, int M, int mode,
                                         const int32_t* candidates, const int32_t* allow, int allow_stride, int V, int C, int S, int n,
                                         void* ws, int ws_keys, int32_t* ids, float* out_scores, int32_t* counts, void* stream) {
  const char* what = "drn_shortlist_fuse_rerank";
  drn_clear_status();
  DRN_CHECK_ARG(candidates && ws && ids && out_scores && counts, "%s: null pointer", what);
  DRN_CHECK_ARG(C >= 1 && C <= DRN_RERANK_MAX_CANDIDATES, "%s: C = %d candidates a sentence outside [1, %d]", what, C, DRN_RERANK_MAX_CANDIDATES);
  if (const int rc = fu_check(what, scores, stride_m, ld, weights, M, mode, allow, allow_stride, V, S, 'C', C)) return rc;
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_DEEP_MAX, "%s: n = %d outside [1, %d]", what, n, DRN_SHORTLIST_DEEP_MAX);
  DRN_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)candidates & 3) == 0, "%s: the workspace must be 8-byte aligned, candidates 4-byte aligned",
                what);
  const int m = n < FU_BLOCK ? n : FU_BLOCK, nblocks = cdiv(C, FU_BLOCK);
  const long need = (long)S * nblocks * m;
  DRN_CHECK_ARG(ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (S * ceil(C / %d) * min(n, %d))", what, ws_keys, need, FU_BLOCK,
                FU_BLOCK);
  const int stride = allow ? allow_stride : 0;
  fuse_slots_kernel<<<dim3(nblocks, S), 256, 0, (hipStream_t)stream>>>(scores, (long)stride_m, (long)ld, weights, M, mode, candidates, allow, stride,
                                                                      V, C, m, nblocks, (sl_key_t*)ws);
  if (n <= DRN_SHORTLIST_MAX) sl_launch_merge((const sl_key_t*)ws, S, n, m, nblocks, ids, out_scores, counts, (hipStream_t)stream);
  else sl_launch_merge_deep((const sl_key_t*)ws, S, n, m, nblocks, ids, out_scores, counts, (hipStream_t)stream);
  return drn_launch_status(what);
}
