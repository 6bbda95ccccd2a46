// The RANK OF A NAMED VIDEO in the full shortlist order (drn_amd/retrieve.py, Shortlister.rank / rank_late): for each sentence, how many
// candidate videos precede targets[s] under the total order of retrieve.hip (score descending, then position ascending) over the WHOLE
// table -- no cap at DRN_SHORTLIST_MAX, no list, no sort -- with the target's score and the number of candidates.
//   drn_shortlist_rank             the plain table   (the scores of drn_shortlist_topn);
//   drn_shortlist_segments_rank    the ragged table  (drn_shortlist_segments_topn: a video's best row);
//   drn_shortlist_late_rank        late interaction  (drn_shortlist_late_topn: the sum over the live tokens of the video's best row).
// Each takes the table plain (scales == NULL) or in block-scaled FP8 (codes and scales), and a nullable packed allow mask.
//   drn_shortlist_rank_phase, drn_shortlist_segments_rank_phase, drn_shortlist_late_rank_phase run launch 1 or launch 2 below alone:
//   the pieces a corpus of several tables ranks with (retrieve_shard_rank.hip).  Same kernels, same bits.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// THREE launches, no atomics, no tickets, nothing read on the host:
//   1. THE TARGET KEYS.  tkey[s] = the 64-bit key (sl_key) of (s, targets[s]), from the very chain the counting kernels run -- the table
//      operand's scores() (AlPlain / AlQ8 of shortlist.h), the same K-steps in ascending order -- so the target's key below EQUALS
//      tkey[s].  Key 0 where the target is outside [0, V) (it is clamped for every read), owns no row, is masked, its score is not
//      finite or (late) the sentence has no live token.  On the plain table one wavefront per 16 sentences: the B rows are the tile's 16
//      targets and the diagonal of one 16x16 accumulator is kept.  On the ragged table one workgroup per sentence walks the target's
//      rows in passes of RK_BLOCK, keeps the maximum per token and folds the live tokens in ascending order (one "token" without lengths).
//   2. THE BLOCK COUNTS.  The phase-one bodies of shortlist_block_allow_kernel, shortlist_segments_allow_kernel (retrieve_allow.hip) and
//      shortlist_late_kernel (retrieve_late.hip) up to the point where a (sentence, video) has its key; then, instead of the sort and the
//      list, per sentence the keys > tkey[s] and the keys != 0 are counted -- in registers and shuffles on the plain table, by wave ballots
//      on the ragged ones -- and one lane writes the pair to cnt[s][b].  The keys of a sentence are distinct and the target's own equals
//      tkey[s]: nothing is counted twice and the target is not counted.  The dark-block skip stays in the first two and writes zeros.
//   3. THE REDUCE.  One wavefront per sentence sums its nblocks pairs: rank = the keys above (-1 where tkey == 0), score = sl_score(tkey)
//      or 0, total = the keys that are not 0.
// ws: S target keys of 8 bytes, then S * nblocks pairs of int32: 8 S (1 + nblocks) bytes.
//
// An answer depends on the sentence, its target, the table and the mask alone: every score is that of the shortlist kernels (fixed
// order per (sentence, row)), and the counts are integers.  As in retrieve_seg.hip every index read from a device table is clamped.
#define RK_BLOCK 256        // = AL_BLOCK = LT_BLOCK = _lib.SHORTLIST_BLOCK = _lib.SHORTLIST_SEG_BLOCK
#define RK_LD (RK_BLOCK + 1)
#define RK_WORDS 8          // mask words of a ranked block: RK_BLOCK / 32
#define RK_SEG_WORDS 9      // of a ragged block, which starts at any video

// two counts of at most RK_BLOCK in one word: the keys above the target's, and (<< 16) the keys that are not 0
__device__ __forceinline__ int rk_two(const bool above, const bool any) { return (int)above + ((int)any << 16); }
__device__ __forceinline__ int2 rk_pair(const int two) { return make_int2(two & 0xffff, two >> 16); }

// may sentence s list video v (v < V: its word lies inside the mask's row)
__device__ __forceinline__ bool rk_allowed(const int* __restrict__ allow, const int stride, const int s, const int v) {
  return allow == nullptr || ((allow[(long)s * stride + (v >> 5)] >> (v & 31)) & 1);
}

// al_load_mask of retrieve_allow.hip with a NULLABLE mask (no mask: every video of [v0, v1) is allowed): the tile's mask words of the
// videos [v0, v1) into mw[sentence of the tile][word - (v0 >> 5)], bits outside [v0, v1) cleared -> does any bit remain
// (workgroup-uniform; ends in a barrier).  A sentence slot past S reads the last sentence's row; v1 <= V.
template <int NW>
__device__ __forceinline__ bool rk_load_mask(const int* __restrict__ allow, const int stride, const int s0, const int S, const int v0,
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

// ---------------------------------------------------------------------------------------------------------------------------
// 1. the target keys

// the plain table: wavefront = 16 sentences; A = their query rows, B = their targets' rows (all four row groups of the operand name the
// same 16 rows: one accumulator is read), and sentence sl's score is the diagonal element (column sl, row sl)
template <typename Op>
__global__ __launch_bounds__(64) void rank_target_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ targets,
                                                         const int* __restrict__ allow, const int allow_stride, const int V, const int E,
                                                         const int S, sl_key_t* __restrict__ tkey) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4, s0 = blockIdx.x * 16;
  const int s = min(s0 + r, S - 1);                           // (a slot past S reads the last sentence instead and writes nothing)
  const int t = targets[s], tc = min(max(t, 0), V - 1);
  const typename Op::Q* qrow = q + (long)s * E;
  long row[4];
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    row[j] = tc;
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  op.scores(qrow, row, E, g, acc);
  // C/D: column (target of sentence) lane & 15, row (sentence) 4 (lane >> 4) + i
  const int i = r & 3;
  const float d = i == 0 ? acc[0][0] : i == 1 ? acc[0][1] : i == 2 ? acc[0][2] : acc[0][3];
  if ((r >> 2) == g && s0 + r < S) {
    const bool ok = t == tc && rk_allowed(allow, allow_stride, s, tc);
    tkey[s] = ok ? sl_key(d, tc) : 0ull;
  }
}

// the ragged table: workgroup = one sentence; A = a tile of 16 of its tokens (without lengths: L = 1, one live token), B = the target's
// rows in passes of RK_BLOCK.  st[token of the tile] is the maximum of the ordered words (a NaN's is all ones), as the segmented maximum
// of the ranking kernels; thread 0 folds the live tokens as shortlist_late_kernel does: ((0 + sim_0) + sim_1) + ... in fp32.
template <typename Op>
__global__ __launch_bounds__(256) void rank_target_rows_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ lengths,
                                                               const int* __restrict__ offsets, const int* __restrict__ targets,
                                                               const int* __restrict__ allow, const int allow_stride, const int R,
                                                               const int V, const int E, const int L, sl_key_t* __restrict__ tkey) {
  __shared__ unsigned wmax[4 * 16];                           // [wave][token of the tile]: the pass's maximum
  __shared__ unsigned st[16];                                 // [token of the tile]: the maximum so far
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x;
  const int r = lane & 15, g = lane >> 4;
  const int Lt = lengths == nullptr ? 1 : min(max(lengths[s], 0), L);
  const int t = targets[s], tc = min(max(t, 0), V - 1);
  const int r0 = min(max(offsets[tc], 0), R), r1 = min(max(offsets[tc + 1], r0), R);
  float sum = 0.f;                                            // (thread 0's is the score)
  for (int t0 = 0; t0 < Lt; t0 += 16) {                       // (workgroup-uniform)
    const int live = min(16, Lt - t0);
    // (a token slot past Lt reads the last live token instead: nobody folds its scores)
    const typename Op::Q* qrow = q + ((long)s * L + min(t0 + r, Lt - 1)) * E;
    if (tid < 16) st[tid] = 0u;
    __syncthreads();
    for (int p0 = r0; p0 < r1; p0 += RK_BLOCK) {
      const int rw = p0 + wave * 64;
      unsigned m[4] = {0u, 0u, 0u, 0u};
      if (rw < r1) {                                          // (wave-uniform: a wave whose 64 rows lie past the video reads nothing)
        // (a row past the video reads the table's last row instead: its score is not folded)
        long row[4];
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          row[j] = min(rw + 16 * j + r, R - 1);
          acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        op.scores(qrow, row, E, g, acc);
        // C/D: column (row of the table) lane & 15, row (token) 4 (lane >> 4) + i
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float d = acc[j][i];
            const unsigned o = d != d ? 0xffffffffu : sl_word(d);
            if (rw + 16 * j + r < r1) m[i] = max(m[i], o);
          }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int w = 8; w > 0; w >>= 1) m[i] = max(m[i], (unsigned)__shfl_xor((int)m[i], w, 64));
        if (r == 0) wmax[wave * 16 + 4 * g + i] = m[i];
      }
      __syncthreads();
      if (tid < 16) st[tid] = max(max(st[tid], max(wmax[tid], wmax[16 + tid])), max(wmax[32 + tid], wmax[48 + tid]));
      __syncthreads();
    }
    if (tid == 0)
      for (int tl = 0; tl < live; ++tl) sum += sl_score((sl_key_t)st[tl] << 32);
    __syncthreads();
  }
  if (tid == 0) {
    const bool ok = t == tc && r1 > r0 && Lt > 0 && rk_allowed(allow, allow_stride, s, tc);
    tkey[s] = ok ? sl_key(sum, tc) : 0ull;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 2. the block counts

// shortlist_block_allow_kernel (retrieve_allow.hip) up to its keys, which stay in registers: lane (r, g) holds the keys of the videos
// v0 + 16 j + r for the sentences 4 g + i
template <typename Op>
__global__ __launch_bounds__(256) void rank_block_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ allow,
                                                         const int allow_stride, const int V, const int E, const int S, const int nblocks,
                                                         const sl_key_t* __restrict__ tkey, int2* __restrict__ cnt) {
  __shared__ int mw[16 * RK_WORDS];                           // [sentence of the tile][mask word of the block]
  __shared__ int wany[4];                                     // each wave's "a bit is set"
  __shared__ int wc[4 * 16];                                  // [wave][sentence of the tile]: its two counts
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, v0 = b * RK_BLOCK + wave * 64;
  const int r = lane & 15, g = lane >> 4;
  const int rows = min(16, S - s0);
  if (!rk_load_mask<RK_WORDS>(allow, allow_stride, s0, S, b * RK_BLOCK, min(b * RK_BLOCK + RK_BLOCK, V), mw, wany, tid)) {
    if (tid < rows) cnt[(long)(s0 + tid) * nblocks + b] = make_int2(0, 0);      // (workgroup-uniform: a dark block)
    return;
  }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the wave's 64 videos are the words 2 wave and 2 wave + 1 of the 16 rows: lane -> (row lane & 15, word (lane >> 4) & 1)
  if (__ballot(mw[r * RK_WORDS + 2 * wave + (g & 1)] != 0) != 0ull) {
    // (a row past S or V reads the last row instead: its scores become no keys below)
    const typename Op::Q* qrow = q + (long)min(s0 + r, S - 1) * E;
    long row[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) row[j] = min(v0 + 16 * j + r, V - 1);
    op.scores(qrow, row, E, g, acc);
  }
  sl_key_t tk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) tk[i] = tkey[min(s0 + 4 * g + i, S - 1)];
  int two[4] = {0, 0, 0, 0};
  // C/D: column (video) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = v0 + 16 * j + r, sl = 4 * g + i, at = wave * 64 + 16 * j + r;
      const bool ok = v < V && s0 + sl < S && ((mw[sl * RK_WORDS + (at >> 5)] >> (at & 31)) & 1);
      const sl_key_t key = ok ? sl_key(acc[j][i], v) : 0ull;
      two[i] += rk_two(key > tk[i], key != 0ull);
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int w = 8; w > 0; w >>= 1) two[i] += __shfl_xor(two[i], w, 64);
    if (r == 0) wc[wave * 16 + 4 * g + i] = two[i];
  }
  __syncthreads();
  if (tid < rows) cnt[(long)(s0 + tid) * nblocks + b] = rk_pair(wc[tid] + wc[16 + tid] + wc[32 + tid] + wc[48 + tid]);
}

// shortlist_segments_allow_kernel (retrieve_allow.hip) up to where its states become keys: each key is counted where that kernel stores it
template <typename Op>
__global__ __launch_bounds__(256) void rank_segments_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ offsets,
                                                            const int* __restrict__ blk_vid, const int* __restrict__ allow,
                                                            const int allow_stride, const int R, const int V, const int E, const int S,
                                                            const int nblocks, const sl_key_t* __restrict__ tkey, int2* __restrict__ cnt) {
  __shared__ sl_key_t keys[16 * RK_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block] states
  __shared__ float sc[16 * RK_LD];                            // [sentence of the tile][row of the pass]
  __shared__ int voff[RK_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ int wlong[4];                                    // each wave's longest run
  __shared__ int mw[16 * RK_SEG_WORDS];                       // [sentence of the tile][mask word from the block's first]
  __shared__ int wany[4];                                     // each wave's "a bit is set"
  __shared__ sl_key_t tk[16];                                 // [sentence of the tile]: its target's key
  __shared__ int wc[16 * 4];                                  // [sentence of the tile][part]: its two counts
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16;
  const int r = lane & 15, g = lane >> 4;
  const int rows = min(16, S - s0);
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + RK_BLOCK, V)), nv = v1 - v0;
  if (!rk_load_mask<RK_SEG_WORDS>(allow, allow_stride, s0, S, v0, v1, mw, wany, tid)) {
    if (tid < rows) cnt[(long)(s0 + tid) * nblocks + b] = make_int2(0, 0);      // (workgroup-uniform; also a block without videos)
    return;
  }
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // states per sentence: 16, 64 or 256 >= nv
  for (int i = tid; i <= nv; i += 256) voff[i] = min(max(offsets[v0 + i], 0), R);
  for (int p = tid; p < 16 * len; p += 256) keys[p] = 0ull;
  if (tid < 16) tk[tid] = tkey[min(s0 + tid, S - 1)];
  if (tid < 64) wc[tid] = 0;
  __syncthreads();
  {
    int mine = tid < nv ? voff[tid + 1] - voff[tid] : 0;      // (nv <= 256: one video per thread)
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) mine = max(mine, __shfl_xor(mine, w, 64));
    if (lane == 0) wlong[wave] = mine;
  }
  __syncthreads();
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), RK_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (sentence, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  // (a sentence past S reads the last one instead: its states become no keys below)
  const typename Op::Q* qrow = q + (long)min(s0 + r, S - 1) * E;
  for (int p0 = r0; p0 < r1; p0 += RK_BLOCK) {
    const int p1 = min(p0 + RK_BLOCK, r1), rw = p0 + wave * 64;
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
        for (int i = 0; i < 4; ++i) sc[(4 * g + i) * RK_LD + wave * 64 + 16 * j + r] = acc[j][i];
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
      const float* mine = sc + sl * RK_LD;
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
  // states -> keys, counted as they are made.  16 len is a multiple of 256: every lane takes every ballot.  A sentence's len states are
  // min(len, 64) adjacent lanes of one wave, in len / 64 waves at most: the group's first lane writes its part
  const int width = min(len, 64);
  for (int p = tid; p < 16 * len; p += 256) {
    const int sl = p >> lenlg, vi = p & (len - 1);
    const sl_key_t state = keys[p];
    const unsigned o = (unsigned)(state >> 32);
    const int v = v0 + min(vi, RK_BLOCK - 1);                 // (v - 32 (v0 >> 5) < 32 RK_SEG_WORDS: inside mw)
    const bool may = (mw[sl * RK_SEG_WORDS + (v >> 5) - (v0 >> 5)] >> (v & 31)) & 1;
    const bool ok = vi < nv && s0 + sl < S && o > 0x007fffffu && o < 0xff800000u && may;
    const sl_key_t key = ok ? ((sl_key_t)o << 32) | (sl_key_t)(~(unsigned)(v0 + vi)) : 0ull;
    const int from = lane & ~(width - 1);
    const unsigned long long in = width == 64 ? ~0ull : 0xffffull;
    const int above = __popcll((__ballot(key > tk[sl]) >> from) & in), any = __popcll((__ballot(key != 0ull) >> from) & in);
    if (lane == from) wc[sl * 4 + (lenlg == 8 ? wave : 0)] = above + (any << 16);
  }
  __syncthreads();
  if (tid < rows) cnt[(long)(s0 + tid) * nblocks + b] = rk_pair(wc[4 * tid] + wc[4 * tid + 1] + wc[4 * tid + 2] + wc[4 * tid + 3]);
}

// shortlist_late_kernel (retrieve_late.hip) up to where its sums become keys: thread vi makes video vi's key and the waves' ballots count
template <typename Op>
__global__ __launch_bounds__(256) void rank_late_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ lengths,
                                                        const int* __restrict__ offsets, const int* __restrict__ blk_vid,
                                                        const int* __restrict__ allow, const int allow_stride, const int R, const int V,
                                                        const int E, const int L, const int nblocks, const sl_key_t* __restrict__ tkey,
                                                        int2* __restrict__ cnt) {
  __shared__ sl_key_t keys[16 * RK_BLOCK];                    // 32 KiB: [token of the tile][video of the block] states
  __shared__ float sc[16 * RK_LD];                            // [token of the tile][row of the pass]
  __shared__ int voff[RK_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ float sums[RK_BLOCK];                            // each video's running sum over the tokens
  __shared__ int wlong[4];                                    // each wave's longest run
  __shared__ int wc[4];                                       // each wave's two counts
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s = blockIdx.y;
  const int r = lane & 15, g = lane >> 4;
  const int Lt = min(max(lengths[s], 0), L);
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + RK_BLOCK, V)), nv = v1 - v0;
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // states per token: 16, 64 or 256 >= nv
  for (int i = tid; i <= nv; i += 256) voff[i] = min(max(offsets[v0 + i], 0), R);
  for (int p = tid; p < 16 * len; p += 256) keys[p] = 0ull;
  sums[tid] = 0.f;
  __syncthreads();
  {
    int mine = tid < nv ? voff[tid + 1] - voff[tid] : 0;      // (nv <= 256: one video per thread)
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) mine = max(mine, __shfl_xor(mine, w, 64));
    if (lane == 0) wlong[wave] = mine;
  }
  __syncthreads();
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), RK_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (token, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  for (int t0 = 0; t0 < Lt; t0 += 16) {                       // (workgroup-uniform: Lt is the sentence's)
    const int live = min(16, Lt - t0);
    // (a token slot past Lt reads the last live token instead: nobody folds its scores)
    const typename Op::Q* qrow = q + ((long)s * L + min(t0 + r, Lt - 1)) * E;
    for (int p0 = r0; p0 < r1; p0 += RK_BLOCK) {
      const int p1 = min(p0 + RK_BLOCK, r1), rw = p0 + wave * 64;
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
          for (int i = 0; i < 4; ++i) sc[(4 * g + i) * RK_LD + wave * 64 + 16 * j + r] = acc[j][i];
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
        const float* mine = sc + tl * RK_LD;
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
  // sums -> keys, one per thread (nv <= 256), counted by the waves' ballots.  sl_key makes no key of a sum that is not finite; a video
  // without rows, a sentence without live tokens or a clear mask bit makes none either.  (v < V: its word lies inside the mask's row.)
  bool ok = tid < nv && Lt > 0;
  if (ok) ok = voff[tid + 1] > voff[tid] && rk_allowed(allow, allow_stride, s, v0 + tid);
  const sl_key_t key = ok ? sl_key(sums[tid], v0 + tid) : 0ull;
  const int above = __popcll(__ballot(key > tkey[s])), any = __popcll(__ballot(key != 0ull));
  if (lane == 0) wc[wave] = above + (any << 16);
  __syncthreads();
  if (tid == 0) cnt[(long)s * nblocks + b] = rk_pair(wc[0] + wc[1] + wc[2] + wc[3]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// 3. the reduce: one wavefront per sentence
__global__ __launch_bounds__(256) void rank_reduce_kernel(const sl_key_t* __restrict__ tkey, const int2* __restrict__ cnt, const int S,
                                                          const int nblocks, int* __restrict__ rank, float* __restrict__ score,
                                                          int* __restrict__ total) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;                                         // (wave-uniform)
  int above = 0, any = 0;
  for (int b = lane; b < nblocks; b += 64) {
    const int2 c = cnt[(long)s * nblocks + b];
    above += c.x;
    any += c.y;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    above += __shfl_xor(above, w, 64);
    any += __shfl_xor(any, w, 64);
  }
  if (lane == 0) {
    const sl_key_t k = tkey[s];
    rank[s] = k != 0ull ? above : -1;
    score[s] = k != 0ull ? sl_score(k) : 0.f;
    total[s] = any;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The entries: one argument record, one list of checks, one launch switch.

enum RkShape { RK_PLAIN, RK_RAGGED, RK_LATE };

struct RkArgs {
  RkShape shape;
  const void* table;                                          // emb, or the codes where scales is given
  const uint8_t* scales;                                      // (null: a plain table)
  const void* queries;
  const int32_t *lengths, *offsets, *blk_vid, *targets, *allow;                 // (allow may be null: no mask)
  int allow_stride, R, V, nblocks, E, S, L, dtype;
  void* ws;
  int ws_bytes;
  int32_t* rank;
  float* score;
  int32_t* total;
  // the phases alone (the *_phase entries; 0 = the three launches above).  1: the target kernel writes S keys to `keys`; 2: the
  // counting kernel reads S THRESHOLDS from `keys` where it reads tkey, and writes cnt [S][blocks] pairs.  ws and the results are unused.
  int phase;
  sl_key_t* keys;
  int2* cnt;
  int cnt_bytes;
};

static int rk_check(const char* what, const RkArgs& a) {
  const bool ragged = a.shape != RK_PLAIN, late = a.shape == RK_LATE;
  const bool mine = a.phase == 0 ? a.targets && a.ws && a.rank && a.score && a.total : a.phase == 1 ? a.targets && a.keys : a.keys && a.cnt;
  DRN_CHECK_ARG(a.table && a.queries && mine && (!ragged || (a.offsets && a.blk_vid)) && (!late || a.lengths), "%s: null pointer", what);
  if (ragged)
    DRN_CHECK_ARG(a.R >= 1 && a.V >= 1 && a.E >= 1 && a.S >= 1, "%s: bad args (R = %d rows, V = %d videos, E = %d columns, S = %d sentences)",
                  what, a.R, a.V, a.E, a.S);
  else
    DRN_CHECK_ARG(a.V >= 1 && a.E >= 1 && a.S >= 1, "%s: bad args (V = %d videos, E = %d columns, S = %d sentences)", what, a.V, a.E, a.S);
  if (late) DRN_CHECK_ARG(a.L >= 1 && a.L <= DRN_LATE_MAX_TOKENS, "%s: L = %d tokens outside [1, %d]", what, a.L, DRN_LATE_MAX_TOKENS);
  if (a.scales) DRN_CHECK_ARG(a.E % MX8_BLOCK == 0, "%s: E = %d is not a multiple of the block of %d columns", what, a.E, MX8_BLOCK);
  if (ragged)
    DRN_CHECK_ARG(a.nblocks >= 1 && a.nblocks <= a.V && (long)a.nblocks * RK_BLOCK >= a.V, "%s: %d blocks outside [ceil(V / %d), V] for V = %d videos",
                  what, a.nblocks, RK_BLOCK, a.V);
  DRN_CHECK_ARG(a.dtype == DRN_F32 || a.dtype == DRN_BF16, "%s: dtype %d (float32 / bfloat16 only)", what, a.dtype);
  DRN_CHECK_ARG(((uintptr_t)a.table & 15) == 0 && ((uintptr_t)a.queries & 15) == 0 && (((uintptr_t)a.ws | (uintptr_t)a.keys | (uintptr_t)a.cnt) & 7) == 0,
                "%s: the table and the queries must be 16-byte aligned, the workspace 8-byte aligned", what);
  DRN_CHECK_ARG(((uintptr_t)a.targets & 3) == 0 && ((uintptr_t)a.lengths & 3) == 0, "%s: targets and lengths must be 4-byte aligned", what);
  if (a.allow) {
    DRN_CHECK_ARG(a.allow_stride == 0 || a.allow_stride == cdiv(a.V, 32),
                  "%s: allow_stride = %d is neither 0 (one mask for all sentences) nor ceil(V / 32) = %d (one row per sentence)", what,
                  a.allow_stride, cdiv(a.V, 32));
    DRN_CHECK_ARG(((uintptr_t)a.allow & 3) == 0, "%s: the mask must be 4-byte aligned", what);
  }
  const long nblocks = ragged ? a.nblocks : cdiv(a.V, RK_BLOCK), need = 8L * a.S * (1 + nblocks), pairs = 8L * a.S * nblocks;
  if (a.phase == 0)
    DRN_CHECK_ARG(need <= 0x7fffffffL && a.ws_bytes >= need, "%s: the workspace holds %d bytes, %ld are needed (8 * S * (1 + blocks))", what,
                  a.ws_bytes, need);
  if (a.phase == 2)
    DRN_CHECK_ARG(pairs <= 0x7fffffffL && a.cnt_bytes >= pairs, "%s: the counts hold %d bytes, %ld are needed (8 * S * blocks)", what,
                  a.cnt_bytes, pairs);
  if (late) DRN_CHECK_ARG(a.S <= 65535, "%s: S = %d, more than 65535 sentences", what, a.S);
  else DRN_CHECK_ARG(cdiv(a.S, 16) <= 65535, "%s: S = %d, more than 65535 tiles of 16 sentences", what, a.S);
  return DRN_OK;
}

// the three launches with the operand Op -- of a phase, its one.  SHAPE is a compile-time switch: an operand instantiates only the
// kernels it is launched on
template <RkShape SHAPE, typename Op>
static void rk_launch(const Op op, const RkArgs& a, hipStream_t stream) {
  typedef typename Op::Q Q;
  const Q* q = (const Q*)a.queries;
  const int stride = a.allow ? a.allow_stride : 0;
  sl_key_t* tkey = a.phase ? a.keys : (sl_key_t*)a.ws;
  int2* cnt = a.phase ? a.cnt : (int2*)(tkey + a.S);
  const bool one = a.phase != 2, two = a.phase != 1;
  int nblocks = a.nblocks;
  if constexpr (SHAPE == RK_PLAIN) {
    nblocks = cdiv(a.V, RK_BLOCK);
    if (one) rank_target_kernel<Op><<<cdiv(a.S, 16), 64, 0, stream>>>(op, q, a.targets, a.allow, stride, a.V, a.E, a.S, tkey);
    if (two) rank_block_kernel<Op><<<dim3(nblocks, cdiv(a.S, 16)), 256, 0, stream>>>(op, q, a.allow, stride, a.V, a.E, a.S, nblocks, tkey, cnt);
  } else if constexpr (SHAPE == RK_RAGGED) {
    if (one) rank_target_rows_kernel<Op><<<a.S, 256, 0, stream>>>(op, q, nullptr, a.offsets, a.targets, a.allow, stride, a.R, a.V, a.E, 1, tkey);
    if (two)
      rank_segments_kernel<Op><<<dim3(nblocks, cdiv(a.S, 16)), 256, 0, stream>>>(op, q, a.offsets, a.blk_vid, a.allow, stride, a.R, a.V, a.E,
                                                                                  a.S, nblocks, tkey, cnt);
  } else {
    if (one)
      rank_target_rows_kernel<Op><<<a.S, 256, 0, stream>>>(op, q, a.lengths, a.offsets, a.targets, a.allow, stride, a.R, a.V, a.E, a.L, tkey);
    if (two)
      rank_late_kernel<Op><<<dim3(nblocks, a.S), 256, 0, stream>>>(op, q, a.lengths, a.offsets, a.blk_vid, a.allow, stride, a.R, a.V, a.E, a.L,
                                                                    nblocks, tkey, cnt);
  }
  if (a.phase == 0) rank_reduce_kernel<<<cdiv(a.S, 4), 256, 0, stream>>>(tkey, cnt, a.S, nblocks, a.rank, a.score, a.total);
}

template <RkShape SHAPE>
static int rk_run(const char* what, const RkArgs& a, void* stream) {
  drn_clear_status();
  if (const int rc = rk_check(what, a)) return rc;
  const uint8_t* codes = (const uint8_t*)a.table;
  const bool bf16 = a.dtype == DRN_BF16;
  // (a quantised bf16 chain keeps two scale blocks of loads in flight on the plain table, one on the ragged: retrieve_q8.hip says why)
  if (!a.scales && bf16) rk_launch<SHAPE>(AlPlain<bf16_t>{(const bf16_t*)a.table}, a, (hipStream_t)stream);
  else if (!a.scales) rk_launch<SHAPE>(AlPlain<float>{(const float*)a.table}, a, (hipStream_t)stream);
  else if (bf16) rk_launch<SHAPE>(AlQ8<bf16_t, SHAPE == RK_PLAIN ? 2 : 1>{codes, a.scales}, a, (hipStream_t)stream);
  else rk_launch<SHAPE>(AlQ8<float, 1>{codes, a.scales}, a, (hipStream_t)stream);
  return drn_launch_status(what);
}

extern "C" int drn_shortlist_rank(const void* table, const uint8_t* scales, const void* queries, const int32_t* targets, const int32_t* allow,
                                  int allow_stride, int V, int E, int S, int dtype, void* ws, int ws_bytes, int32_t* rank, float* score,
                                  int32_t* total, void* stream) {
  const RkArgs a = {RK_PLAIN, table, scales, queries, nullptr, nullptr, nullptr, targets, allow, allow_stride, 0, V, 0, E, S, 1, dtype, ws,
                    ws_bytes, rank, score, total};
  return rk_run<RK_PLAIN>("drn_shortlist_rank", a, stream);
}

extern "C" int drn_shortlist_segments_rank(const void* table, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                           const int32_t* blk_vid, const int32_t* targets, const int32_t* allow, int allow_stride, int R,
                                           int V, int nblocks, int E, int S, int dtype, void* ws, int ws_bytes, int32_t* rank, float* score,
                                           int32_t* total, void* stream) {
  const RkArgs a = {RK_RAGGED, table, scales, queries, nullptr, offsets, blk_vid, targets, allow, allow_stride, R, V, nblocks, E, S, 1, dtype,
                    ws, ws_bytes, rank, score, total};
  return rk_run<RK_RAGGED>("drn_shortlist_segments_rank", a, stream);
}

extern "C" int drn_shortlist_late_rank(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths,
                                       const int32_t* offsets, const int32_t* blk_vid, const int32_t* targets, const int32_t* allow,
                                       int allow_stride, int R, int V, int nblocks, int E, int S, int L, int dtype, void* ws, int ws_bytes,
                                       int32_t* rank, float* score, int32_t* total, void* stream) {
  const RkArgs a = {RK_LATE, table, scales, queries, lengths, offsets, blk_vid, targets, allow, allow_stride, R, V, nblocks, E, S, L, dtype,
                    ws, ws_bytes, rank, score, total};
  return rk_run<RK_LATE>("drn_shortlist_late_rank", a, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The phases alone, for a corpus kept as several tables (retrieve_shard_rank.hip says why a shard's counting kernel gives the corpus's
// count when it is handed a per-shard threshold in the place of tkey[s]).  phase 1: the target kernel of the matching entry above
// writes keys [S] (cnt is not used and may be null); phase 2: its counting kernel reads keys [S] as THRESHOLDS and writes cnt [S][blocks]
// pairs, cnt_bytes >= 8 S blocks (targets is not used and may be null).  One launch each; the kernels and their bits are the entries'.
// In a phase the record's slots from ws on hold: no workspace and no results (the reduce does not run), the phase, keys, cnt, cnt_bytes.

extern "C" int drn_shortlist_rank_phase(const void* table, const uint8_t* scales, const void* queries, const int32_t* targets,
                                        const int32_t* allow, int allow_stride, int V, int E, int S, int dtype, int phase, void* keys,
                                        void* cnt, int cnt_bytes, void* stream) {
  const char* what = "drn_shortlist_rank_phase";
  drn_clear_status();
  DRN_CHECK_ARG(phase == 1 || phase == 2, "%s: phase = %d is neither 1 (the target keys) nor 2 (the block counts)", what, phase);
  const RkArgs a = {RK_PLAIN, table, scales, queries, nullptr, nullptr, nullptr, targets, allow, allow_stride, 0, V, 0, E, S, 1, dtype, nullptr,
                    0, nullptr, nullptr, nullptr, phase, (sl_key_t*)keys, (int2*)cnt, cnt_bytes};
  return rk_run<RK_PLAIN>(what, a, stream);
}

extern "C" int drn_shortlist_segments_rank_phase(const void* table, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                                 const int32_t* blk_vid, const int32_t* targets, const int32_t* allow, int allow_stride,
                                                 int R, int V, int nblocks, int E, int S, int dtype, int phase, void* keys, void* cnt,
                                                 int cnt_bytes, void* stream) {
  const char* what = "drn_shortlist_segments_rank_phase";
  drn_clear_status();
  DRN_CHECK_ARG(phase == 1 || phase == 2, "%s: phase = %d is neither 1 (the target keys) nor 2 (the block counts)", what, phase);
  const RkArgs a = {RK_RAGGED, table, scales, queries, nullptr, offsets, blk_vid, targets, allow, allow_stride, R, V, nblocks, E, S, 1, dtype,
                    nullptr, 0, nullptr, nullptr, nullptr, phase, (sl_key_t*)keys, (int2*)cnt, cnt_bytes};
  return rk_run<RK_RAGGED>(what, a, stream);
}

extern "C" int drn_shortlist_late_rank_phase(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths,
                                             const int32_t* offsets, const int32_t* blk_vid, const int32_t* targets, const int32_t* allow,
                                             int allow_stride, int R, int V, int nblocks, int E, int S, int L, int dtype, int phase,
                                             void* keys, void* cnt, int cnt_bytes, void* stream) {
  const char* what = "drn_shortlist_late_rank_phase";
  drn_clear_status();
  DRN_CHECK_ARG(phase == 1 || phase == 2, "%s: phase = %d is neither 1 (the target keys) nor 2 (the block counts)", what, phase);
  const RkArgs a = {RK_LATE, table, scales, queries, lengths, offsets, blk_vid, targets, allow, allow_stride, R, V, nblocks, E, S, L, dtype,
                    nullptr, 0, nullptr, nullptr, nullptr, phase, (sl_key_t*)keys, (int2*)cnt, cnt_bytes};
  return rk_run<RK_LATE>(what, a, stream);
}
