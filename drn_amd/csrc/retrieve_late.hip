// The shortlist by LATE INTERACTION (drn_amd/retrieve.py, Shortlister.shortlist_late): a sentence is L token vectors of which the first
// lengths[s] are live, a video is its ragged run of segment rows, and
//   score[s][v] = sum over the live tokens t of   max over the rows r of v of   q[s][t] . emb[r]
//   drn_shortlist_late_topn / drn_shortlist_late_topn_q8   each sentence's best n videos by that score, under the total order of retrieve.hip.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// ONE (token, row) dot product is the accumulator element of the chain shortlist_segments_kernel runs (retrieve_seg.hip: the block plan,
// the passes, the segmented maximum and the states are described there) -- the table operand's scores(), AlPlain / AlQ8 of shortlist.h
// -- and sim[s][t][v] is that kernel's segmented maximum, so a sim has the bits drn_shortlist_segments_topn gives the (query row, video)
// pair.  What is new is the FOLD over a sentence's tokens inside the ranking workgroup.
//
// Workgroup (b, s) owns block b of the plan and sentence s.  Lt = lengths[s] clamped into [0, L] is read here, on the device.  The live
// tokens are walked in TILES of 16: the 16 token rows are the A operand of the chain (a slot past Lt reads the last live token's row
// instead, as a sentence slot past S does elsewhere; its scores are never folded), the block's rows go by in passes of LT_BLOCK into sc,
// and the segmented maximum folds each pass into the states [token of the tile][video of the block].  After the tile's last pass ONE
// thread per video adds the tile's live tokens to the video's fp32 sum in ascending t -- ((0 + sim_0) + sim_1) + ..., plain adds; a NaN
// state is a NaN term and an infinity stays one, so what is not finite carries through by itself -- and clears the video's states for
// the next tile.  The trip count is ceil(Lt / 16): workgroup-uniform, and it follows lengths, not L, so padding costs nothing.  After
// the last tile a video becomes the key (sum, ~video), or 0 when it has no rows, Lt is 0, the sum is not finite or its mask bit is clear;
// ONE row of 16, 64 or 256 keys is sorted and its first m = min(n, LT_BLOCK) go to ws[s][b][0..m).  Phase two is shortlist_merge_kernel
// of retrieve.hip as it stands: a video lies in one block, so no video reaches it twice.  Two launches, no atomics, no tickets.
//
// A (sentence, video) sum depends on that sentence's live tokens and that video's rows alone: the lanes per pair (P, from the block's
// longest run) only regroup an exact maximum, the token order of the adds is fixed, and the mask and the other videos enter after it.
//
// The block's rows are read once per (sentence, token tile) -- from L2 / Infinity Cache after the first -- which is the known cost of
// this shape.  As in retrieve_seg.hip every index read from a device table is clamped.
#define LT_BLOCK 256        // = SG_BLOCK = _lib.SHORTLIST_SEG_BLOCK: videos of a block at most, rows of a pass
#define LT_LD (LT_BLOCK + 1)

template <typename Op>
__global__ __launch_bounds__(256) void shortlist_late_kernel(const Op op, const typename Op::Q* __restrict__ q, const int* __restrict__ lengths,
                                                             const int* __restrict__ offsets, const int* __restrict__ blk_vid,
                                                             const int* __restrict__ allow, const int allow_stride, const int R, const int V,
                                                             const int E, const int L, const int m, const int nblocks,
                                                             sl_key_t* __restrict__ ws) {
  __shared__ sl_key_t keys[16 * LT_BLOCK];                    // 32 KiB: [token of the tile][video of the block] states; at the end one row of keys
  __shared__ float sc[16 * LT_LD];                            // [token of the tile][row of the pass]
  __shared__ int voff[LT_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ float sums[LT_BLOCK];                            // each video's running sum over the tokens
  __shared__ int wlong[4];                                    // each wave's longest run
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s = blockIdx.y;
  const int r = lane & 15, g = lane >> 4;
  const int Lt = min(max(lengths[s], 0), L);
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + LT_BLOCK, V)), nv = v1 - v0;
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // states per token and keys: 16, 64 or 256 >= nv
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
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), LT_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (token, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  for (int t0 = 0; t0 < Lt; t0 += 16) {                       // (workgroup-uniform: Lt is the sentence's)
    const int live = min(16, Lt - t0);
    // (a token slot past Lt reads the last live token instead: nobody folds its scores)
    const typename Op::Q* qrow = q + ((long)s * L + min(t0 + r, Lt - 1)) * E;
    for (int p0 = r0; p0 < r1; p0 += LT_BLOCK) {
      const int p1 = min(p0 + LT_BLOCK, r1), rw = p0 + wave * 64;
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
          for (int i = 0; i < 4; ++i) sc[(4 * g + i) * LT_LD + wave * 64 + 16 * j + r] = acc[j][i];
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
        const float* mine = sc + tl * LT_LD;
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
    // the fold: the video's thread adds the tile's live tokens in ascending t and clears their states.  The ordered word of a NaN is
    // all ones and sl_score makes a NaN of it again; those of the infinities become the infinities.  (A video without rows has no
    // state and becomes no key below: what its sum holds is never read.)
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
  // sums -> ONE row of keys (every state is zero again: the row is written whole).  sl_key makes no key of a sum that is not finite; the
  // mask enters here: a video whose bit is clear becomes no key.  (v < V: its word lies inside the mask's row.)
  for (int vi = tid; vi < len; vi += 256) {
    bool ok = vi < nv && Lt > 0;
    if (ok) {
      const int v = v0 + vi;
      ok = voff[vi + 1] > voff[vi] && (allow == nullptr || ((allow[(long)s * allow_stride + (v >> 5)] >> (v & 31)) & 1));
    }
    keys[vi] = ok ? sl_key(sums[vi], v0 + vi) : 0ull;
  }
  __syncthreads();
  if (lenlg == 4) sl_sort_desc<16, 256>(keys, 1, tid);        // (block-uniform)
  else if (lenlg == 6) sl_sort_desc<64, 256>(keys, 1, tid);
  else sl_sort_desc<LT_BLOCK, 256>(keys, 1, tid);
  for (int i = tid; i < m; i += 256) ws[((long)s * nblocks + b) * m + i] = i < len ? keys[i] : 0ull;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The entries: one argument record, one list of checks, one launch switch.

struct LtArgs {
  bool q8;                                                    // scales is read
  const void* table;                                          // emb, or the codes
  const void* scales;
  const void* queries;
  const int32_t *lengths, *offsets, *blk_vid, *allow;         // (allow may be null: no mask)
  int allow_stride, R, V, nblocks, E, S, L, n, dtype;
  void* ws;
  int ws_keys;
  int32_t* ids;
  float* scores;
  int32_t* counts;
};

static int lt_check(const char* what, const LtArgs& a) {
  DRN_CHECK_ARG(a.table && (!a.q8 || a.scales) && a.queries && a.lengths && a.offsets && a.blk_vid && a.ws && a.ids && a.scores && a.counts,
                "%s: null pointer", what);
  DRN_CHECK_ARG(a.R >= 1 && a.V >= 1 && a.E >= 1 && a.S >= 1, "%s: bad args (R = %d rows, V = %d videos, E = %d columns, S = %d sentences)", what,
                a.R, a.V, a.E, a.S);
  DRN_CHECK_ARG(a.L >= 1 && a.L <= DRN_LATE_MAX_TOKENS, "%s: L = %d tokens outside [1, %d]", what, a.L, DRN_LATE_MAX_TOKENS);
  if (a.q8) DRN_CHECK_ARG(a.E % MX8_BLOCK == 0, "%s: E = %d is not a multiple of the block of %d columns", what, a.E, MX8_BLOCK);
  DRN_CHECK_ARG(a.nblocks >= 1 && a.nblocks <= a.V && (long)a.nblocks * LT_BLOCK >= a.V, "%s: %d blocks outside [ceil(V / %d), V] for V = %d videos",
                what, a.nblocks, LT_BLOCK, a.V);
  DRN_CHECK_ARG(a.n >= 1 && a.n <= DRN_SHORTLIST_MAX, "%s: n = %d outside [1, %d]", what, a.n, DRN_SHORTLIST_MAX);
  DRN_CHECK_ARG(a.dtype == DRN_F32 || a.dtype == DRN_BF16, "%s: dtype %d (float32 / bfloat16 only)", what, a.dtype);
  // (the chain loads 16 bytes at once only where E makes every row, a token's among them, a multiple of 16 bytes)
  DRN_CHECK_ARG(((uintptr_t)a.table & 15) == 0 && ((uintptr_t)a.queries & 15) == 0 && ((uintptr_t)a.ws & 7) == 0,
                "%s: the table and the queries must be 16-byte aligned, the workspace 8-byte aligned", what);
  DRN_CHECK_ARG(((uintptr_t)a.lengths & 3) == 0, "%s: lengths must be 4-byte aligned", what);
  if (a.allow) {
    DRN_CHECK_ARG(a.allow_stride == 0 || a.allow_stride == cdiv(a.V, 32),
                  "%s: allow_stride = %d is neither 0 (one mask for all sentences) nor ceil(V / 32) = %d (one row per sentence)", what,
                  a.allow_stride, cdiv(a.V, 32));
    DRN_CHECK_ARG(((uintptr_t)a.allow & 3) == 0, "%s: the mask must be 4-byte aligned", what);
  }
  const int m = a.n < LT_BLOCK ? a.n : LT_BLOCK;
  const long need = (long)a.S * a.nblocks * m;
  DRN_CHECK_ARG(need <= 0x7fffffffL && a.ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (S * blocks * min(n, %d))", what,
                a.ws_keys, need, LT_BLOCK);
  DRN_CHECK_ARG(a.S <= 65535, "%s: S = %d, more than 65535 sentences", what, a.S);
  return DRN_OK;
}

// phase one with the operand Op, then the merge of the other shortlists
template <typename Op>
static void lt_launch(const Op op, const LtArgs& a, hipStream_t stream) {
  typedef typename Op::Q Q;
  const int m = a.n < LT_BLOCK ? a.n : LT_BLOCK;
  const dim3 grid(a.nblocks, a.S);
  sl_key_t* lists = (sl_key_t*)a.ws;
  shortlist_late_kernel<Op><<<grid, 256, 0, stream>>>(op, (const Q*)a.queries, a.lengths, a.offsets, a.blk_vid, a.allow,
                                                       a.allow ? a.allow_stride : 0, a.R, a.V, a.E, a.L, m, a.nblocks, lists);
  sl_launch_merge(lists, a.S, a.n, m, a.nblocks, a.ids, a.scores, a.counts, stream);
}

static int lt_run(const char* what, const LtArgs& a, void* stream) {
  drn_clear_status();
  if (const int rc = lt_check(what, a)) return rc;
  const uint8_t *codes = (const uint8_t*)a.table, *scales = (const uint8_t*)a.scales;
  const bool bf16 = a.dtype == DRN_BF16;
  // (a quantised chain keeps one scale block of loads in flight, as the ragged kernels of retrieve_q8.hip and retrieve_allow.hip do)
  if (!a.q8 && bf16) lt_launch(AlPlain<bf16_t>{(const bf16_t*)a.table}, a, (hipStream_t)stream);
  else if (!a.q8) lt_launch(AlPlain<float>{(const float*)a.table}, a, (hipStream_t)stream);
  else if (bf16) lt_launch(AlQ8<bf16_t, 1>{codes, scales}, a, (hipStream_t)stream);
  else lt_launch(AlQ8<float, 1>{codes, scales}, a, (hipStream_t)stream);
  return drn_launch_status(what);
}

extern "C" int drn_shortlist_late_topn(const void* emb, const void* queries, const int32_t* lengths, const int32_t* offsets,
                                       const int32_t* blk_vid, const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S,
                                       int L, int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts,
                                       void* stream) {
  const LtArgs a = {false, emb, nullptr, queries, lengths, offsets, blk_vid, allow, allow_stride, R, V, nblocks, E, S, L, n, dtype, ws, ws_keys,
                    ids, scores, counts};
  return lt_run("drn_shortlist_late_topn", a, stream);
}

extern "C" int drn_shortlist_late_topn_q8(const uint8_t* codes, const uint8_t* scales, const void* queries, const int32_t* lengths,
                                          const int32_t* offsets, const int32_t* blk_vid, const int32_t* allow, int allow_stride, int R, int V,
                                          int nblocks, int E, int S, int L, int n, int dtype, void* ws, int ws_keys, int32_t* ids,
                                          float* scores, int32_t* counts, void* stream) {
  const LtArgs a = {true, codes, scales, queries, lengths, offsets, blk_vid, allow, allow_stride, R, V, nblocks, E, S, L, n, dtype, ws, ws_keys,
                    ids, scores, counts};
  return lt_run("drn_shortlist_late_topn_q8", a, stream);
}
