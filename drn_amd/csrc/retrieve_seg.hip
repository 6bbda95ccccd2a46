// The shortlist over a RAGGED table (drn_amd/retrieve.py, Shortlister(offsets=)): video v owns the rows offsets[v] .. offsets[v + 1] - 1
// of an (R, E) table of segment embeddings, its score is the score of its best row, and the list names which row that was.
//   drn_shortlist_segments_topn   each sentence's best n videos by their best segment, under the total order of retrieve.hip.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// score[s][v] = max over the rows r of v of sum_e q[s][e] * emb[r][e]; rows[s][v] = the lowest r - offsets[v] that reaches it.  ONE
// (s, r) dot product is the accumulator element of the same chain of MFMAs over the same K-steps as in shortlist_block_kernel
// (retrieve.hip), so its bits depend on the row and the query alone -- not on the offsets, V, S, n, the pass or the grid -- and with one
// row per video the scores are that kernel's.
//
// The BLOCK PLAN is made on the host once (retrieve.plan_segment_blocks): block b holds the videos blk_vid[b] .. blk_vid[b + 1] - 1, at
// most SG_BLOCK of them, every video whole inside one block.  Phase one (shortlist_segments_kernel): workgroup (b, t) walks its block's
// rows in passes of SG_BLOCK against the 16 sentences of tile t.  A pass leaves its 16 x SG_BLOCK scores in LDS and then folds each
// video's rows of that pass into the video's STATE, a 64-bit word: the score as an ordered unsigned word (NaN above everything, so that
// it sticks) above the complement of the segment number.  The maximum of such words is the best score and, among equal scores, the
// lowest segment.  A (sentence, video) pair belongs to P adjacent lanes, P a power of two up to 16 chosen per block from its longest
// run (one lane per 16 rows of it): each lane scans its share of the run, the P words meet in a butterfly of lane exchanges, and lane 0
// of the group is the pair's ONE writer in every pass: no atomics.  Then the states become (score, ~video) keys -- 0 for a video
// without rows, a score that is not finite, a sentence past S -- at a stride of 16, 64 or 256 keys per sentence, the smallest that holds
// the block's videos, so that the shared sort orders no more keys than the block can have; the first m = min(n, SG_BLOCK) go to
// ws[s][b][0..m) with their winning segments beside them in wsr.
// Phase two is shortlist_merge_kernel of retrieve.hip as it stands: a video lies in one block, so no video reaches it twice.
// Phase three (shortlist_segment_rows_kernel): one thread per listed (sentence, place) finds its video's key in the list of the
// video's block (vid_blk) and copies the segment.  Three launches, no atomics, no tickets.
//
// The tables come from the device and cannot be checked here without a synchronise: every index read from them is clamped, so a bad
// table gives a wrong list and never an access outside emb, ws or the tables themselves.
#define SG_BLOCK 256        // videos of a block at most, rows of a pass (= _lib.SHORTLIST_SEG_BLOCK)
#define SG_LD (SG_BLOCK + 1) // a sentence's scores of a pass, padded: the 16 sentences of one row fall in 16 banks

template <typename T>
__global__ __launch_bounds__(256) void shortlist_segments_kernel(const T* __restrict__ emb, const T* __restrict__ q,
                                                                 const int* __restrict__ offsets, const int* __restrict__ blk_vid,
                                                                 const int R, const int V, const int E, const int S, const int m,
                                                                 const int nblocks, sl_key_t* __restrict__ ws, int* __restrict__ wsr) {
  __shared__ sl_key_t keys[16 * SG_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block], states then keys
  __shared__ float sc[16 * SG_LD];                            // [sentence of the tile][row of the pass]; after the last pass, as
  int* const seg = reinterpret_cast<int*>(sc);                // integers, the winning segment of [sentence][video]
  __shared__ int voff[SG_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words (a multiple of 16 bytes)
  __shared__ int wlong[4];                                    // each wave's longest run
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16;
  const int r = lane & 15, g = lane >> 4;
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + SG_BLOCK, V)), nv = v1 - v0;
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // keys per sentence: 16, 64 or 256 >= nv
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
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), SG_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (sentence, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  // (a sentence past S reads the last one instead: its states become no keys below)
  const T* qrow = q + (long)min(s0 + r, S - 1) * E;
  constexpr int COLS = SlStep<T>::COLS, PER_LANE = SlStep<T>::PER_LANE;
  const int whole = E % PER_LANE == 0 ? E / COLS * COLS : 0;
  for (int p0 = r0; p0 < r1; p0 += SG_BLOCK) {
    const int p1 = min(p0 + SG_BLOCK, r1), rw = p0 + wave * 64;
    if (rw < p1) {                                            // (wave-uniform: a wave whose 64 rows lie past the block reads nothing)
      // (a row past the block reads the table's last row instead: nobody folds its score)
      const T* erow[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) erow[j] = emb + (long)min(rw + 16 * j + r, R - 1) * E;
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      int c = 0;
      for (; c < whole; c += COLS) {
        const int c0 = c + g * PER_LANE;
        const auto a = sl_frag(qrow, c0);
        decltype(sl_frag(qrow, c0)) bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = sl_frag(erow[j], c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = sl_mfma(a, bv[j], acc[j]);
      }
      for (; c < E; c += COLS) {
        const int c0 = c + g * PER_LANE;
        const auto a = sl_frag_tail(qrow, c0, E);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = sl_mfma(a, sl_frag_tail(erow[j], c0, E), acc[j]);
      }
      // C/D: column (row of the table) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[(4 * g + i) * SG_LD + wave * 64 + 16 * j + r] = acc[j][i];
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
      const float* mine = sc + sl * SG_LD;
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
  // states -> keys.  An ordered word is a finite score's between those of -inf and +inf; 0 is a video without rows.
  for (int p = tid; p < 16 * len; p += 256) {
    const int sl = p >> lenlg, vi = p & (len - 1);
    const sl_key_t st = keys[p];
    const unsigned o = (unsigned)(st >> 32);
    const bool ok = vi < nv && s0 + sl < S && o > 0x007fffffu && o < 0xff800000u;
    seg[p] = (int)~(unsigned)st;
    keys[p] = ok ? ((sl_key_t)o << 32) | (sl_key_t)(~(unsigned)(v0 + vi)) : 0ull;
  }
  __syncthreads();
  if (lenlg == 4) sl_sort_desc<16, 256>(keys, 16, tid);       // (block-uniform)
  else if (lenlg == 6) sl_sort_desc<64, 256>(keys, 16, tid);
  else sl_sort_desc<SG_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    const sl_key_t k = i < len ? keys[sl * len + i] : 0ull;
    const long at = ((long)(s0 + sl) * nblocks + b) * m + i;
    ws[at] = k;
    wsr[at] = k != 0ull ? seg[sl * len + (sl_video(k) - v0)] : -1;
  }
}

__global__ __launch_bounds__(256) void shortlist_segment_rows_kernel(const sl_key_t* __restrict__ ws, const int* __restrict__ wsr,
                                                                     const int* __restrict__ vid_blk, const int* __restrict__ ids,
                                                                     const int V, const int total, const int n, const int m,
                                                                     const int nblocks, int* __restrict__ rows) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int s = idx / n, v = ids[idx];
  int row = -1;
  if (v >= 0 && v < V) {
    const int b = min(max(vid_blk[v], 0), nblocks - 1);
    const long at = ((long)s * nblocks + b) * m;
    // (the low word of a key is its video's: one key of the list at most has it, and the empty key 0 has nobody's)
    for (int i = 0; i < m; ++i)
      if ((unsigned)ws[at + i] == ~(unsigned)v) {
        row = wsr[at + i];
        break;
      }
  }
  rows[idx] = row;
}

// (declared in shortlist.h: retrieve_q8.hip's lists are looked up by the same kernel; not part of the C ABI)
void sl_launch_segment_rows(const sl_key_t* ws, const int* wsr, const int32_t* vid_blk, const int32_t* ids, int V, int S, int n, int m,
                            int nblocks, int32_t* rows, hipStream_t stream) {
  shortlist_segment_rows_kernel<<<cdiv(S * n, 256), 256, 0, stream>>>(ws, wsr, vid_blk, ids, V, S * n, n, m, nblocks, rows);
}

extern "C" int drn_shortlist_segments_topn(const void* emb, const void* queries, const int32_t* offsets, const int32_t* blk_vid,
                                           const int32_t* vid_blk, int R, int V, int nblocks, int E, int S, int n, int dtype, void* ws,
                                           int ws_keys, int32_t* ids, float* scores, int32_t* counts, int32_t* rows, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(emb && queries && offsets && blk_vid && vid_blk && ws && ids && scores && counts && rows,
                "drn_shortlist_segments_topn: null pointer");
  DRN_CHECK_ARG(R >= 1 && V >= 1 && E >= 1 && S >= 1,
                "drn_shortlist_segments_topn: bad args (R = %d rows, V = %d videos, E = %d columns, S = %d sentences)", R, V, E, S);
  DRN_CHECK_ARG(nblocks >= 1 && nblocks <= V && (long)nblocks * SG_BLOCK >= V,
                "drn_shortlist_segments_topn: %d blocks outside [ceil(V / %d), V] for V = %d videos", nblocks, SG_BLOCK, V);
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_MAX, "drn_shortlist_segments_topn: n = %d outside [1, %d]", n, DRN_SHORTLIST_MAX);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "drn_shortlist_segments_topn: dtype %d (float32 / bfloat16 only)", dtype);
  DRN_CHECK_ARG(((uintptr_t)emb & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)ws & 7) == 0,
                "drn_shortlist_segments_topn: the table and the queries must be 16-byte aligned, the workspace 8-byte aligned");
  const int m = n < SG_BLOCK ? n : SG_BLOCK, tiles = cdiv(S, 16);
  const long lists = (long)S * nblocks * m, need = lists + (lists + 1) / 2;
  DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need,
                "drn_shortlist_segments_topn: the workspace holds %d keys, %ld are needed (1.5 * S * blocks * min(n, %d))", ws_keys, need, SG_BLOCK);
  DRN_CHECK_ARG(tiles <= 65535, "drn_shortlist_segments_topn: S = %d, more than 65535 tiles of 16 sentences", S);
  sl_key_t* lists_k = (sl_key_t*)ws;
  int* lists_r = (int*)(lists_k + lists);
  const dim3 grid(nblocks, tiles);
  if (dtype == DRN_BF16)
    shortlist_segments_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)emb, (const bf16_t*)queries, offsets, blk_vid, R,
                                                                             V, E, S, m, nblocks, lists_k, lists_r);
  else
    shortlist_segments_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)emb, (const float*)queries, offsets, blk_vid, R, V,
                                                                            E, S, m, nblocks, lists_k, lists_r);
  sl_launch_merge(lists_k, S, n, m, nblocks, ids, scores, counts, (hipStream_t)stream);
  sl_launch_segment_rows(lists_k, lists_r, vid_blk, ids, V, S, n, m, nblocks, rows, (hipStream_t)stream);
  return drn_launch_status("drn_shortlist_segments_topn");
}
