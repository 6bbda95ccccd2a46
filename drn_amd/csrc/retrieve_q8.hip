// The shortlist over a table kept in block-scaled FP8 (drn_amd/retrieve.py, Shortlister(quantize="mxfp8") / Shortlister.from_mx8):
//   drn_shortlist_topn_q8            drn_shortlist_topn (retrieve.hip) with the (V, E) table as codes (V, E) u8 + scales (V, E / 32) u8;
//   drn_shortlist_segments_topn_q8   drn_shortlist_segments_topn (retrieve_seg.hip) with the ragged (R, E) table in the same layout.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// The format is drn_amd/index.py mx8_quantize: OCP e4m3fn codes, one power-of-two scale byte (e8m0) per 32 columns, E + E / 32 bytes
// a row.  A dequantised value, float(code) * 2^(scale - 127), is EXACT in fp32 and in bf16.  Phase one here is the plain kernel's phase
// one with the table fragment built from codes (sl_codes_q8 / sl_frag_q8, shortlist.h) instead of loaded: the same grid, the same
// 16-sentence x 64-rows-per-wave tiles, the same K-steps in ascending order through the same sl_mfma chain per (sentence, row), the
// query operand loaded as there.  So the lists are BIT FOR BIT those of the plain kernels over the dequantised table.
//
// Step k of a bf16 chain (32 columns) lies inside scale block k: lane group g reads the 8 code bytes of columns 32 k + 8 g .. + 7.
// Step k of an fp32 chain (16 columns) lies inside scale block k >> 1: lane group g reads the 4 code bytes of columns 16 k + 4 g .. + 3.
// The scale byte is fetched singly, per row and step: the 16 lanes of a row's four groups read the same byte, a row's scale bytes of
// all steps lie in one or two cache lines, and a word covering several steps would need E / 32 to be a multiple of 4.  The loads of
// two steps are in flight in the plain ranking kernel (sq_blocks: two blocks of a bf16 chain, an odd last block alone; the one block of
// two fp32 steps, which share their scale byte).  The segmented bf16 kernel keeps ONE block in flight: with two the compiler takes 172
// registers, over the cap of 128 the plain kernels are held to.  E % 32 == 0 is required: there is no tail.
//
// Everything after the scores -- the keys and the sort, the segmented maximum, the merge (sl_launch_merge) and the segment look-up
// (sl_launch_segment_rows) -- is the plain kernels' code; the two phase-one bodies are repeated here because retrieve.hip and
// retrieve_seg.hip are held to their kernel counts and resource notes by their tests.
#define SQ_BLOCK 256        // = SL_BLOCK (retrieve.hip) = SG_BLOCK (retrieve_seg.hip) = _lib.SHORTLIST_BLOCK = _lib.SHORTLIST_SEG_BLOCK
#define SQ_LD (SQ_BLOCK + 1)

// (sq_blocks / sq_scores, the scores of a tile from codes and scale bytes: shortlist.h, shared with retrieve_allow.hip)

template <typename T>
__global__ __launch_bounds__(256) void shortlist_block_q8_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                                 const T* __restrict__ q, const int V, const int E, const int S,
                                                                 const int m, const int nblocks, sl_key_t* __restrict__ ws) {
  __shared__ sl_key_t keys[16 * SQ_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, v0 = b * SQ_BLOCK + wave * 64;
  const int r = lane & 15, g = lane >> 4;
  // (a row past S or V reads the last row instead: its scores become no keys below)
  const T* qrow = q + (long)min(s0 + r, S - 1) * E;
  const uint8_t* crow[4];
  const uint8_t* srow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long row = min(v0 + 16 * j + r, V - 1);
    crow[j] = codes + row * E;
    srow[j] = scales + row * (E / MX8_BLOCK);
  }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  sq_scores<T, SlStep<T>::COLS / 16>(qrow, crow, srow, E, g, acc);          // (two steps of loads in flight)
  // C/D: column (video) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = v0 + 16 * j + r, sl = 4 * g + i;
      keys[sl * SQ_BLOCK + wave * 64 + 16 * j + r] = (v < V && s0 + sl < S) ? sl_key(acc[j][i], v) : 0ull;
    }
  __syncthreads();
  sl_sort_desc<SQ_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    ws[((long)(s0 + sl) * nblocks + b) * m + i] = keys[sl * SQ_BLOCK + i];
  }
}

// shortlist_segments_kernel (retrieve_seg.hip: the block plan, the passes, the segmented maximum, the states and the keys are described
// there) with the scores of a pass from sq_scores.  As there, every index read from the device tables is clamped.
template <typename T>
__global__ __launch_bounds__(256) void shortlist_segments_q8_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                                    const T* __restrict__ q, const int* __restrict__ offsets,
                                                                    const int* __restrict__ blk_vid, const int R, const int V,
                                                                    const int E, const int S, const int m, const int nblocks,
                                                                    sl_key_t* __restrict__ ws, int* __restrict__ wsr) {
  __shared__ sl_key_t keys[16 * SQ_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block], states then keys
  __shared__ float sc[16 * SQ_LD];                            // [sentence of the tile][row of the pass]; after the last pass, as
  int* const seg = reinterpret_cast<int*>(sc);                // integers, the winning segment of [sentence][video]
  __shared__ int voff[SQ_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ int wlong[4];                                    // each wave's longest run
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16;
  const int r = lane & 15, g = lane >> 4;
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + SQ_BLOCK, V)), nv = v1 - v0;
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
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), SQ_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (sentence, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  // (a sentence past S reads the last one instead: its states become no keys below)
  const T* qrow = q + (long)min(s0 + r, S - 1) * E;
  for (int p0 = r0; p0 < r1; p0 += SQ_BLOCK) {
    const int p1 = min(p0 + SQ_BLOCK, r1), rw = p0 + wave * 64;
    if (rw < p1) {                                            // (wave-uniform: a wave whose 64 rows lie past the block reads nothing)
      // (a row past the block reads the table's last row instead: nobody folds its score)
      const uint8_t* crow[4];
      const uint8_t* srow[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long row = min(rw + 16 * j + r, R - 1);
        crow[j] = codes + row * E;
        srow[j] = scales + row * (E / MX8_BLOCK);
      }
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      sq_scores<T, 1>(qrow, crow, srow, E, g, acc);
      // C/D: column (row of the table) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[(4 * g + i) * SQ_LD + wave * 64 + 16 * j + r] = acc[j][i];
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
      const float* mine = sc + sl * SQ_LD;
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
  else sl_sort_desc<SQ_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    const sl_key_t k = i < len ? keys[sl * len + i] : 0ull;
    const long at = ((long)(s0 + sl) * nblocks + b) * m + i;
    ws[at] = k;
    wsr[at] = k != 0ull ? seg[sl * len + (sl_video(k) - v0)] : -1;
  }
}

extern "C" int drn_shortlist_topn_q8(const uint8_t* codes, const uint8_t* scales, const void* queries, int V, int E, int S, int n, int dtype,
                                     void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(codes && scales && queries && ws && ids && scores && counts, "drn_shortlist_topn_q8: null pointer");
  DRN_CHECK_ARG(V >= 1 && E >= 1 && S >= 1, "drn_shortlist_topn_q8: bad args (V = %d videos, E = %d columns, S = %d sentences)", V, E, S);
  DRN_CHECK_ARG(E % MX8_BLOCK == 0, "drn_shortlist_topn_q8: E = %d is not a multiple of the block of %d columns", E, MX8_BLOCK);
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_MAX, "drn_shortlist_topn_q8: n = %d outside [1, %d]", n, DRN_SHORTLIST_MAX);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "drn_shortlist_topn_q8: dtype %d (float32 / bfloat16 queries only)", dtype);
  DRN_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)ws & 7) == 0,
                "drn_shortlist_topn_q8: the codes and the queries must be 16-byte aligned, the workspace 8-byte aligned");
  const int m = n < SQ_BLOCK ? n : SQ_BLOCK, nblocks = cdiv(V, SQ_BLOCK), tiles = cdiv(S, 16);
  const long need = (long)S * nblocks * m;
  DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need,
                "drn_shortlist_topn_q8: the workspace holds %d keys, %ld are needed (S * ceil(V / %d) * min(n, %d))", ws_keys, need, SQ_BLOCK,
                SQ_BLOCK);
  DRN_CHECK_ARG(tiles <= 65535, "drn_shortlist_topn_q8: S = %d, more than 65535 tiles of 16 sentences", S);
  const dim3 grid(nblocks, tiles);
  if (dtype == DRN_BF16)
    shortlist_block_q8_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>(codes, scales, (const bf16_t*)queries, V, E, S, m, nblocks,
                                                                             (sl_key_t*)ws);
  else
    shortlist_block_q8_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(codes, scales, (const float*)queries, V, E, S, m, nblocks,
                                                                            (sl_key_t*)ws);
  sl_launch_merge((const sl_key_t*)ws, S, n, m, nblocks, ids, scores, counts, (hipStream_t)stream);
  return drn_launch_status("drn_shortlist_topn_q8");
}

extern "C" int drn_shortlist_segments_topn_q8(const uint8_t* codes, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                              const int32_t* blk_vid, const int32_t* vid_blk, int R, int V, int nblocks, int E, int S, int n,
                                              int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, int32_t* rows,
                                              void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(codes && scales && queries && offsets && blk_vid && vid_blk && ws && ids && scores && counts && rows,
                "drn_shortlist_segments_topn_q8: null pointer");
  DRN_CHECK_ARG(R >= 1 && V >= 1 && E >= 1 && S >= 1,
                "drn_shortlist_segments_topn_q8: bad args (R = %d rows, V = %d videos, E = %d columns, S = %d sentences)", R, V, E, S);
  DRN_CHECK_ARG(E % MX8_BLOCK == 0, "drn_shortlist_segments_topn_q8: E = %d is not a multiple of the block of %d columns", E, MX8_BLOCK);
  DRN_CHECK_ARG(nblocks >= 1 && nblocks <= V && (long)nblocks * SQ_BLOCK >= V,
                "drn_shortlist_segments_topn_q8: %d blocks outside [ceil(V / %d), V] for V = %d videos", nblocks, SQ_BLOCK, V);
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_MAX, "drn_shortlist_segments_topn_q8: n = %d outside [1, %d]", n, DRN_SHORTLIST_MAX);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "drn_shortlist_segments_topn_q8: dtype %d (float32 / bfloat16 queries only)", dtype);
  DRN_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)ws & 7) == 0,
                "drn_shortlist_segments_topn_q8: the codes and the queries must be 16-byte aligned, the workspace 8-byte aligned");
  const int m = n < SQ_BLOCK ? n : SQ_BLOCK, tiles = cdiv(S, 16);
  const long lists = (long)S * nblocks * m, need = lists + (lists + 1) / 2;
  DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need,
                "drn_shortlist_segments_topn_q8: the workspace holds %d keys, %ld are needed (1.5 * S * blocks * min(n, %d))", ws_keys, need,
                SQ_BLOCK);
  DRN_CHECK_ARG(tiles <= 65535, "drn_shortlist_segments_topn_q8: S = %d, more than 65535 tiles of 16 sentences", S);
  sl_key_t* lists_k = (sl_key_t*)ws;
  int* lists_r = (int*)(lists_k + lists);
  const dim3 grid(nblocks, tiles);
  if (dtype == DRN_BF16)
    shortlist_segments_q8_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>(codes, scales, (const bf16_t*)queries, offsets, blk_vid, R, V,
                                                                                E, S, m, nblocks, lists_k, lists_r);
  else
    shortlist_segments_q8_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(codes, scales, (const float*)queries, offsets, blk_vid, R, V,
                                                                               E, S, m, nblocks, lists_k, lists_r);
  sl_launch_merge(lists_k, S, n, m, nblocks, ids, scores, counts, (hipStream_t)stream);
  sl_launch_segment_rows(lists_k, lists_r, vid_blk, ids, V, S, n, m, nblocks, rows, (hipStream_t)stream);
  return drn_launch_status("drn_shortlist_segments_topn_q8");
}
