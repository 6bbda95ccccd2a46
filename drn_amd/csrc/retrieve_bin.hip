// Binary shortlists (drn_amd/binary.py, BinaryShortlister.shortlist): a table of 1-BIT SIGN CODES ranked by Hamming distance.
//   shortlist_bin_block_kernel<T, VEC>      phase one on a table of one row per video: XOR and popcount, then the sort of retrieve.hip;
//   shortlist_bin_segments_kernel<T, VEC>   phase one on a ragged table: the block plan, the passes and the segmented maximum of
//                                           retrieve_seg.hip over integer scores;
//   drn_shortlist_bin                       the one entry: either phase one, then sl_launch_merge_deep and sl_launch_segment_rows
//                                           (shortlist.h) as they stand.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// THE FORMAT.  A row is W = ceil(E / 32) int32 words: bit e & 31 of word e >> 5 is 1 unless x[e] < 0 (so +0 and -0 give 1), the bits at
// or past E are 0 -- the bit convention of a packed allow mask, and drn_pack_allow over ~(x < 0) is the quantiser.  A query row is
// binarised by the same rule HERE, once per workgroup, into LDS; a row that holds an element that is not finite is flagged there and
// lists nothing.  score[s][r] = E - 2 popcount(code(q_s) xor codes[r]) = sum_e sign(q_e) sign(x_e): an integer in [-E, E], exact as a
// float (E <= DRN_BINARY_MAX_E), which becomes an sl_key as every other score does.  The pad bits are 0 on both sides and cancel.
//
// One table row per thread, 16 integer accumulators (the tile's sentences); a query word is read from LDS by all lanes at one address
// (a broadcast).  VEC: W % 4 == 0 and a row is read in 16-byte loads (the table is 16-byte aligned, so every row is); else word by word.
//
// A disallowed video, a sentence past S, a video past V and a flagged sentence become key 0 -- "no candidate" -- so the sort, the
// merges and the segment look-up serve as they stand.  No dark-block skip: every block scores its rows whatever the mask says.
#define BN_BLOCK 256        // = SL_BLOCK = SG_BLOCK = AL_BLOCK = _lib.SHORTLIST_BLOCK = _lib.SHORTLIST_SEG_BLOCK
#define BN_LD (BN_BLOCK + 1)
#define BN_MAX_W (DRN_BINARY_MAX_E / 32)   // 128 words: 16 sentences' query codes are 8 KiB of LDS
#define BN_WORDS 8          // mask words of a ranked block: BN_BLOCK / 32
#define BN_SEG_WORDS 9      // of a ragged block, which starts at any video
#define BN_LOADS 8          // query elements a lane has in flight while it binarises (a choice, not a measurement)

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The tile's 16 query rows -> qc[sentence of the tile][word], W words a row, and bad[sentence] = a element of the row is not finite.
// One wavefront per 64 columns of a row: a lane reads one element and the ballot is two words (pack_allow_kernel's shape).  A
// sentence slot past S reads the last sentence's row: its keys become 0 below.  Ends in a barrier.
template <typename T>
__device__ __forceinline__ void bn_binarise(const T* __restrict__ q, const int s0, const int S, const int E, const int W, unsigned* qc,
                                            int* bad, const int tid) {
  const int lane = tid & 63, wave = tid >> 6, W64 = (E + 63) >> 6;
  if (tid < 16) bad[tid] = 0;
  __syncthreads();
  const int total = 16 * W64;
  for (int i0 = wave; i0 < total; i0 += 4 * BN_LOADS) {       // (wave-uniform, as every condition on i below)
    float x[BN_LOADS];                                        // BN_LOADS independent loads are issued before the first ballot waits
#pragma unroll
    for (int u = 0; u < BN_LOADS; ++u) {
      const int i = i0 + 4 * u, sl = i / W64, e = 64 * (i - sl * W64) + lane;
      x[u] = i < total && e < E ? (float)q[(long)min(s0 + sl, S - 1) * E + e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < BN_LOADS; ++u) {
      const int i = i0 + 4 * u, sl = i / W64, k = i - sl * W64, e = 64 * k + lane;
      if (i >= total) break;
      const unsigned long long set = __ballot(e < E && !(x[u] < 0.f));
      const bool wild = __ballot(!isfinite(x[u])) != 0ull;
      if (lane == 0) qc[sl * W + 2 * k] = (unsigned)set;
      if (lane == 1 && 2 * k + 1 < W) qc[sl * W + 2 * k + 1] = (unsigned)(set >> 32);
      if (lane == 2 && wild) bad[sl] = 1;                     // (every writer of a flag writes the same word)
    }
  }
  __syncthreads();
}

// h[sl] = popcount(qc[sl] xor row), sl = 0..15, over the row's W words
template <bool VEC>
__device__ __forceinline__ void bn_hamming(const int* __restrict__ row, const unsigned* qc, const int W, int (&h)[16]) {
#pragma unroll
  for (int sl = 0; sl < 16; ++sl) h[sl] = 0;
  if constexpr (VEC) {
    for (int w = 0; w < W; w += 4) {
      const i32x4 x = *reinterpret_cast<const i32x4*>(row + w);
#pragma unroll
      for (int sl = 0; sl < 16; ++sl) {
        const i32x4 c = *reinterpret_cast<const i32x4*>(qc + sl * W + w);
        h[sl] += __popc((unsigned)(x[0] ^ c[0])) + __popc((unsigned)(x[1] ^ c[1])) + __popc((unsigned)(x[2] ^ c[2])) +
                 __popc((unsigned)(x[3] ^ c[3]));
      }
    }
  } else {
    for (int w = 0; w < W; ++w) {
      const unsigned x = (unsigned)row[w];
#pragma unroll
      for (int sl = 0; sl < 16; ++sl) h[sl] += __popc(x ^ qc[sl * W + w]);
    }
  }
}

// The tile's mask words from word w0 on into mw[sentence of the tile][word - w0], NW words a row; a word at or past Wm = ceil(V / 32)
// is not read (zero).  A sentence slot past S reads the last sentence's row.  The caller's next barrier publishes them.
template <int NW>
__device__ __forceinline__ void bn_load_mask(const int* __restrict__ allow, const int stride, const int s0, const int S, const int w0,
                                             const int Wm, int* mw, const int tid) {
  if (tid < 16 * NW) {
    const int sl = tid / NW, w = w0 + tid - sl * NW;
    mw[tid] = w < Wm ? allow[(long)min(s0 + sl, S - 1) * stride + w] : 0;
  }
}

// Static LDS: keys 32,768 + qc 8,192 + mw 512 + bad 64 = 41,536 B.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void shortlist_bin_block_kernel(const int* __restrict__ codes, const T* __restrict__ q,
                                                                  const int* __restrict__ allow, const int allow_stride, const int V,
                                                                  const int E, const int S, const int m, const int nblocks,
                                                                  sl_key_t* __restrict__ ws) {
  __shared__ sl_key_t keys[16 * BN_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block]
  __shared__ __attribute__((aligned(16))) unsigned qc[16 * BN_MAX_W];   // [sentence of the tile][word]: W words a row are used
  __shared__ int mw[16 * BN_WORDS];                           // [sentence of the tile][mask word of the block]
  __shared__ int bad[16];                                     // the sentence's query row is not finite
  const int tid = threadIdx.x, b = blockIdx.x, s0 = blockIdx.y * 16, W = (E + 31) >> 5;
  bn_load_mask<BN_WORDS>(allow, allow_stride, s0, S, b * BN_WORDS, (V + 31) >> 5, mw, tid);
  bn_binarise<T>(q, s0, S, E, W, qc, bad, tid);
  const int v = b * BN_BLOCK + tid;
  int h[16];
  // (a video past V reads the last row instead: its scores become no keys below)
  bn_hamming<VEC>(codes + (long)min(v, V - 1) * W, qc, W, h);
#pragma unroll
  for (int sl = 0; sl < 16; ++sl) {
    const bool ok = v < V && s0 + sl < S && !bad[sl] && ((mw[sl * BN_WORDS + (tid >> 5)] >> (tid & 31)) & 1);
    keys[sl * BN_BLOCK + tid] = ok ? sl_key((float)(E - 2 * h[sl]), v) : 0ull;
  }
  __syncthreads();
  sl_sort_desc<BN_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    ws[((long)(s0 + sl) * nblocks + b) * m + i] = keys[sl * BN_BLOCK + i];
  }
}

// shortlist_segments_kernel (retrieve_seg.hip: the block plan, the passes, the segmented maximum, the states and the keys are described
// there) over integer scores: a pass scores 256 table rows, one per thread, into sc; then item (sentence, video, part) folds its share
// of the video's rows of the pass, the parts meet by shuffles and part 0 -- the ONE writer of its (sentence, video) -- keeps the
// maximum.  A state is (ordered score word, ~segment): the lowest segment wins a tie; 0 is a video without rows.  As there, every
// index read from the device tables is clamped.
// Static LDS: keys 32,768 + sc 16,448 + qc 8,192 + voff 1,040 + mw 576 + bad 64 + wlong 16 = 59,104 B.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void shortlist_bin_segments_kernel(const int* __restrict__ codes, const T* __restrict__ q,
                                                                     const int* __restrict__ offsets, const int* __restrict__ blk_vid,
                                                                     const int* __restrict__ allow, const int allow_stride, const int R,
                                                                     const int V, const int E, const int S, const int m,
                                                                     const int nblocks, sl_key_t* __restrict__ ws, int* __restrict__ wsr) {
  __shared__ sl_key_t keys[16 * BN_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block], states then keys
  __shared__ int sc[16 * BN_LD];                              // [sentence of the tile][row of the pass]; after the last pass the
  int* const seg = sc;                                        // winning segment of [sentence][video]
  __shared__ __attribute__((aligned(16))) unsigned qc[16 * BN_MAX_W];
  __shared__ int voff[BN_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ int wlong[4];                                    // each wave's longest run
  __shared__ int mw[16 * BN_SEG_WORDS];                       // [sentence of the tile][mask word from the block's first]
  __shared__ int bad[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, W = (E + 31) >> 5;
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + BN_BLOCK, V)), nv = v1 - v0;
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // keys per sentence: 16, 64 or 256 >= nv
  for (int i = tid; i <= nv; i += 256) voff[i] = min(max(offsets[min(v0 + i, V)], 0), R);
  for (int p = tid; p < 16 * len; p += 256) keys[p] = 0ull;
  bn_load_mask<BN_SEG_WORDS>(allow, allow_stride, s0, S, v0 >> 5, (V + 31) >> 5, mw, tid);
  bn_binarise<T>(q, s0, S, E, W, qc, bad, tid);               // (its barriers publish voff, keys and mw too)
  {
    int mine = tid < nv ? voff[tid + 1] - voff[tid] : 0;      // (nv <= 256: one video per thread)
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) mine = max(mine, __shfl_xor(mine, w, 64));
    if (lane == 0) wlong[wave] = mine;
  }
  __syncthreads();
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), BN_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (sentence, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  for (int p0 = r0; p0 < r1; p0 += BN_BLOCK) {
    const int p1 = min(p0 + BN_BLOCK, r1), row = p0 + tid;
    if (row < p1) {                                           // (p1 <= r1 <= R: the row is the table's; a row past the pass is nobody's)
      int h[16];
      bn_hamming<VEC>(codes + (long)row * W, qc, W, h);
#pragma unroll
      for (int sl = 0; sl < 16; ++sl) sc[sl * BN_LD + tid] = E - 2 * h[sl];
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
      const int* mine = sc + sl * BN_LD;
      sl_key_t best = 0ull;
      for (int x = from; x < to; ++x) {
        const sl_key_t cand = ((sl_key_t)sl_word((float)mine[x - p0]) << 32) | (sl_key_t)(~(unsigned)(x - base));
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
  // states -> keys: the mask and the flag enter here
  for (int p = tid; p < 16 * len; p += 256) {
    const int sl = p >> lenlg, vi = p & (len - 1);
    const sl_key_t st = keys[p];
    const int v = v0 + min(vi, BN_BLOCK - 1);                 // (v - 32 (v0 >> 5) < 32 BN_SEG_WORDS: inside mw)
    const bool may = (mw[sl * BN_SEG_WORDS + (v >> 5) - (v0 >> 5)] >> (v & 31)) & 1;
    const bool ok = vi < nv && s0 + sl < S && st != 0ull && may && !bad[sl];
    seg[p] = (int)~(unsigned)st;
    keys[p] = ok ? (st & 0xffffffff00000000ull) | (sl_key_t)(~(unsigned)(v0 + vi)) : 0ull;
  }
  __syncthreads();
  if (lenlg == 4) sl_sort_desc<16, 256>(keys, 16, tid);       // (block-uniform)
  else if (lenlg == 6) sl_sort_desc<64, 256>(keys, 16, tid);
  else sl_sort_desc<BN_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    const sl_key_t k = i < len ? keys[sl * len + i] : 0ull;
    const long at = ((long)(s0 + sl) * nblocks + b) * m + i;
    ws[at] = k;
    wsr[at] = k != 0ull ? seg[sl * len + (sl_video(k) - v0)] : -1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC>
static void bn_launch(const int32_t* codes, const void* queries, const int32_t* offsets, const int32_t* blk_vid, const int32_t* vid_blk,
                      const int32_t* allow, const int allow_stride, const int R, const int V, const int nblocks, const int E, const int S,
                      const int n, sl_key_t* lists_k, int32_t* ids, float* scores, int32_t* counts, int32_t* rows, hipStream_t stream) {
  const int m = n < BN_BLOCK ? n : BN_BLOCK;
  const dim3 grid(nblocks, cdiv(S, 16));
  // (the deep merge at every n, as drn_shortlist_deep: the best n of a set of distinct keys do not depend on how they are found, and
  // with sl_launch_merge below DRN_SHORTLIST_MAX the call measured 1.05x to 1.43x of drn_shortlist_deep's at n = 16 and 128)
  const auto merge = sl_launch_merge_deep;
  if (!offsets) {
    shortlist_bin_block_kernel<T, VEC><<<grid, 256, 0, stream>>>(codes, (const T*)queries, allow, allow_stride, V, E, S, m, nblocks, lists_k);
    merge(lists_k, S, n, m, nblocks, ids, scores, counts, stream);
  } else {
    int* lists_r = (int*)(lists_k + (long)S * nblocks * m);
    shortlist_bin_segments_kernel<T, VEC><<<grid, 256, 0, stream>>>(codes, (const T*)queries, offsets, blk_vid, allow, allow_stride, R, V, E,
                                                                    S, m, nblocks, lists_k, lists_r);
    merge(lists_k, S, n, m, nblocks, ids, scores, counts, stream);
    sl_launch_segment_rows(lists_k, lists_r, vid_blk, ids, V, S, n, m, nblocks, rows, stream);
  }
}

extern "C" int drn_shortlist_bin(const int32_t* codes, const void* queries, const int32_t* offsets, const int32_t* blk_vid,
                                 const int32_t* vid_blk, const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S,
                                 int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, int32_t* rows,
                                 void* stream) {
  const char* what = "drn_shortlist_bin";
  drn_clear_status();
  const bool ragged = offsets != nullptr;
  DRN_CHECK_ARG(ragged || !(blk_vid || vid_blk || rows),
                "%s: null pointer: offsets is NULL (one row per video), so blk_vid, vid_blk and rows must be NULL too", what);
  DRN_CHECK_ARG(codes && queries && allow && ws && ids && scores && counts && (!ragged || (blk_vid && vid_blk && rows)), "%s: null pointer",
                what);
  if (ragged)
    DRN_CHECK_ARG(R >= 1 && V >= 1 && E >= 1 && S >= 1, "%s: bad args (R = %d rows, V = %d videos, E = %d columns, S = %d sentences)", what, R,
                  V, E, S);
  else
    DRN_CHECK_ARG(V >= 1 && E >= 1 && S >= 1, "%s: bad args (V = %d videos, E = %d columns, S = %d sentences)", what, V, E, S);
  DRN_CHECK_ARG(E <= DRN_BINARY_MAX_E, "%s: E = %d columns above %d (16 sentences' query codes are kept in 8 KiB of LDS)", what, E,
                DRN_BINARY_MAX_E);
  if (ragged)
    DRN_CHECK_ARG(nblocks >= 1 && nblocks <= V && (long)nblocks * BN_BLOCK >= V, "%s: %d blocks outside [ceil(V / %d), V] for V = %d videos",
                  what, nblocks, BN_BLOCK, V);
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_DEEP_MAX, "%s: n = %d outside [1, %d]", what, n, DRN_SHORTLIST_DEEP_MAX);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "%s: dtype %d (float32 / bfloat16 only)", what, dtype);
  DRN_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)ws & 7) == 0,
                "%s: the table and the queries must be 16-byte aligned, the workspace 8-byte aligned", what);
  DRN_CHECK_ARG(allow_stride == 0 || allow_stride == cdiv(V, 32),
                "%s: allow_stride = %d is neither 0 (one mask for all sentences) nor ceil(V / 32) = %d (one row per sentence)", what,
                allow_stride, cdiv(V, 32));
  DRN_CHECK_ARG(((uintptr_t)allow & 3) == 0, "%s: the mask must be 4-byte aligned", what);
  const int m = n < BN_BLOCK ? n : BN_BLOCK, blocks = ragged ? nblocks : cdiv(V, BN_BLOCK), tiles = cdiv(S, 16);
  const long lists = (long)S * blocks * m, need = ragged ? lists + (lists + 1) / 2 : lists;
  if (ragged)
    DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (1.5 * S * blocks * min(n, %d))", what,
                  ws_keys, need, BN_BLOCK);
  else
    DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (S * ceil(V / %d) * min(n, %d))", what,
                  ws_keys, need, BN_BLOCK, BN_BLOCK);
  DRN_CHECK_ARG(tiles <= 65535, "%s: S = %d, more than 65535 tiles of 16 sentences", what, S);
  const bool vec = cdiv(E, 32) % 4 == 0, bf16 = dtype == DRN_BF16;
  const auto launch = bf16 ? (vec ? bn_launch<bf16_t, true> : bn_launch<bf16_t, false>) : (vec ? bn_launch<float, true> : bn_launch<float, false>);
  launch(codes, queries, offsets, blk_vid, vid_blk, allow, allow_stride, ragged ? R : 0, V, blocks, E, S, n, (sl_key_t*)ws, ids, scores, counts,
         rows, (hipStream_t)stream);
  return drn_launch_status(what);
}
