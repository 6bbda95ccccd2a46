// ASYMMETRIC binary shortlists (drn_amd/binary.py, BinaryShortlister.shortlist_asym): FLOAT queries against a table of 1-bit SIGN CODES.
//   shortlist_bin_asym_block_kernel<T, VEC>      phase one on a table of one row per video: the MFMA chain of the plain shortlist with
//                                                its table operand built from the code bits in registers, then the sort of retrieve.hip;
//   shortlist_bin_asym_segments_kernel<T, VEC>   phase one on a ragged table: the block plan, the passes and the segmented maximum of
//                                                retrieve_seg.hip over the fp32 scores of the same chain;
//   drn_shortlist_bin_asym                       the one entry: either phase one, then sl_launch_merge_deep and sl_launch_segment_rows
//                                                (shortlist.h) as they stand.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// THE FORMAT is retrieve_bin.hip's: a row is W = ceil(E / 32) int32 words, bit e & 31 of word e >> 5 is 1 unless x[e] < 0, the bits at
// or past E are 0.  The codes stand for the (rows, E) table of +-1 (bit set: +1), and score[s][r] = sum_e q[s][e] * (+-1): the PLAIN
// shortlist over that table.  So there is no definition of its own and no arithmetic of its own: the tiling is
// shortlist_block_allow_kernel's (retrieve_allow.hip: a workgroup takes 256 videos x 16 sentences, a wave 64 videos as four 16x16
// accumulators, lane (r = lane & 15, g = lane >> 4) holds query row s0 + r as operand A), the chain is AlPlain<T>::scores' (shortlist.h:
// K-steps in ascending order, sl_mfma, 32 columns a step in bf16 and 16 in fp32, lane g owning columns c + g * PER_LANE ...), and
// operand B is what sl_frag / sl_frag_tail would load from the dequantised row, value for value at the same operand position:
//   bf16   byte g of code word c / 32 of the row -> eight bf16 of +-1 (0x3f80 / 0xbf80);
//   fp32   the nibble at bit (c & 31) + 4 g of that word -> four floats of +-1;
//   tail   a column at or past E is ZERO on both sides, as sl_frag_tail makes it (a pad bit is 0 and would read as -1).
// Equal operands through the same instructions in the same order give equal bits: every field is that of drn_shortlist_deep over the
// dequantised table.  A query row that holds an element that is not finite scores nothing finite, and sl_key drops it there as here.
//
// VEC: W % 4 == 0 and a row's words are read four at a time in 16-byte loads (the table is 16-byte aligned, so every row is); else word
// by word.  A word's loads for the four rows of a lane are issued before its steps run.
//
// A disallowed video, a sentence past S, a video past V and a score that is not finite become key 0 -- "no candidate" -- so the sort,
// the merges and the segment look-up serve as they stand.  No dark-block skip: every block scores its rows whatever the mask says.
#define BA_BLOCK 256        // = SL_BLOCK = SG_BLOCK = AL_BLOCK = BN_BLOCK = _lib.SHORTLIST_BLOCK = _lib.SHORTLIST_SEG_BLOCK
#define BA_LD (BA_BLOCK + 1)
#define BA_WORDS 8          // mask words of a ranked block: BA_BLOCK / 32
#define BA_SEG_WORDS 9      // of a ragged block, which starts at any video

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The fragment sl_frag(row, c0) loads from the dequantised row, c0 = c + g * PER_LANE, from the row's code word `w` = word c / 32.
// bf16: the lane's eight columns are byte g of the word; two columns a 32-bit half: 0x3f80 with the sign bit set where the code bit
// is clear.
__device__ __forceinline__ bf16x8 ba_frag(const unsigned w, const int c, const int g, bf16_t) {
  const unsigned clear = ~(w >> (8 * g));                    // bit j: column c0 + j is -1
  u32x4 f;
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = 0x3f803f80u | (((clear >> (2 * k)) & 1u) << 15) | (((clear >> (2 * k + 1)) & 1u) << 31);
  return __builtin_bit_cast(bf16x8, f);
}
// fp32: the lane's four columns are the nibble at bit (c & 31) + 4 g (c is a multiple of 16: the word's low or high half)
__device__ __forceinline__ f32x4 ba_frag(const unsigned w, const int c, const int g, float) {
  const unsigned clear = ~(w >> ((c & 31) + 4 * g));
  u32x4 f;
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = 0x3f800000u | (((clear >> k) & 1u) << 31);
  return __builtin_bit_cast(f32x4, f);
}
// ... and sl_frag_tail(row, c0, E): zeros at or past E
__device__ __forceinline__ bf16x8 ba_frag_tail(const unsigned w, const int c, const int g, const int E, bf16_t) {
  u32x4 f = __builtin_bit_cast(u32x4, ba_frag(w, c, g, bf16_t()));
  const int c0 = c + 8 * g;
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] &= (c0 + 2 * k < E ? 0x0000ffffu : 0u) | (c0 + 2 * k + 1 < E ? 0xffff0000u : 0u);
  return __builtin_bit_cast(bf16x8, f);
}
__device__ __forceinline__ f32x4 ba_frag_tail(const unsigned w, const int c, const int g, const int E, float) {
  u32x4 f = __builtin_bit_cast(u32x4, ba_frag(w, c, g, float()));
  const int c0 = c + 4 * g;
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = c0 + k < E ? f[k] : 0u;
  return __builtin_bit_cast(f32x4, f);
}

// the K-steps of one code word (columns 32 word .. 32 word + 31: one step in bf16, two in fp32) for the lane's four rows, whose
// words are w[0..3].  `whole` is AlPlain's: below it a step is sl_frag on both sides, from it on sl_frag_tail (wave-uniform)
template <typename T>
__device__ __forceinline__ void ba_word(const T* qrow, const unsigned (&w)[4], const int word, const int E, const int whole, const int g,
                                        f32x4 (&acc)[4]) {
  constexpr int COLS = SlStep<T>::COLS, PER_LANE = SlStep<T>::PER_LANE;
#pragma unroll
  for (int k = 0; k < 32 / COLS; ++k) {
    const int c = 32 * word + k * COLS, c0 = c + g * PER_LANE;
    if (c < whole) {
      const auto a = sl_frag(qrow, c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = sl_mfma(a, ba_frag(w[j], c, g, T()), acc[j]);
    } else if (c < E) {
      const auto a = sl_frag_tail(qrow, c0, E);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = sl_mfma(a, ba_frag_tail(w[j], c, g, E, T()), acc[j]);
    }
  }
}

// acc[j] += q[16 sentences] x the +-1 rows that the codes of row[j] stand for (j = 0..3): AlPlain<T>::scores over the dequantised table
template <typename T, bool VEC>
__device__ __forceinline__ void ba_scores(const int* __restrict__ codes, const T* qrow, const long (&row)[4], const int E, const int W,
                                          const int g, f32x4 (&acc)[4]) {
  constexpr int COLS = SlStep<T>::COLS, PER_LANE = SlStep<T>::PER_LANE;
  const int whole = E % PER_LANE == 0 ? E / COLS * COLS : 0;
  const int* crow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) crow[j] = codes + row[j] * W;
  if constexpr (VEC) {
    for (int w0 = 0; w0 < W; w0 += 4) {
      i32x4 x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const i32x4*>(crow[j] + w0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned w[4] = {(unsigned)x[0][u], (unsigned)x[1][u], (unsigned)x[2][u], (unsigned)x[3][u]};
        ba_word<T>(qrow, w, w0 + u, E, whole, g, acc);
      }
    }
  } else {
    for (int w0 = 0; w0 < W; ++w0) {
      const unsigned w[4] = {(unsigned)crow[0][w0], (unsigned)crow[1][w0], (unsigned)crow[2][w0], (unsigned)crow[3][w0]};
      ba_word<T>(qrow, w, w0, E, whole, g, acc);
    }
  }
}

// The tile's mask words from word w0 on into mw[sentence of the tile][word - w0], NW words a row; a word at or past Wm = ceil(V / 32)
// is not read (zero).  A sentence slot past S reads the last sentence's row.  The caller's next barrier publishes them.
template <int NW>
__device__ __forceinline__ void ba_load_mask(const int* __restrict__ allow, const int stride, const int s0, const int S, const int w0,
                                             const int Wm, int* mw, const int tid) {
  if (tid < 16 * NW) {
    const int sl = tid / NW, w = w0 + tid - sl * NW;
    mw[tid] = w < Wm ? allow[(long)min(s0 + sl, S - 1) * stride + w] : 0;
  }
}

// Static LDS: keys 32,768 + mw 512 = 33,280 B.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void shortlist_bin_asym_block_kernel(const int* __restrict__ codes, const T* __restrict__ q,
                                                                       const int* __restrict__ allow, const int allow_stride, const int V,
                                                                       const int E, const int S, const int m, const int nblocks,
                                                                       sl_key_t* __restrict__ ws) {
  __shared__ sl_key_t keys[16 * BA_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block]
  __shared__ int mw[16 * BA_WORDS];                           // [sentence of the tile][mask word of the block]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, v0 = b * BA_BLOCK + wave * 64, W = (E + 31) >> 5;
  const int r = lane & 15, g = lane >> 4;
  ba_load_mask<BA_WORDS>(allow, allow_stride, s0, S, b * BA_WORDS, (V + 31) >> 5, mw, tid);
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    // (a row past S or V reads the last row instead: its scores become no keys below)
    const T* qrow = q + (long)min(s0 + r, S - 1) * E;
    long row[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) row[j] = min(v0 + 16 * j + r, V - 1);
    ba_scores<T, VEC>(codes, qrow, row, E, W, g, acc);
  }
  __syncthreads();                                            // (publishes mw)
  // C/D: column (video) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = v0 + 16 * j + r, sl = 4 * g + i, at = wave * 64 + 16 * j + r;
      const bool ok = v < V && s0 + sl < S && ((mw[sl * BA_WORDS + (at >> 5)] >> (at & 31)) & 1);
      keys[sl * BA_BLOCK + at] = ok ? sl_key(acc[j][i], v) : 0ull;
    }
  __syncthreads();
  sl_sort_desc<BA_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    ws[((long)(s0 + sl) * nblocks + b) * m + i] = keys[sl * BA_BLOCK + i];
  }
}

// shortlist_segments_kernel (retrieve_seg.hip: the block plan, the passes, the segmented maximum, the states and the keys are described
// there) over the fp32 scores of ba_scores: a pass scores 256 table rows, 64 a wave, into sc; then item (sentence, video, part) folds
// its share of the video's rows of the pass, the parts meet by shuffles and part 0 -- the ONE writer of its (sentence, video) -- keeps
// the maximum.  A state is (ordered score word, ~segment): the lowest segment wins a tie; 0 is a video without rows, 0xffffffff a NaN.
// As there, every index read from the device tables is clamped.
// Static LDS: keys 32,768 + sc 16,448 + voff 1,040 + mw 576 + wlong 16 = 50,848 B.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void shortlist_bin_asym_segments_kernel(const int* __restrict__ codes, const T* __restrict__ q,
                                                                          const int* __restrict__ offsets, const int* __restrict__ blk_vid,
                                                                          const int* __restrict__ allow, const int allow_stride,
                                                                          const int R, const int V, const int E, const int S, const int m,
                                                                          const int nblocks, sl_key_t* __restrict__ ws,
                                                                          int* __restrict__ wsr) {
  __shared__ sl_key_t keys[16 * BA_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block], states then keys
  __shared__ float sc[16 * BA_LD];                            // [sentence of the tile][row of the pass]; after the last pass, as
  int* const seg = reinterpret_cast<int*>(sc);                // integers, the winning segment of [sentence][video]
  __shared__ int voff[BA_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ int wlong[4];                                    // each wave's longest run
  __shared__ int mw[16 * BA_SEG_WORDS];                       // [sentence of the tile][mask word from the block's first]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, W = (E + 31) >> 5;
  const int r = lane & 15, g = lane >> 4;
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + BA_BLOCK, V)), nv = v1 - v0;
  const int lenlg = nv <= 16 ? 4 : nv <= 64 ? 6 : 8, len = 1 << lenlg;          // keys per sentence: 16, 64 or 256 >= nv
  for (int i = tid; i <= nv; i += 256) voff[i] = min(max(offsets[min(v0 + i, V)], 0), R);
  for (int p = tid; p < 16 * len; p += 256) keys[p] = 0ull;
  ba_load_mask<BA_SEG_WORDS>(allow, allow_stride, s0, S, v0 >> 5, (V + 31) >> 5, mw, tid);
  __syncthreads();
  {
    int mine = tid < nv ? voff[tid + 1] - voff[tid] : 0;      // (nv <= 256: one video per thread)
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) mine = max(mine, __shfl_xor(mine, w, 64));
    if (lane == 0) wlong[wave] = mine;
  }
  __syncthreads();
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), BA_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (sentence, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  // (a sentence past S reads the last one instead: its states become no keys below)
  const T* qrow = q + (long)min(s0 + r, S - 1) * E;
  for (int p0 = r0; p0 < r1; p0 += BA_BLOCK) {
    const int p1 = min(p0 + BA_BLOCK, r1), rw = p0 + wave * 64;
    if (rw < p1) {                                            // (wave-uniform: a wave whose 64 rows lie past the block reads nothing)
      // (a row past the block reads the table's last row instead: nobody folds its score; p1 <= r1 <= R and R >= 1)
      long row[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = min(rw + 16 * j + r, R - 1);
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      ba_scores<T, VEC>(codes, qrow, row, E, W, g, acc);
      // C/D: column (row of the table) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[(4 * g + i) * BA_LD + wave * 64 + 16 * j + r] = acc[j][i];
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
      const float* mine = sc + sl * BA_LD;
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
  // states -> keys.  An ordered word is a finite score's between those of -inf and +inf; 0 is a video without rows.  The mask enters
  // here: a video whose bit is clear becomes no key.
  for (int p = tid; p < 16 * len; p += 256) {
    const int sl = p >> lenlg, vi = p & (len - 1);
    const sl_key_t st = keys[p];
    const unsigned o = (unsigned)(st >> 32);
    const int v = v0 + min(vi, BA_BLOCK - 1);                 // (v - 32 (v0 >> 5) < 32 BA_SEG_WORDS: inside mw)
    const bool may = (mw[sl * BA_SEG_WORDS + (v >> 5) - (v0 >> 5)] >> (v & 31)) & 1;
    const bool ok = vi < nv && s0 + sl < S && o > 0x007fffffu && o < 0xff800000u && may;
    seg[p] = (int)~(unsigned)st;
    keys[p] = ok ? ((sl_key_t)o << 32) | (sl_key_t)(~(unsigned)(v0 + vi)) : 0ull;
  }
  __syncthreads();
  if (lenlg == 4) sl_sort_desc<16, 256>(keys, 16, tid);       // (block-uniform)
  else if (lenlg == 6) sl_sort_desc<64, 256>(keys, 16, tid);
  else sl_sort_desc<BA_BLOCK, 256>(keys, 16, tid);
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
static void ba_launch(const int32_t* codes, const void* queries, const int32_t* offsets, const int32_t* blk_vid, const int32_t* vid_blk,
                      const int32_t* allow, const int allow_stride, const int R, const int V, const int nblocks, const int E, const int S,
                      const int n, sl_key_t* lists_k, int32_t* ids, float* scores, int32_t* counts, int32_t* rows, hipStream_t stream) {
  const int m = n < BA_BLOCK ? n : BA_BLOCK;
  const dim3 grid(nblocks, cdiv(S, 16));
  // (the deep merge at every n, as drn_shortlist_bin and for the reason recorded there)
  if (!offsets) {
    shortlist_bin_asym_block_kernel<T, VEC><<<grid, 256, 0, stream>>>(codes, (const T*)queries, allow, allow_stride, V, E, S, m, nblocks,
                                                                      lists_k);
    sl_launch_merge_deep(lists_k, S, n, m, nblocks, ids, scores, counts, stream);
  } else {
    int* lists_r = (int*)(lists_k + (long)S * nblocks * m);
    shortlist_bin_asym_segments_kernel<T, VEC><<<grid, 256, 0, stream>>>(codes, (const T*)queries, offsets, blk_vid, allow, allow_stride, R, V,
                                                                         E, S, m, nblocks, lists_k, lists_r);
    sl_launch_merge_deep(lists_k, S, n, m, nblocks, ids, scores, counts, stream);
    sl_launch_segment_rows(lists_k, lists_r, vid_blk, ids, V, S, n, m, nblocks, rows, stream);
  }
}

extern "C" int drn_shortlist_bin_asym(const int32_t* codes, const void* queries, const int32_t* offsets, const int32_t* blk_vid,
                                      const int32_t* vid_blk, const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E,
                                      int S, int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts,
                                      int32_t* rows, void* stream) {
  const char* what = "drn_shortlist_bin_asym";
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
  DRN_CHECK_ARG(E <= DRN_BINARY_MAX_E, "%s: E = %d columns above %d (the limit of a table of sign codes)", what, E, DRN_BINARY_MAX_E);
  if (ragged)
    DRN_CHECK_ARG(nblocks >= 1 && nblocks <= V && (long)nblocks * BA_BLOCK >= V, "%s: %d blocks outside [ceil(V / %d), V] for V = %d videos",
                  what, nblocks, BA_BLOCK, V);
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_DEEP_MAX, "%s: n = %d outside [1, %d]", what, n, DRN_SHORTLIST_DEEP_MAX);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "%s: dtype %d (float32 / bfloat16 only)", what, dtype);
  DRN_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)ws & 7) == 0,
                "%s: the table and the queries must be 16-byte aligned, the workspace 8-byte aligned", what);
  DRN_CHECK_ARG(allow_stride == 0 || allow_stride == cdiv(V, 32),
                "%s: allow_stride = %d is neither 0 (one mask for all sentences) nor ceil(V / 32) = %d (one row per sentence)", what,
                allow_stride, cdiv(V, 32));
  DRN_CHECK_ARG(((uintptr_t)allow & 3) == 0, "%s: the mask must be 4-byte aligned", what);
  const int m = n < BA_BLOCK ? n : BA_BLOCK, blocks = ragged ? nblocks : cdiv(V, BA_BLOCK), tiles = cdiv(S, 16);
  const long lists = (long)S * blocks * m, need = ragged ? lists + (lists + 1) / 2 : lists;
  if (ragged)
    DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (1.5 * S * blocks * min(n, %d))", what,
                  ws_keys, need, BA_BLOCK);
  else
    DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (S * ceil(V / %d) * min(n, %d))", what,
                  ws_keys, need, BA_BLOCK, BA_BLOCK);
  DRN_CHECK_ARG(tiles <= 65535, "%s: S = %d, more than 65535 tiles of 16 sentences", what, S);
  const bool vec = cdiv(E, 32) % 4 == 0, bf16 = dtype == DRN_BF16;
  const auto launch = bf16 ? (vec ? ba_launch<bf16_t, true> : ba_launch<bf16_t, false>) : (vec ? ba_launch<float, true> : ba_launch<float, false>);
  launch(codes, queries, offsets, blk_vid, vid_blk, allow, allow_stride, ragged ? R : 0, V, blocks, E, S, n, (sl_key_t*)ws, ids, scores, counts,
         rows, (hipStream_t)stream);
  return drn_launch_status(what);
}
