// Filtered shortlists (drn_amd/retrieve.py, Shortlister.shortlist(allow=)): the four shortlist entries with a packed ALLOW MASK, and its maker.
//   drn_shortlist_topn_allow / drn_shortlist_segments_topn_allow             the plain and the ragged table (retrieve.hip, retrieve_seg.hip);
//   drn_shortlist_topn_q8_allow / drn_shortlist_segments_topn_q8_allow       the same two kept in block-scaled FP8 (retrieve_q8.hip);
//   drn_pack_allow                                                           a bool mask (V,) or (S, V) -> the packed words, one launch;
//   drn_shortlist_deep                                                       the four tables at n up to 1024: host code over the same phase one.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// A packed mask is W = ceil(V / 32) int32 words a row: bit v & 31 of word v >> 5 set = video v may be listed; bits at or past V are
// ignored.  allow_stride = 0: one row for every sentence; = W: row s for sentence s.
//
// A disallowed video becomes key 0 -- "no candidate" -- in phase one, where states become keys: the keys of a sentence stay distinct, so
// the sort, shortlist_merge_kernel and shortlist_segment_rows_kernel serve as they stand (sl_launch_merge, sl_launch_segment_rows), and
// the list is the unmasked definition applied to the allowed videos.  The scores come from the chain of the unmasked kernels -- the
// same fragments, the same K-steps in ascending order, the same sl_mfma -- so a listed score has the bits those kernels give it.
//
// Phase one is TWO kernel bodies, the ranked block and the ranked segment block, templated on the TABLE OPERAND (shortlist.h): AlPlain<T> loads a
// row's fragments (sl_frag / sl_frag_tail), AlQ8<T, NB> builds them from codes and scale bytes (sq_scores: sl_codes_q8 / sl_frag_q8,
// NB scale blocks of loads in flight as in retrieve_q8.hip: two in the ranked block's bf16 chain, one elsewhere).
//
// THE DARK-BLOCK SKIP.  Before any table row is read, the workgroup loads the mask words of its block's videos for its tile's
// sentences into LDS (a block of the plain plan is 8 words of 16 rows; a block of the ragged plan starts at any video and spans up to
// 9), with the bits outside the block cleared.  If no word has a bit left -- the decision is workgroup-uniform: per-wave ballots
// through LDS and a barrier -- it writes m zero keys per live sentence (and -1 segments) and returns without reading a row.  The
// merge finds every list written.  In the ranked block a wave whose own 64 videos are dark for all 16 sentences skips its MFMA chain
// the same way (wave-uniform); the ragged kernel's passes do not map waves to videos and have no such skip.
#define AL_BLOCK 256        // = SL_BLOCK = SG_BLOCK = SQ_BLOCK = _lib.SHORTLIST_BLOCK = _lib.SHORTLIST_SEG_BLOCK
#define AL_LD (AL_BLOCK + 1)
#define AL_WORDS 8          // mask words of a ranked block: AL_BLOCK / 32
#define AL_SEG_WORDS 9      // of a ragged block, which starts at any video

// The tile's mask words of the videos [v0, v1) into mw[sentence of the tile][word - (v0 >> 5)], NW words a row, bits outside
// [v0, v1) cleared, words past the block zero -> does any bit remain (workgroup-uniform; ends in a barrier).  A sentence slot past S
// reads the last sentence's row (as its query row); v1 <= V, so no word at or past ceil(V / 32) is read.
template <int NW>
__device__ __forceinline__ bool al_load_mask(const int* __restrict__ allow, const int stride, const int s0, const int S, const int v0,
                                             const int v1, int* mw, int* wany, const int tid) {
  const int w0 = v0 >> 5;
  unsigned word = 0u;
  if (tid < 16 * NW) {
    const int sl = tid / NW, w = tid - sl * NW;
    const int lo = max(v0, (w0 + w) * 32), hi = min(v1, (w0 + w) * 32 + 32), bits = hi - lo;
    if (bits > 0) {
      const unsigned in = (bits == 32 ? 0xffffffffu : (1u << bits) - 1u) << (lo & 31);
      word = (unsigned)allow[(long)min(s0 + sl, S - 1) * stride + w0 + w] & in;
    }
    mw[tid] = (int)word;
  }
  const bool any = __ballot(word != 0u) != 0ull;
  if ((tid & 63) == 0) wany[tid >> 6] = any;
  __syncthreads();
  return (wany[0] | wany[1] | wany[2] | wany[3]) != 0;
}

// a dark block's lists: m zero keys per live sentence (and -1 segments where the table is ragged)
__device__ __forceinline__ void al_write_dark(sl_key_t* __restrict__ ws, int* __restrict__ wsr, const int s0, const int S, const int b,
                                              const int nblocks, const int m, const int tid) {
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    const long at = ((long)(s0 + sl) * nblocks + b) * m + i;
    ws[at] = 0ull;
    if (wsr) wsr[at] = -1;
  }
}

// shortlist_block_kernel (retrieve.hip: the tiles, the keys, the sort and the lists are described there) with the table operand Op
// and the mask
template <typename Op>
__global__ __launch_bounds__(256) void shortlist_block_allow_kernel(const Op op, const typename Op::Q* __restrict__ q,
                                                                    const int* __restrict__ allow, const int allow_stride, const int V,
                                                                    const int E, const int S, const int m, const int nblocks,
                                                                    sl_key_t* __restrict__ ws) {
  __shared__ sl_key_t keys[16 * AL_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block]
  __shared__ int mw[16 * AL_WORDS];                           // [sentence of the tile][mask word of the block]
  __shared__ int wany[4];                                     // each wave's "a bit is set"
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, v0 = b * AL_BLOCK + wave * 64;
  const int r = lane & 15, g = lane >> 4;
  if (!al_load_mask<AL_WORDS>(allow, allow_stride, s0, S, b * AL_BLOCK, min(b * AL_BLOCK + AL_BLOCK, V), mw, wany, tid)) {
    al_write_dark(ws, nullptr, s0, S, b, nblocks, m, tid);    // (workgroup-uniform)
    return;
  }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the wave's 64 videos are the words 2 wave and 2 wave + 1 of the 16 rows: lane -> (row lane & 15, word (lane >> 4) & 1)
  if (__ballot(mw[r * AL_WORDS + 2 * wave + (g & 1)] != 0) != 0ull) {
    // (a row past S or V reads the last row instead: its scores become no keys below)
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
      const bool ok = v < V && s0 + sl < S && ((mw[sl * AL_WORDS + (at >> 5)] >> (at & 31)) & 1);
      keys[sl * AL_BLOCK + at] = ok ? sl_key(acc[j][i], v) : 0ull;
    }
  __syncthreads();
  sl_sort_desc<AL_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    ws[((long)(s0 + sl) * nblocks + b) * m + i] = keys[sl * AL_BLOCK + i];
  }
}

// shortlist_segments_kernel (retrieve_seg.hip: the block plan, the passes, the segmented maximum, the states and the keys are described
// there) with the table operand Op and the mask, which is over VIDEOS.  As there, every index read from the device tables is clamped.
template <typename Op>
__global__ __launch_bounds__(256) void shortlist_segments_allow_kernel(const Op op, const typename Op::Q* __restrict__ q,
                                                                       const int* __restrict__ offsets, const int* __restrict__ blk_vid,
                                                                       const int* __restrict__ allow, const int allow_stride, const int R,
                                                                       const int V, const int E, const int S, const int m,
                                                                       const int nblocks, sl_key_t* __restrict__ ws, int* __restrict__ wsr) {
  __shared__ sl_key_t keys[16 * AL_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block], states then keys
  __shared__ float sc[16 * AL_LD];                            // [sentence of the tile][row of the pass]; after the last pass, as
  int* const seg = reinterpret_cast<int*>(sc);                // integers, the winning segment of [sentence][video]
  __shared__ int voff[AL_BLOCK + 4];                          // the block's slice of the offsets, nv + 1 words
  __shared__ int wlong[4];                                    // each wave's longest run
  __shared__ int mw[16 * AL_SEG_WORDS];                       // [sentence of the tile][mask word from the block's first]
  __shared__ int wany[4];                                     // each wave's "a bit is set"
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16;
  const int r = lane & 15, g = lane >> 4;
  const int v0 = min(max(blk_vid[b], 0), V), v1 = min(max(blk_vid[b + 1], v0), min(v0 + AL_BLOCK, V)), nv = v1 - v0;
  if (!al_load_mask<AL_SEG_WORDS>(allow, allow_stride, s0, S, v0, v1, mw, wany, tid)) {
    al_write_dark(ws, wsr, s0, S, b, nblocks, m, tid);        // (workgroup-uniform; also a block without videos)
    return;
  }
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
  const int longest = min(max(max(wlong[0], wlong[1]), max(wlong[2], wlong[3])), AL_BLOCK);   // (of one pass at most)
  int plg = 0;                                                // P = 1 << plg lanes per (sentence, video): one per 16 rows of the longest run
  while (plg < 4 && (16 << plg) < longest) ++plg;
  const int P = 1 << plg;
  const int r0 = voff[0], r1 = voff[nv];
  // (a sentence past S reads the last one instead: its states become no keys below)
  const typename Op::Q* qrow = q + (long)min(s0 + r, S - 1) * E;
  for (int p0 = r0; p0 < r1; p0 += AL_BLOCK) {
    const int p1 = min(p0 + AL_BLOCK, r1), rw = p0 + wave * 64;
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
        for (int i = 0; i < 4; ++i) sc[(4 * g + i) * AL_LD + wave * 64 + 16 * j + r] = acc[j][i];
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
      const float* mine = sc + sl * AL_LD;
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
    const int v = v0 + min(vi, AL_BLOCK - 1);                 // (v - 32 (v0 >> 5) < 32 AL_SEG_WORDS: inside mw)
    const bool may = (mw[sl * AL_SEG_WORDS + (v >> 5) - (v0 >> 5)] >> (v & 31)) & 1;
    const bool ok = vi < nv && s0 + sl < S && o > 0x007fffffu && o < 0xff800000u && may;
    seg[p] = (int)~(unsigned)st;
    keys[p] = ok ? ((sl_key_t)o << 32) | (sl_key_t)(~(unsigned)(v0 + vi)) : 0ull;
  }
  __syncthreads();
  if (lenlg == 4) sl_sort_desc<16, 256>(keys, 16, tid);       // (block-uniform)
  else if (lenlg == 6) sl_sort_desc<64, 256>(keys, 16, tid);
  else sl_sort_desc<AL_BLOCK, 256>(keys, 16, tid);
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
// The entries: one argument record, one list of checks (each twin's, then the mask's), one launch switch.

struct AlArgs {
  bool ragged, q8;                                            // offsets, blk_vid, vid_blk, R, nblocks, rows are read; scales is read
  const void* table;                                          // emb, or the codes
  const void* scales;
  const void* queries;
  const int32_t *offsets, *blk_vid, *vid_blk;
  const int32_t* allow;
  int allow_stride, R, V, nblocks, E, S, n, dtype;
  void* ws;
  int ws_keys;
  int32_t* ids;
  float* scores;
  int32_t* counts;
  int32_t* rows;
};

static int al_check(const char* what, const AlArgs& a, const int cap) {
  const bool ragged = a.ragged, q8 = a.q8;
  DRN_CHECK_ARG(a.table && (!q8 || a.scales) && a.queries && a.allow && a.ws && a.ids && a.scores && a.counts &&
                    (!ragged || (a.offsets && a.blk_vid && a.vid_blk && a.rows)),
                "%s: null pointer", what);
  if (ragged)
    DRN_CHECK_ARG(a.R >= 1 && a.V >= 1 && a.E >= 1 && a.S >= 1, "%s: bad args (R = %d rows, V = %d videos, E = %d columns, S = %d sentences)",
                  what, a.R, a.V, a.E, a.S);
  else
    DRN_CHECK_ARG(a.V >= 1 && a.E >= 1 && a.S >= 1, "%s: bad args (V = %d videos, E = %d columns, S = %d sentences)", what, a.V, a.E, a.S);
  if (q8) DRN_CHECK_ARG(a.E % MX8_BLOCK == 0, "%s: E = %d is not a multiple of the block of %d columns", what, a.E, MX8_BLOCK);
  if (ragged)
    DRN_CHECK_ARG(a.nblocks >= 1 && a.nblocks <= a.V && (long)a.nblocks * AL_BLOCK >= a.V, "%s: %d blocks outside [ceil(V / %d), V] for V = %d videos",
                  what, a.nblocks, AL_BLOCK, a.V);
  DRN_CHECK_ARG(a.n >= 1 && a.n <= cap, "%s: n = %d outside [1, %d]", what, a.n, cap);
  DRN_CHECK_ARG(a.dtype == DRN_F32 || a.dtype == DRN_BF16, "%s: dtype %d (float32 / bfloat16 only)", what, a.dtype);
  DRN_CHECK_ARG(((uintptr_t)a.table & 15) == 0 && ((uintptr_t)a.queries & 15) == 0 && ((uintptr_t)a.ws & 7) == 0,
                "%s: the table and the queries must be 16-byte aligned, the workspace 8-byte aligned", what);
  DRN_CHECK_ARG(a.allow_stride == 0 || a.allow_stride == cdiv(a.V, 32),
                "%s: allow_stride = %d is neither 0 (one mask for all sentences) nor ceil(V / 32) = %d (one row per sentence)", what,
                a.allow_stride, cdiv(a.V, 32));
  DRN_CHECK_ARG(((uintptr_t)a.allow & 3) == 0, "%s: the mask must be 4-byte aligned", what);
  const int m = a.n < AL_BLOCK ? a.n : AL_BLOCK, nblocks = ragged ? a.nblocks : cdiv(a.V, AL_BLOCK), tiles = cdiv(a.S, 16);
  const long lists = (long)a.S * nblocks * m, need = ragged ? lists + (lists + 1) / 2 : lists;
  if (ragged)
    DRN_CHECK_ARG(need <= 0x7fffffffL && a.ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (1.5 * S * blocks * min(n, %d))",
                  what, a.ws_keys, need, AL_BLOCK);
  else
    DRN_CHECK_ARG(need <= 0x7fffffffL && a.ws_keys >= need, "%s: the workspace holds %d keys, %ld are needed (S * ceil(V / %d) * min(n, %d))",
                  what, a.ws_keys, need, AL_BLOCK, AL_BLOCK);
  DRN_CHECK_ARG(tiles <= 65535, "%s: S = %d, more than 65535 tiles of 16 sentences", what, a.S);
  return DRN_OK;
}

// phase one with the operand Op, then the merge (and the segment look-up) of the unmasked entries -- DEEP: the deep merge of
// retrieve_deep.hip in its place.  RAGGED is a compile-time switch: an operand instantiates only the kernel it is launched on; deep is
// a run-time one: both depths launch the same phase-one instantiations
template <bool RAGGED, typename Op>
static void al_launch(const Op op, const AlArgs& a, const bool deep, hipStream_t stream) {
  typedef typename Op::Q Q;
  const int m = a.n < AL_BLOCK ? a.n : AL_BLOCK, nblocks = RAGGED ? a.nblocks : cdiv(a.V, AL_BLOCK);
  const dim3 grid(nblocks, cdiv(a.S, 16));
  sl_key_t* lists_k = (sl_key_t*)a.ws;
  if constexpr (!RAGGED) {
    shortlist_block_allow_kernel<Op><<<grid, 256, 0, stream>>>(op, (const Q*)a.queries, a.allow, a.allow_stride, a.V, a.E, a.S, m, nblocks,
                                                                lists_k);
    (deep ? sl_launch_merge_deep : sl_launch_merge)(lists_k, a.S, a.n, m, nblocks, a.ids, a.scores, a.counts, stream);
  } else {
    int* lists_r = (int*)(lists_k + (long)a.S * nblocks * m);
    shortlist_segments_allow_kernel<Op><<<grid, 256, 0, stream>>>(op, (const Q*)a.queries, a.offsets, a.blk_vid, a.allow, a.allow_stride,
                                                                   a.R, a.V, a.E, a.S, m, nblocks, lists_k, lists_r);
    (deep ? sl_launch_merge_deep : sl_launch_merge)(lists_k, a.S, a.n, m, nblocks, a.ids, a.scores, a.counts, stream);
    sl_launch_segment_rows(lists_k, lists_r, a.vid_blk, a.ids, a.V, a.S, a.n, m, nblocks, a.rows, stream);
  }
}

template <bool RAGGED>
static void al_launch_table(const AlArgs& a, const bool deep, hipStream_t stream) {
  const uint8_t *codes = (const uint8_t*)a.table, *scales = (const uint8_t*)a.scales;
  const bool bf16 = a.dtype == DRN_BF16;
  // (a quantised bf16 chain keeps two scale blocks of loads in flight in the ranked block, one in the ragged kernel: retrieve_q8.hip
  // says why)
  if (!a.q8 && bf16) al_launch<RAGGED>(AlPlain<bf16_t>{(const bf16_t*)a.table}, a, deep, stream);
  else if (!a.q8) al_launch<RAGGED>(AlPlain<float>{(const float*)a.table}, a, deep, stream);
  else if (bf16) al_launch<RAGGED>(AlQ8<bf16_t, RAGGED ? 1 : 2>{codes, scales}, a, deep, stream);
  else al_launch<RAGGED>(AlQ8<float, 1>{codes, scales}, a, deep, stream);
}

static int al_run(const char* what, const AlArgs& a, void* stream, const bool deep = false) {
  drn_clear_status();
  if (const int rc = al_check(what, a, deep ? DRN_SHORTLIST_DEEP_MAX : DRN_SHORTLIST_MAX)) return rc;
  if (a.ragged) al_launch_table<true>(a, deep, (hipStream_t)stream);
  else al_launch_table<false>(a, deep, (hipStream_t)stream);
  return drn_launch_status(what);
}

extern "C" int drn_shortlist_topn_allow(const void* emb, const void* queries, const int32_t* allow, int allow_stride, int V, int E, int S,
                                        int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts,
                                        void* stream) {
  const AlArgs a = {false, false, emb, nullptr, queries, nullptr, nullptr, nullptr, allow, allow_stride, 0, V, 0, E, S, n, dtype, ws, ws_keys,
                    ids, scores, counts, nullptr};
  return al_run("drn_shortlist_topn_allow", a, stream);
}

extern "C" int drn_shortlist_segments_topn_allow(const void* emb, const void* queries, const int32_t* offsets, const int32_t* blk_vid,
                                                 const int32_t* vid_blk, const int32_t* allow, int allow_stride, int R, int V, int nblocks,
                                                 int E, int S, int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores,
                                                 int32_t* counts, int32_t* rows, void* stream) {
  const AlArgs a = {true, false, emb, nullptr, queries, offsets, blk_vid, vid_blk, allow, allow_stride, R, V, nblocks, E, S, n, dtype,
                    ws, ws_keys, ids, scores, counts, rows};
  return al_run("drn_shortlist_segments_topn_allow", a, stream);
}

extern "C" int drn_shortlist_topn_q8_allow(const uint8_t* codes, const uint8_t* scales, const void* queries, const int32_t* allow,
                                           int allow_stride, int V, int E, int S, int n, int dtype, void* ws, int ws_keys, int32_t* ids,
                                           float* scores, int32_t* counts, void* stream) {
  const AlArgs a = {false, true, codes, scales, queries, nullptr, nullptr, nullptr, allow, allow_stride, 0, V, 0, E, S, n, dtype, ws, ws_keys,
                    ids, scores, counts, nullptr};
  return al_run("drn_shortlist_topn_q8_allow", a, stream);
}

extern "C" int drn_shortlist_segments_topn_q8_allow(const uint8_t* codes, const uint8_t* scales, const void* queries,
                                                    const int32_t* offsets, const int32_t* blk_vid, const int32_t* vid_blk,
                                                    const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S, int n,
                                                    int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts,
                                                    int32_t* rows, void* stream) {
  const AlArgs a = {true, true, codes, scales, queries, offsets, blk_vid, vid_blk, allow, allow_stride, R, V, nblocks, E, S, n, dtype,
                    ws, ws_keys, ids, scores, counts, rows};
  return al_run("drn_shortlist_segments_topn_q8_allow", a, stream);
}

// The DEEP shortlist (include/drn_hip.h): all four tables behind one entry, by the convention of the rank and rerank entries -- scales ==
// NULL is a plain table, offsets == NULL one row per video.  Host code only: phase one is the eight instantiations above, which already
// write m up to 256; the merge is sl_launch_merge_deep (retrieve_deep.hip).  The mask is required (the caller without a filter passes
// an all-ones row with stride 0), so no unmasked phase one is instantiated for it.
extern "C" int drn_shortlist_deep(const void* table, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                  const int32_t* blk_vid, const int32_t* vid_blk, const int32_t* allow, int allow_stride, int R, int V,
                                  int nblocks, int E, int S, int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores,
                                  int32_t* counts, int32_t* rows, void* stream) {
  const char* what = "drn_shortlist_deep";
  const bool ragged = offsets != nullptr;
  DRN_CHECK_ARG(ragged || !(blk_vid || vid_blk || rows),
                "%s: null pointer: offsets is NULL (one row per video), so blk_vid, vid_blk and rows must be NULL too", what);
  const AlArgs a = {ragged, scales != nullptr, table, scales, queries, offsets, blk_vid, vid_blk, allow, allow_stride, ragged ? R : 0, V,
                    ragged ? nblocks : 0, E, S, n, dtype, ws, ws_keys, ids, scores, counts, rows};
  return al_run(what, a, stream, true);
}

// ---------------------------------------------------------------------------------------------------------------------------
// mask [S][V] bool bytes (non-zero = allowed) -> words [S][W], W = ceil(V / 32): one wavefront per 64 videos of a row reads a byte a
// lane, and its ballot is two words.  Every word is written, with zero bits past V.
__global__ __launch_bounds__(256) void pack_allow_kernel(const uint8_t* __restrict__ mask, const int V, const int W, const int W64,
                                                         const long waves, int* __restrict__ words) {
  const int lane = threadIdx.x & 63;
  const long wv = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= waves) return;                                    // (wave-uniform)
  const long s = wv / W64;
  const int k = (int)(wv - s * W64), v = 64 * k + lane;
  const unsigned long long set = __ballot(v < V && mask[s * V + v] != 0);
  if (lane == 0) words[s * W + 2 * k] = (int)(unsigned)set;
  if (lane == 1 && 2 * k + 1 < W) words[s * W + 2 * k + 1] = (int)(unsigned)(set >> 32);
}

extern "C" int drn_pack_allow(const uint8_t* mask, int S, int V, int32_t* words, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(mask && words, "drn_pack_allow: null pointer");
  DRN_CHECK_ARG(S >= 1 && V >= 1, "drn_pack_allow: bad args (S = %d rows, V = %d videos)", S, V);
  DRN_CHECK_ARG(((uintptr_t)words & 3) == 0, "drn_pack_allow: the words must be 4-byte aligned");
  const int W = cdiv(V, 32);
  const int W64 = cdiv(V, 64);
  const long waves = (long)S * W64;
  DRN_CHECK_ARG((waves + 3) / 4 <= 0x7fffffffL, "drn_pack_allow: S = %d rows of %d videos are more than 2^31 workgroups", S, V);
  pack_allow_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, (hipStream_t)stream>>>(mask, V, W, W64, waves, words);
  return drn_launch_status("drn_pack_allow");
}
