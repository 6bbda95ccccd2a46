// What the two shortlist translation units share (retrieve.hip: one vector per video; retrieve_seg.hip: a ragged run of segment vectors
// per video): the 64-bit candidate key, the bitonic sort, the fragment loaders and the MFMA step of one (sentence, row) score, and the
// host-side launch of the merging kernel, which lives in retrieve.hip and serves both.  retrieve_q8.hip ranks the same two tables kept in
// block-scaled FP8: its table operand is sl_frag_q8 below, everything after the scores is what is declared here.  retrieve_allow.hip
// ranks all four under an allow mask: the plain chain, and the FP8 chain sq_scores below, which it shares with retrieve_q8.hip.
// retrieve_late.hip ranks the ragged tables by late interaction (per-token queries) on the table operands AlPlain / AlQ8 below.
// retrieve_rank.hip counts, on the same operands and keys, the videos that precede a named one: no sort, no list.
// retrieve_rerank.hip scores, on the same operands, keys and merge, only the (sentence, video) pairs a candidate list names.
// retrieve_shard.hip merges the finished lists of several tables: the same key, rebuilt from (score, base + id), and the same sort.
// retrieve_deep.hip merges the lists of phase one into lists of up to 1024: the same key and sort, one workgroup per sentence.
#pragma once
#include "common.h"
#include "mx8.h"

typedef unsigned long long sl_key_t;

// the score as an unsigned word that orders as the float does (-0 folded into +0); a finite score's word is never 0
__device__ __forceinline__ unsigned sl_word(float score) {
  const unsigned b = __float_as_uint(score + 0.f);                              // (-0 + 0 = +0)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ sl_key_t sl_key(float score, int v) {
  if (!isfinite(score)) return 0ull;
  return ((sl_key_t)sl_word(score) << 32) | (sl_key_t)(~(unsigned)v);
}
__device__ __forceinline__ float sl_score(sl_key_t k) {
  const unsigned o = (unsigned)(k >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ int sl_video(sl_key_t k) { return (int)~(unsigned)k; }

// Bitonic sort, descending, of ROWS rows of LEN keys each by NT threads (LEN a power of two).
template <int LEN, int NT>
__device__ __forceinline__ void sl_sort_desc(sl_key_t* keys, const int rows, const int tid) {
  const int total = rows * (LEN / 2);
  for (int k = 2; k <= LEN; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < total; p += NT) {
        const int row = p / (LEN / 2), t = p - row * (LEN / 2);
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        sl_key_t* r = keys + row * LEN;
        const sl_key_t a = r[i], b = r[l];
        const bool desc = (i & k) == 0;
        if (desc ? a < b : a > b) { r[i] = b; r[l] = a; }
      }
      __syncthreads();
    }
}

// 8 bf16 / 4 fp32 of `row` from column c0: one 16-byte load, or (the tail, a row that is not 16-byte aligned) element by element
// with zeros past E
__device__ __forceinline__ bf16x8 sl_frag(const bf16_t* row, const int c0) { return *reinterpret_cast<const bf16x8*>(row + c0); }
__device__ __forceinline__ f32x4 sl_frag(const float* row, const int c0) { return *reinterpret_cast<const f32x4*>(row + c0); }
__device__ __forceinline__ bf16x8 sl_frag_tail(const bf16_t* row, const int c0, const int E) {
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = c0 + j < E ? row[c0 + j] : (bf16_t)0.f;
  return f;
}
__device__ __forceinline__ f32x4 sl_frag_tail(const float* row, const int c0, const int E) {
  f32x4 f;
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = c0 + j < E ? row[c0 + j] : 0.f;
  return f;
}
__device__ __forceinline__ f32x4 sl_mfma(const bf16x8 a, const bf16x8 b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x4 sl_mfma(const f32x4 a, const f32x4 b, f32x4 acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], acc, 0, 0, 0);
  return acc;
}
// The table operand of a block-scaled FP8 table (drn_amd/index.py mx8_quantize is the format): the PER_LANE code bytes of `codes` from
// column c0, as loaded, and -- with their block's scale byte -- the fragment sl_frag would load from the dequantised row.  code -> fp32
// by v_cvt_pk_f32_fp8 (OCP on gfx950), times 2^(scale - 127) (the scale byte placed in the fp32 exponent field), then -> bf16 for a
// bf16 chain: every step is exact (four significant bits; the format keeps every value zero or a normal number), the statements of
// gate_gather_packed_q8_kernel (qindex.hip).  c0 is a multiple of PER_LANE, which divides 32: a lane's columns lie inside one block.
__device__ __forceinline__ u32x2 sl_codes_q8(const uint8_t* codes, const int c0, bf16_t) { return *reinterpret_cast<const u32x2*>(codes + c0); }
__device__ __forceinline__ unsigned sl_codes_q8(const uint8_t* codes, const int c0, float) { return *reinterpret_cast<const unsigned*>(codes + c0); }
__device__ __forceinline__ bf16x8 sl_frag_q8(const u32x2 w, const unsigned scale) {
  const float sc = __uint_as_float(scale << 23);
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
    f[4 * j] = (bf16_t)(lo[0] * sc); f[4 * j + 1] = (bf16_t)(lo[1] * sc); f[4 * j + 2] = (bf16_t)(hi[0] * sc); f[4 * j + 3] = (bf16_t)(hi[1] * sc);
  }
  return f;
}
__device__ __forceinline__ f32x4 sl_frag_q8(const unsigned w, const unsigned scale) {
  const float sc = __uint_as_float(scale << 23);
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  return f32x4{lo[0] * sc, lo[1] * sc, hi[0] * sc, hi[1] * sc};
}
template <typename T> struct SlStep;
template <> struct SlStep<bf16_t> { static constexpr int COLS = 32, PER_LANE = 8; };
template <> struct SlStep<float> { static constexpr int COLS = 16, PER_LANE = 4; };

// acc[j] += q[16 sentences] x the dequantised rows crow[j] / srow[j] (j = 0..3) over NB scale blocks from column c: every load of their
// NB * 32 / COLS steps is issued before the first conversion, then the steps run in ascending order
template <typename T, int NB>
__device__ __forceinline__ void sq_blocks(const T* qrow, const uint8_t* const (&crow)[4], const uint8_t* const (&srow)[4], const int c,
                                          const int g, f32x4 (&acc)[4]) {
  constexpr int COLS = SlStep<T>::COLS, PER_LANE = SlStep<T>::PER_LANE, STEPS = NB * MX8_BLOCK / COLS;
  decltype(sl_frag(qrow, 0)) a[STEPS];
  decltype(sl_codes_q8(crow[0], 0, T())) w[STEPS][4];
  unsigned sb[NB][4];
#pragma unroll
  for (int u = 0; u < NB; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) sb[u][j] = srow[j][c / MX8_BLOCK + u];
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int c0 = c + k * COLS + g * PER_LANE;
    a[k] = sl_frag(qrow, c0);
#pragma unroll
    for (int j = 0; j < 4; ++j) w[k][j] = sl_codes_q8(crow[j], c0, T());
  }
#pragma unroll
  for (int k = 0; k < STEPS; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = sl_mfma(a[k], sl_frag_q8(w[k][j], sb[k * COLS / MX8_BLOCK][j]), acc[j]);
}

// all K-steps of E in ascending order, NB blocks at a time
template <typename T, int NB>
__device__ __forceinline__ void sq_scores(const T* qrow, const uint8_t* const (&crow)[4], const uint8_t* const (&srow)[4], const int E,
                                          const int g, f32x4 (&acc)[4]) {
  int c = 0;
  for (; c + NB * MX8_BLOCK <= E; c += NB * MX8_BLOCK) sq_blocks<T, NB>(qrow, crow, srow, c, g, acc);
  if (NB > 1 && c < E) sq_blocks<T, 1>(qrow, crow, srow, c, g, acc);      // (an odd number of blocks)
}

// THE TABLE OPERAND of the kernels that are templated on it (retrieve_allow.hip, retrieve_late.hip): AlPlain<T> loads a row's fragments
// (sl_frag / sl_frag_tail), AlQ8<T, NB> builds them from codes and scale bytes (sq_scores).  Either runs the chain of the kernel it names.
template <typename T>
struct AlPlain {
  typedef T Q;
  const T* emb;
  // acc[j] += q[16 sentences] x the rows row[j] (j = 0..3): shortlist_block_kernel's chain (retrieve.hip)
  __device__ __forceinline__ void scores(const T* qrow, const long (&row)[4], const int E, const int g, f32x4 (&acc)[4]) const {
    constexpr int COLS = SlStep<T>::COLS, PER_LANE = SlStep<T>::PER_LANE;
    const T* erow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) erow[j] = emb + row[j] * E;
    // whole steps on 16-byte loads where every row starts on a 16-byte boundary (the tables are 16-byte aligned), then the rest
    const int whole = E % PER_LANE == 0 ? E / COLS * COLS : 0;
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
  }
};

template <typename T, int NB>
struct AlQ8 {
  typedef T Q;
  const uint8_t* codes;
  const uint8_t* scales;
  // the same from a block-scaled FP8 table: shortlist_block_q8_kernel's chain (retrieve_q8.hip); E % MX8_BLOCK == 0
  __device__ __forceinline__ void scores(const T* qrow, const long (&row)[4], const int E, const int g, f32x4 (&acc)[4]) const {
    const uint8_t* crow[4];
    const uint8_t* srow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      crow[j] = codes + row[j] * E;
      srow[j] = scales + row[j] * (E / MX8_BLOCK);
    }
    sq_scores<T, NB>(qrow, crow, srow, E, g, acc);
  }
};

// shortlist_merge_kernel (retrieve.hip) on `stream`: sentence s merges its nblocks sorted lists of m keys, ws[s][block][0..m), into
// ids, scores [S][n] and counts [S].  Not part of the C ABI.
void sl_launch_merge(const sl_key_t* ws, int S, int n, int m, int nblocks, int32_t* ids, float* scores, int32_t* counts, hipStream_t stream);
// shortlist_merge_deep_kernel (retrieve_deep.hip) on `stream`: the same contract for n up to DRN_SHORTLIST_DEEP_MAX, m = min(n, 256) --
// one workgroup of 256 threads per sentence, four lists in flight.  Not part of the C ABI.
void sl_launch_merge_deep(const sl_key_t* ws, int S, int n, int m, int nblocks, int32_t* ids, float* scores, int32_t* counts, hipStream_t stream);
// shortlist_segment_rows_kernel (retrieve_seg.hip) on `stream`: the winning segment of each listed (sentence, place), looked up in the
// lists ws / wsr of the video's block, into rows [S][n].  Not part of the C ABI.
void sl_launch_segment_rows(const sl_key_t* ws, const int* wsr, const int32_t* vid_blk, const int32_t* ids, int V, int S, int n, int m,
                            int nblocks, int32_t* rows, hipStream_t stream);
