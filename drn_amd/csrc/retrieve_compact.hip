// Compacting a corpus kept as several tables into ONE (drn_amd/retrieve.py, ShardedShortlister.compact): the videos a packed mask
// keeps, in corpus order, in a new table; the dropped ones gone.
//   drn_compact_plan   one launch per shard, in stream order: the shard's slice of `positions` (new position, -1 where dropped), on
//                      ragged shards the new offsets of its kept videos, and the running carry (videos kept, rows kept);
//   drn_compact_rows   one launch per shard: the kept rows of the shard moved to their places in the destination, plain -> plain,
//                      FP8 -> FP8 (codes and scale bytes as they are) or FP8 -> plain (dequantised in registers).
// (The kernels live here and not in retrieve_shard.hip, whose kernel list is pinned by its resource test.)
#include "common.h"
#include "mx8.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// THE PLAN is an exclusive scan over the corpus's videos of (kept ? 1 : 0, kept ? rows : 0), cut at the shard boundaries.  ONE
// workgroup walks one shard, CP_THREADS * CP_ITEMS videos a step: a thread takes CP_ITEMS neighbouring videos (their mask bits lie in
// one word: CP_ITEMS divides 32), the pair is packed into 64 bits -- videos in the low word, rows in the high one, each below 2^31, so
// one add carries both --, a wavefront scans by shuffles, the wavefronts' totals meet in LDS (two buffers, one barrier a step) and the
// running total stays in a register.  The carry of the shards before comes from carry[k], written by the launch before this one in
// stream order (shard 0 starts from zero and writes it), and the total goes to carry[k + 1]: no workgroup waits on another, there is no
// flag, no look-back and no atomic.  A new offset is written at the new position of its video, and new_offsets[videos so far] = rows
// so far closes the table after every shard (the next shard's first kept video writes the same value there).  An index at or past
// `cap` is never written, whatever the carry holds.
#define CP_THREADS 1024
#define CP_ITEMS 4
static_assert(32 % CP_ITEMS == 0, "a thread's mask bits lie in one word");

__global__ __launch_bounds__(CP_THREADS) void compact_plan_kernel(const int* __restrict__ keep, const int* __restrict__ offsets, const int V,
                                                                  const int first, const int cap, int* __restrict__ carry,
                                                                  int* __restrict__ positions, int* __restrict__ new_offsets) {
  __shared__ unsigned long long tot[2][CP_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long run = 0ull;                               // (rows kept << 32) | videos kept, before the videos of this step
  if (!first) run = ((unsigned long long)(unsigned)max(carry[1], 0) << 32) | (unsigned)max(carry[0], 0);
  else if (tid == 0) carry[0] = carry[1] = 0;
  int it = 0;
  for (long base = 0; base < V; base += CP_THREADS * CP_ITEMS, ++it) {
    const long v0 = base + (long)tid * CP_ITEMS;
    const unsigned word = v0 < V ? (keep ? (unsigned)keep[v0 >> 5] : ~0u) : 0u;
    const unsigned bits = word >> (v0 & 31);
    unsigned long long inc[CP_ITEMS], sum = 0ull;
#pragma unroll
    for (int i = 0; i < CP_ITEMS; ++i) {
      const bool in = v0 + i < V;
      const int len = !in ? 0 : offsets ? max(offsets[v0 + i + 1] - offsets[v0 + i], 0) : 1;
      inc[i] = (in && ((bits >> i) & 1u)) ? (((unsigned long long)(unsigned)len << 32) | 1ull) : 0ull;
      sum += inc[i];
    }
    unsigned long long scan = sum;                              // inclusive over the wavefront's threads
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long up = __shfl_up(scan, d, 64);
      if (lane >= d) scan += up;
    }
    if (lane == 63) tot[it & 1][wave] = scan;
    __syncthreads();
    unsigned long long before = run + scan - sum;
#pragma unroll
    for (int w = 0; w < CP_THREADS / 64; ++w) {
      const unsigned long long t = tot[it & 1][w];
      run += t;
      if (w < wave) before += t;
    }
#pragma unroll
    for (int i = 0; i < CP_ITEMS; ++i) {
      if (v0 + i >= V) break;
      const int p = (int)(unsigned)before;
      positions[v0 + i] = inc[i] ? p : -1;
      if (inc[i] && new_offsets && p >= 0 && p < cap) new_offsets[p] = (int)(before >> 32);
      before += inc[i];
    }
  }
  if (tid == 0) {
    const int videos = (int)(unsigned)run, rows = (int)(run >> 32);
    carry[2] = videos;
    carry[3] = rows;
    if (new_offsets && videos >= 0 && videos < cap) new_offsets[videos] = rows;
  }
}

extern "C" int drn_compact_plan(const int32_t* keep, const int32_t* offsets, int V, int k, int K, int cap, int32_t* carry,
                                int32_t* positions, int32_t* new_offsets, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(carry && positions, "drn_compact_plan: null pointer");
  DRN_CHECK_ARG((offsets == nullptr) == (new_offsets == nullptr),
                "drn_compact_plan: offsets and new_offsets must both be given (a ragged shard) or neither");
  DRN_CHECK_ARG(K >= 1 && K <= DRN_SHARDS_MAX, "drn_compact_plan: K = %d shards outside [1, %d]", K, DRN_SHARDS_MAX);
  DRN_CHECK_ARG(k >= 0 && k < K, "drn_compact_plan: shard k = %d outside [0, %d)", k, K);
  DRN_CHECK_ARG(V >= 1, "drn_compact_plan: bad args (V = %d videos)", V);
  DRN_CHECK_ARG(new_offsets == nullptr || cap >= 2, "drn_compact_plan: cap = %d entries of new_offsets below 2", cap);
  DRN_CHECK_ARG((((uintptr_t)keep | (uintptr_t)offsets | (uintptr_t)carry | (uintptr_t)positions | (uintptr_t)new_offsets) & 3) == 0,
                "drn_compact_plan: every buffer must be 4-byte aligned");
  compact_plan_kernel<<<1, CP_THREADS, 0, (hipStream_t)stream>>>(keep, offsets, V, k == 0, cap, carry + 2 * k, positions, new_offsets);
  return drn_launch_status("drn_compact_plan");
}

// ---------------------------------------------------------------------------------------------------------------------------
// THE ROWS.  One wavefront per source video (four a workgroup, a bounded grid and a grid-stride loop): p = positions[v] is the video's
// place in the new table; a dropped video (p < 0) and one whose place is not a place (p >= dst_videos) is left at once.  Its source
// rows are src_offsets[v] .. src_offsets[v + 1] - 1 clamped into [0, src_rows) -- row v itself on a table of one row a video -- and
// row j of the video goes to destination row dst_offsets[p] + j (row p); `dst` is a WINDOW of the destination, its rows
// [dst_row0, dst_row0 + dst_rows), and a row outside it is not written: that is how a staging buffer takes a table in chunks, and why
// nothing is written outside `dst` whatever the tables hold.  Row addresses are 64-bit (rows * E may pass 2^31).
//   CR_COPY   the row's E elements of ES bytes as they are -- a plain row, or the codes of an FP8 row, whose E / 32 scale bytes follow
//             byte by byte: nothing is requantised;
//   CR_DEQ    float(code) * 2^(scale - 127) -> T, exact in bf16 and fp32: sl_frag_q8 (shortlist.h), the statements the q8 shortlist
//             kernels score with.
// VEC: 16-byte accesses (CR_DEQ: 8 codes in, 8 values out a lane) when the host found every base pointer and row pitch a multiple of 16
// bytes (8 for the codes CR_DEQ reads); otherwise one element a lane.  At E = 512 a bf16 row is one 16-byte access a lane.
#define CR_COPY 0
#define CR_DEQ 1

struct CrArgs {
  const uint8_t* src;          // the plain rows or the codes
  const uint8_t* src_scales;   // [src_rows][E / 32] or null
  const int* src_offsets;      // [V + 1] or null
  const int* positions;        // [V]
  const int* dst_offsets;      // [dst_videos + 1] or null
  uint8_t* dst;
  uint8_t* dst_scales;         // [dst_rows][E / 32] or null
  int V, src_rows, E, dst_videos, dst_row0, dst_rows;
};

template <int ES, bool VEC>
__device__ __forceinline__ void cr_copy(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, const int E, const int lane) {
  if (VEC) {
    for (int i = lane * 16; i < E * ES; i += 64 * 16) *reinterpret_cast<u32x4*>(d + i) = *reinterpret_cast<const u32x4*>(s + i);
  } else if (ES == 4) {
    for (int c = lane; c < E; c += 64) reinterpret_cast<uint32_t*>(d)[c] = reinterpret_cast<const uint32_t*>(s)[c];
  } else if (ES == 2) {
    for (int c = lane; c < E; c += 64) reinterpret_cast<uint16_t*>(d)[c] = reinterpret_cast<const uint16_t*>(s)[c];
  } else {
    for (int c = lane; c < E; c += 64) d[c] = s[c];
  }
}

template <bool VEC>
__device__ __forceinline__ void cr_deq(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, bf16_t* __restrict__ d, const int E,
                                       const int lane) {
  if (VEC) {
    for (int c = lane * 8; c < E; c += 64 * 8)
      *reinterpret_cast<bf16x8*>(d + c) = sl_frag_q8(*reinterpret_cast<const u32x2*>(codes + c), (unsigned)scales[c >> 5]);
  } else {
    for (int c = lane; c < E; c += 64)
      d[c] = (bf16_t)(__builtin_amdgcn_cvt_f32_fp8((int)codes[c], 0) * __uint_as_float((unsigned)scales[c >> 5] << 23));
  }
}
template <bool VEC>
__device__ __forceinline__ void cr_deq(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, float* __restrict__ d, const int E,
                                       const int lane) {
  if (VEC) {
    for (int c = lane * 8; c < E; c += 64 * 8) {
      const u32x2 w = *reinterpret_cast<const u32x2*>(codes + c);
      const unsigned scale = scales[c >> 5];
      *reinterpret_cast<f32x4*>(d + c) = sl_frag_q8(w[0], scale);
      *reinterpret_cast<f32x4*>(d + c + 4) = sl_frag_q8(w[1], scale);
    }
  } else {
    for (int c = lane; c < E; c += 64)
      d[c] = __builtin_amdgcn_cvt_f32_fp8((int)codes[c], 0) * __uint_as_float((unsigned)scales[c >> 5] << 23);
  }
}

// T: CR_COPY moves elements of sizeof(T) bytes (uint8_t: the codes of an FP8 row); CR_DEQ writes values of type T
template <int MODE, typename T, bool VEC>
__global__ __launch_bounds__(256) void compact_rows_kernel(const CrArgs a) {
  const int lane = threadIdx.x & 63;
  const long waves = (long)gridDim.x * 4;
  const int SB = a.E / MX8_BLOCK;                              // scale bytes a row
  for (long v = (long)blockIdx.x * 4 + (threadIdx.x >> 6); v < a.V; v += waves) {          // (wave-uniform)
    const int p = a.positions[v];
    if (p < 0 || p >= a.dst_videos) continue;
    long s0 = v, s1 = v + 1, d0 = p;
    if (a.src_offsets) {
      s0 = a.src_offsets[v];
      s1 = a.src_offsets[v + 1];
      d0 = a.dst_offsets[p];
    }
    s0 = max(s0, 0L);
    s1 = min(s1, (long)a.src_rows);
    d0 -= a.dst_row0;
    for (long r = s0; r < s1; ++r) {
      const long d = d0 + (r - s0);
      if (d < 0 || d >= a.dst_rows) continue;
      if constexpr (MODE == CR_COPY) {
        cr_copy<(int)sizeof(T), VEC>(a.src + r * a.E * (long)sizeof(T), a.dst + d * a.E * (long)sizeof(T), a.E, lane);
        if (a.src_scales) cr_copy<1, false>(a.src_scales + r * SB, a.dst_scales + d * SB, SB, lane);
      } else {
        cr_deq<VEC>(a.src + r * a.E, a.src_scales + r * SB, reinterpret_cast<T*>(a.dst) + d * a.E, a.E, lane);
      }
    }
  }
}

extern "C" int drn_compact_rows(const void* src, const uint8_t* src_scales, const int32_t* src_offsets, const int32_t* positions,
                                const int32_t* dst_offsets, int V, int src_rows, int E, int src_format, int dst_format, int dtype,
                                int dst_videos, int dst_row0, int dst_rows, void* dst, uint8_t* dst_scales, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(src && positions && dst, "drn_compact_rows: null pointer");
  DRN_CHECK_ARG((src_format == DRN_COMPACT_PLAIN || src_format == DRN_COMPACT_MX8) && (dst_format == DRN_COMPACT_PLAIN || dst_format == DRN_COMPACT_MX8),
                "drn_compact_rows: formats %d -> %d: each must be DRN_COMPACT_PLAIN (0) or DRN_COMPACT_MX8 (1)", src_format, dst_format);
  DRN_CHECK_ARG(!(src_format == DRN_COMPACT_PLAIN && dst_format == DRN_COMPACT_MX8),
                "drn_compact_rows: plain -> mxfp8 is not taken here (no second quantiser): move the plain rows into a staging buffer and "
                "run drn_quantize_rows_mx8 on it");
  DRN_CHECK_ARG((src_scales != nullptr) == (src_format == DRN_COMPACT_MX8) && (dst_scales != nullptr) == (dst_format == DRN_COMPACT_MX8),
                "drn_compact_rows: scale bytes must be given exactly beside a block-scaled FP8 table");
  DRN_CHECK_ARG((src_offsets == nullptr) == (dst_offsets == nullptr),
                "drn_compact_rows: src_offsets and dst_offsets must both be given (ragged tables) or neither");
  DRN_CHECK_ARG(V >= 1 && E >= 1 && src_rows >= 1, "drn_compact_rows: bad args (V = %d videos, E = %d columns, src_rows = %d)", V, E, src_rows);
  DRN_CHECK_ARG(src_offsets != nullptr || src_rows == V, "drn_compact_rows: a table of one row a video has src_rows == V, not %d and %d", src_rows, V);
  DRN_CHECK_ARG(dst_videos >= 1 && dst_row0 >= 0 && dst_rows >= 1, "drn_compact_rows: bad destination (dst_videos = %d, dst_row0 = %d, dst_rows = %d)",
                dst_videos, dst_row0, dst_rows);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "drn_compact_rows: bad dtype %d", dtype);
  const bool fp8 = src_format == DRN_COMPACT_MX8;
  DRN_CHECK_ARG(!fp8 || E % MX8_BLOCK == 0, "drn_compact_rows: a block-scaled FP8 table needs E to be a multiple of %d, not E = %d", MX8_BLOCK, E);
  DRN_CHECK_ARG((((uintptr_t)src_offsets | (uintptr_t)positions | (uintptr_t)dst_offsets) & 3) == 0,
                "drn_compact_rows: positions and the offsets must be 4-byte aligned");
  const int es = dtype == DRN_BF16 ? 2 : 4;
  DRN_CHECK_ARG((fp8 || ((uintptr_t)src & (es - 1)) == 0) && (dst_format == DRN_COMPACT_MX8 || ((uintptr_t)dst & (es - 1)) == 0),
                "drn_compact_rows: a plain table must be aligned to its element size (%d bytes)", es);
  const CrArgs a{(const uint8_t*)src, src_scales, src_offsets, positions, dst_offsets, (uint8_t*)dst, dst_scales,
                 V, src_rows, E, dst_videos, dst_row0, dst_rows};
  const int grid = ew_blocks(V, 4, 2048);
  hipStream_t st = (hipStream_t)stream;
  const uintptr_t both = (uintptr_t)src | (uintptr_t)dst;
#define CR_LAUNCH(MODE, T, VEC) compact_rows_kernel<MODE, T, VEC><<<grid, 256, 0, st>>>(a)
  if (!fp8) {                                                  // plain -> plain
    const bool vec = (both & 15) == 0 && ((long)E * es) % 16 == 0;
    if (es == 2) { if (vec) CR_LAUNCH(CR_COPY, uint16_t, true); else CR_LAUNCH(CR_COPY, uint16_t, false); }
    else { if (vec) CR_LAUNCH(CR_COPY, uint32_t, true); else CR_LAUNCH(CR_COPY, uint32_t, false); }
  } else if (dst_format == DRN_COMPACT_MX8) {                  // codes and scale bytes as they are
    if ((both & 15) == 0) CR_LAUNCH(CR_COPY, uint8_t, true); else CR_LAUNCH(CR_COPY, uint8_t, false);
  } else {                                                     // dequantised in registers
    const bool vec = ((uintptr_t)src & 7) == 0 && ((uintptr_t)dst & 15) == 0;
    if (es == 2) { if (vec) CR_LAUNCH(CR_DEQ, bf16_t, true); else CR_LAUNCH(CR_DEQ, bf16_t, false); }
    else { if (vec) CR_LAUNCH(CR_DEQ, float, true); else CR_LAUNCH(CR_DEQ, float, false); }
  }
#undef CR_LAUNCH
  return drn_launch_status("drn_compact_rows");
}
