// Pooling the segments of a ragged table into a COARSE one (drn_amd/retrieve.py, Shortlister.pooled): one row a video, or one row per
// `group` rows of a video, from a plain or a block-scaled FP8 source, always into PLAIN rows of the table's dtype.
//   drn_pool_segments   one launch: output row r of video v pools the source rows offsets[v] + j * group .. (at most group of them, cut at
//                       the video's end), j = r - out_offsets[v]; with group == 0 output row v pools every row of video v.  `out` is a
//                       WINDOW of the output, its rows [out_row0, out_row0 + R_out): that is how a staging buffer takes it in chunks.
// drn_amd.retrieve.pool_segments_reference is the definition, bit for bit:
//   PL_MEAN   an fp32 accumulator from +0, the group's rows added in ASCENDING row order, one plain fp32 add a row, one IEEE fp32
//             division by float(count), one rounding to T (round to nearest even);
//   PL_MAX    the first row, then acc = x > acc ? x : acc in ascending row order: the maximum, and of two zeros of either sign the
//             earlier row's (no value is computed, so nothing is rounded).
// A group without rows (a video without rows under group == 0) gives a row of +0.
#include "common.h"
#include "mx8.h"
#include "shortlist.h"
#include "vec.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// ONE WAVEFRONT owns one output row x one column slab: a lane owns PER_LANE contiguous columns (SlStep<T>: 8 bf16 / 4 fp32, 16 bytes
// of a plain row), a slab is the 64 * PER_LANE columns of one pass (512 bf16 / 256 fp32).  Four wavefronts a workgroup, a bounded grid
// and a grid-stride loop over the R_out * slabs items.  The wavefront walks its group's rows in ascending order, PL_AHEAD rows'
// loads issued before the first add and the adds in row order: where a row lands never depends on arrival.  No atomics, no LDS, no
// scratch.
//   PL_VEC    a plain source whose rows all start on a 16-byte boundary (E % PER_LANE == 0; the entry refuses a base that does not):
//             one 16-byte load a row and one 16-byte store a lane;
//   PL_TAIL   a plain source with E % PER_LANE != 0: element by element, zeros past E (sl_frag_tail), and the stores likewise;
//   PL_Q8     codes and scale bytes (E % 32 == 0): PER_LANE code bytes a row in one load (sl_codes_q8) and ONE scale byte a lane -- a
//             lane's columns lie inside one block --, float(code) * 2^(scale - 127), exact in fp32 (sl_frag_q8's statements without
//             the trip through T); dq * scale being exact, a contracted FMA gives the bits of the add.
// The row and slab of an item are made wave-uniform (readfirstlane), so the offsets are read by scalar loads; for a grouped output the
// row's video is found by a bisection of out_offsets, the same in every lane.  EVERY index read from a device table is clamped: the
// bisection stays inside [0, V] whatever the table holds and always ends, the source rows are cut into [0, R), and a store is
// bounded by (window row < R_out, column < E) alone.  Row addresses are 64-bit.
#define PL_MEAN 0
#define PL_MAX 1
#define PL_VEC 0
#define PL_TAIL 1
#define PL_Q8 2
#define PL_AHEAD 4

struct PlArgs {
  const uint8_t* table;        // the plain rows or the codes
  const uint8_t* scales;       // [R][E / 32] or null
  const int* offsets;          // [V + 1]
  const int* out_offsets;      // [V + 1] or null (group == 0)
  uint8_t* out;                // [R_out][E] of T
  int R, V, R_out, row0, E, group;   // out holds the output rows [row0, row0 + R_out)
};

// what a lane holds of one source row between its load and its add
template <typename T, int SRC> struct PlRow;
template <typename T>
struct PlRow<T, PL_VEC> {
  decltype(sl_frag((const T*)nullptr, 0)) f;
  __device__ __forceinline__ void load(const PlArgs& a, const long row, const int c0) { f = sl_frag(reinterpret_cast<const T*>(a.table) + row * a.E, c0); }
  __device__ __forceinline__ float get(const int j) const { return (float)f[j]; }
};
template <typename T>
struct PlRow<T, PL_TAIL> {
  decltype(sl_frag((const T*)nullptr, 0)) f;
  __device__ __forceinline__ void load(const PlArgs& a, const long row, const int c0) {
    f = sl_frag_tail(reinterpret_cast<const T*>(a.table) + row * a.E, c0, a.E);
  }
  __device__ __forceinline__ float get(const int j) const { return (float)f[j]; }
};
template <>
struct PlRow<bf16_t, PL_Q8> {
  u32x2 w;
  unsigned scale;
  __device__ __forceinline__ void load(const PlArgs& a, const long row, const int c0) {
    w = sl_codes_q8(a.table + row * a.E, c0, bf16_t());
    scale = a.scales[row * (a.E / MX8_BLOCK) + (c0 / MX8_BLOCK)];
  }
  __device__ __forceinline__ void values(float (&x)[8]) const {
    const float sc = __uint_as_float(scale << 23);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], true);
      x[4 * h] = lo[0] * sc; x[4 * h + 1] = lo[1] * sc; x[4 * h + 2] = hi[0] * sc; x[4 * h + 3] = hi[1] * sc;
    }
  }
};
template <>
struct PlRow<float, PL_Q8> {
  unsigned w, scale;
  __device__ __forceinline__ void load(const PlArgs& a, const long row, const int c0) {
    w = sl_codes_q8(a.table + row * a.E, c0, float());
    scale = a.scales[row * (a.E / MX8_BLOCK) + (c0 / MX8_BLOCK)];
  }
  __device__ __forceinline__ void values(float (&x)[4]) const {
    const float sc = __uint_as_float(scale << 23);
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    x[0] = lo[0] * sc; x[1] = lo[1] * sc; x[2] = hi[0] * sc; x[3] = hi[1] * sc;
  }
};

// the row's PER_LANE values in fp32 (exact: a bf16 widens, a code times its power of two is a normal fp32 number or zero)
template <typename T, int SRC, int N>
__device__ __forceinline__ void pl_values(const PlRow<T, SRC>& row, float (&x)[N]) {
  if constexpr (SRC == PL_Q8) {
    row.values(x);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = row.get(j);
  }
}

// acc <- acc (+) row; `first` (PL_MAX only): the group's first row starts the maximum
template <int HOW, int N>
__device__ __forceinline__ void pl_step(float (&acc)[N], const float (&x)[N], const bool first) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (HOW == PL_MEAN) acc[j] = acc[j] + x[j];
    else acc[j] = (first || x[j] > acc[j]) ? x[j] : acc[j];
  }
}

template <typename T, int SRC, int HOW>
__global__ __launch_bounds__(256) void pool_segments_kernel(const PlArgs a) {
  constexpr int N = SlStep<T>::PER_LANE, SLAB = 64 * N;
  const int lane = threadIdx.x & 63;
  const int slabs = (a.E + SLAB - 1) / SLAB;
  const long items = (long)a.R_out * slabs, waves = (long)gridDim.x * 4;
  for (long item = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); item < items; item += waves) {   // (wave-uniform)
    const int w = (int)(item / slabs), c0 = (int)(item - (long)w * slabs) * SLAB + lane * N;
    const int r = a.row0 + w;                                  // the output row; row w of the window `out` (the host checked r < 2^31)
    // the group's source rows [s0, s1)
    long s0, s1;
    if (a.out_offsets == nullptr) {
      s0 = a.offsets[r];                                       // (the host checked row0 + R_out <= V)
      s1 = a.offsets[r + 1];
    } else {
      int lo = 0, hi = a.V;                                    // out_offsets[lo] <= r < out_offsets[hi] on a sound table; v = lo
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.out_offsets[mid] <= r) lo = mid; else hi = mid;
      }
      const long j = max((long)r - (long)a.out_offsets[lo], 0L);
      s0 = (long)a.offsets[lo] + j * a.group;
      s1 = min(s0 + a.group, (long)a.offsets[lo + 1]);
    }
    s0 = min(max(s0, 0L), (long)a.R);
    s1 = min(max(s1, s0), (long)a.R);
    const int count = (int)(s1 - s0);
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    if (c0 < a.E) {                                            // (a lane past the row's end in the last slab has nothing to do)
      long s = s0;
      for (; s + PL_AHEAD <= s1; s += PL_AHEAD) {              // PL_AHEAD rows' loads in flight, then their adds in row order
        PlRow<T, SRC> rows[PL_AHEAD];
#pragma unroll
        for (int u = 0; u < PL_AHEAD; ++u) rows[u].load(a, s + u, c0);
#pragma unroll
        for (int u = 0; u < PL_AHEAD; ++u) {
          float x[N];
          pl_values<T, SRC, N>(rows[u], x);
          pl_step<HOW, N>(acc, x, u == 0 && s == s0);
        }
      }
      for (; s < s1; ++s) {
        PlRow<T, SRC> row;
        row.load(a, s, c0);
        float x[N];
        pl_values<T, SRC, N>(row, x);
        pl_step<HOW, N>(acc, x, s == s0);
      }
      if (HOW == PL_MEAN && count > 0) {
        const float n = (float)count;
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = __fdiv_rn(acc[j], n);                // ONE correctly rounded fp32 division
      }
      T* orow = reinterpret_cast<T*>(a.out) + (long)w * a.E;
      if (SRC != PL_TAIL) {
        V16<T>::store(orow + c0, acc);
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
          if (c0 + j < a.E) orow[c0 + j] = (T)acc[j];
      }
    }
  }
}

extern "C" int drn_pool_segments(const void* table, const uint8_t* scales, const int32_t* offsets, const int32_t* out_offsets, int R, int V,
                                 int R_out, int out_row0, int E, int group, int how, int dtype, void* out, void* stream) {
  drn_clear_status();
  const char* what = "drn_pool_segments";
  DRN_CHECK_ARG(table && offsets && out, "%s: null pointer", what);
  DRN_CHECK_ARG(R >= 1 && V >= 1 && E >= 1, "%s: bad args (R = %d rows, V = %d videos, E = %d columns)", what, R, V, E);
  DRN_CHECK_ARG(R_out >= 1, "%s: R_out = %d outside [1, 2^31)", what, R_out);
  DRN_CHECK_ARG(group >= 0, "%s: group = %d below 0 (0: one row a video)", what, group);
  DRN_CHECK_ARG((group == 0) == (out_offsets == nullptr),
                "%s: out_offsets must be given exactly with group >= 1 (group = 0 and NULL: one row a video)", what);
  DRN_CHECK_ARG(out_row0 >= 0, "%s: out_row0 = %d below 0", what, out_row0);
  DRN_CHECK_ARG(group != 0 || (long)out_row0 + R_out <= (long)V,
                "%s: one row a video: the output rows [%d, %d + %d) do not lie inside the V = %d videos", what, out_row0, out_row0, R_out, V);
  DRN_CHECK_ARG(group == 0 || (long)out_row0 + R_out <= (long)R,
                "%s: the output rows [%d, %d + %d) from R = %d source rows: a group holds at least one row", what, out_row0, out_row0, R_out, R);
  DRN_CHECK_ARG(how == DRN_POOL_MEAN || how == DRN_POOL_MAX, "%s: how = %d is neither DRN_POOL_MEAN (0) nor DRN_POOL_MAX (1)", what, how);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "%s: dtype %d (float32 / bfloat16 only)", what, dtype);
  const bool q8 = scales != nullptr;
  if (q8) DRN_CHECK_ARG(E % MX8_BLOCK == 0, "%s: E = %d is not a multiple of the block of %d columns", what, E, MX8_BLOCK);
  DRN_CHECK_ARG(((uintptr_t)table & 15) == 0 && ((uintptr_t)out & 15) == 0, "%s: the table and out must be 16-byte aligned", what);
  DRN_CHECK_ARG((((uintptr_t)offsets | (uintptr_t)out_offsets) & 3) == 0, "%s: the offsets must be 4-byte aligned", what);
  const PlArgs a{(const uint8_t*)table, scales, offsets, out_offsets, (uint8_t*)out, R, V, R_out, out_row0, E, group};
  const int per_lane = dtype == DRN_BF16 ? 8 : 4;
  const long items = (long)R_out * cdiv(E, 64 * per_lane);
  const int grid = ew_blocks(items, 4, 8192);
  hipStream_t st = (hipStream_t)stream;
  const int src = q8 ? PL_Q8 : E % per_lane == 0 ? PL_VEC : PL_TAIL;
#define PL_LAUNCH(T, SRC, HOW) pool_segments_kernel<T, SRC, HOW><<<grid, 256, 0, st>>>(a)
#define PL_HOW(T, SRC) do { if (how == DRN_POOL_MEAN) PL_LAUNCH(T, SRC, PL_MEAN); else PL_LAUNCH(T, SRC, PL_MAX); } while (0)
#define PL_SRC(T) do { if (src == PL_Q8) PL_HOW(T, PL_Q8); else if (src == PL_VEC) PL_HOW(T, PL_VEC); else PL_HOW(T, PL_TAIL); } while (0)
  if (dtype == DRN_BF16) PL_SRC(bf16_t); else PL_SRC(float);
#undef PL_SRC
#undef PL_HOW
#undef PL_LAUNCH
  return drn_launch_status(what);
}
