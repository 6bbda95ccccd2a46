// drn_pool_props: proposal features pooled on the device from a resident feature store (include/drn_hip.h, drn_amd/store.py).
//
// out[b][t][:] = max over rows lo..hi of video vids[b]; a bandwidth kernel: the output (B*T*D elements) is written once, each clip's
// slab (S rows) is read from memory once per column block, the runs (8-64 rows per proposal) are read from LDS.
//
// Order comparison without floating-point semantics: a value's bits x map to the key x ^ ((x >> w-1) & max) (sign-magnitude ->
// two's complement: monotone, its own inverse, -0 < +0), keys are compared as signed integers (v_pk_max_i16 for bf16: 8 elements in
// 4 instructions) and mapped back before the store.  The slab is staged as keys, so a run costs one ds_read_b128 + the maxima per row.
#include "common.h"
#include "../../include/drn_hip.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

#define POOL_THREADS 256
#define POOL_LDS_BYTES 65536          // one workgroup's slab at most (no opt-in needed; 30 KB at S = 120 rows x 256-byte blocks)
#define POOL_TARGET_WGS 1024          // workgroups wanted before the column block stops shrinking (4 per CU)

template <typename E> struct Key;
template <> struct Key<int> {
  typedef i32x4 vec_t;
  static __device__ __forceinline__ int one(int x) { return x ^ ((x >> 31) & 0x7fffffff); }
  static __device__ __forceinline__ vec_t vec(vec_t x) { return x ^ ((x >> 31) & 0x7fffffff); }
};
template <> struct Key<short> {
  typedef i16x8 vec_t;
  static __device__ __forceinline__ short one(short x) { return (short)(x ^ ((x >> 15) & 0x7fff)); }
  static __device__ __forceinline__ vec_t vec(vec_t x) { return x ^ ((x >> (short)15) & (short)0x7fff); }
};

struct PoolArgs {
  const void* feats; const long long* seg_off; const int* prop_off; const int* win; const double* pse; const int* vids;
  void* out; double* out_pse;
  int Nv, B, T, D;
};

// what a workgroup knows about its clip: proposals n (0 for a bad index), first proposal p0, first row row0, rows S
struct Clip { int n, p0, S; long long row0; };
static __device__ __forceinline__ Clip pool_clip(const PoolArgs& a, int b) {
  Clip c = {0, 0, 0, 0};
  const int v = a.vids[b];
  if (v < 0 || v >= a.Nv) return c;
  c.row0 = a.seg_off[v];
  const long long S = a.seg_off[v + 1] - c.row0;
  if (S < 1 || c.row0 < 0) return c;
  c.S = (int)(S < 0x7fffffffLL ? S : 0x7fffffffLL);
  c.p0 = a.prop_off[v];
  c.n = min(max(a.prop_off[v + 1] - c.p0, 0), a.T);
  return c;
}

// the (B, T, 2) bounds of clip b: 16 bytes per proposal
static __device__ __forceinline__ void pool_pse(const PoolArgs& a, int b, const Clip& c) {
  const double2* src = (const double2*)a.pse + c.p0;
  double2* dst = (double2*)a.out_pse + (long long)b * a.T;
  for (int t = threadIdx.x; t < a.T; t += blockDim.x) dst[t] = t < c.n ? src[t] : make_double2(0.0, 0.0);
}

// grid: ncb column blocks x B clips; cpr (a power of two <= 64) 16-byte chunks per column block; nchunks chunks per row;
// lds_rows: rows the dynamic LDS allocation holds
template <typename E>
__global__ __launch_bounds__(POOL_THREADS) void pool_props_kernel(PoolArgs a, int cpr, int ncb, int nchunks, int lds_rows) {
  typedef typename Key<E>::vec_t V;
  extern __shared__ uint4 pool_slab_raw[];
  V* slab = (V*)pool_slab_raw;
  const int b = blockIdx.x / ncb, cb = blockIdx.x - b * ncb;
  const Clip c = pool_clip(a, b);
  if (cb == 0) pool_pse(a, b, c);
  const int chunk = threadIdx.x & (cpr - 1), slot = threadIdx.x / cpr, nslots = POOL_THREADS / cpr;
  const int gchunk = cb * cpr + chunk;
  const bool active = gchunk < nchunks;
  const V* src = (const V*)a.feats + c.row0 * nchunks + gchunk;      // this lane's column chunk of the video's first row
  const bool staged = c.n > 0 && c.S <= lds_rows;                   // (uniform over the workgroup)
  if (staged) {
    if (active)
      for (int r = slot; r < c.S; r += nslots) slab[r * cpr + chunk] = Key<E>::vec(src[(long long)r * nchunks]);
    __syncthreads();
  }
  if (!active) return;
  V* dst = (V*)a.out + (long long)b * a.T * nchunks + gchunk;
  for (int t = slot; t < a.T; t += nslots) {
    V acc = (V)0;
    if (t < c.n) {
      const int2 w = ((const int2*)a.win)[c.p0 + t];
      const int lo = min(max(w.x, 0), c.S - 1), hi = min(max(w.y, lo), c.S - 1);
      if (staged) {
        const V* p = slab + chunk;
        acc = p[lo * cpr];
#pragma unroll 4
        for (int r = lo + 1; r <= hi; ++r) acc = __builtin_elementwise_max(acc, p[r * cpr]);
      } else {
        acc = Key<E>::vec(src[(long long)lo * nchunks]);
#pragma unroll 4
        for (int r = lo + 1; r <= hi; ++r) acc = __builtin_elementwise_max(acc, Key<E>::vec(src[(long long)r * nchunks]));
      }
      acc = Key<E>::vec(acc);
    }
    dst[(long long)t * nchunks] = acc;
  }
}

// rows that are not 16-byte multiples (D = 12 in bf16: 24 bytes) or unaligned bases: one element per thread, rows through L2.
// grid: (blocks per clip, B)
template <typename E>
__global__ __launch_bounds__(POOL_THREADS) void pool_props_elem_kernel(PoolArgs a) {
  const int b = blockIdx.y;
  const Clip c = pool_clip(a, b);
  if (blockIdx.x == 0) pool_pse(a, b, c);
  const E* feats = (const E*)a.feats + c.row0 * a.D;
  E* dst = (E*)a.out + (long long)b * a.T * a.D;
  const long long total = (long long)a.T * a.D;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i / a.D), col = (int)(i - (long long)t * a.D);
    E acc = 0;
    if (t < c.n) {
      const int2 w = ((const int2*)a.win)[c.p0 + t];
      const int lo = min(max(w.x, 0), c.S - 1), hi = min(max(w.y, lo), c.S - 1);
      acc = Key<E>::one(feats[(long long)lo * a.D + col]);
      for (int r = lo + 1; r <= hi; ++r) {
        const E k = Key<E>::one(feats[(long long)r * a.D + col]);
        acc = k > acc ? k : acc;
      }
      acc = Key<E>::one(acc);
    }
    dst[i] = acc;
  }
}

// chunks per column block: the widest power of two (<= 64 lanes x 16 bytes) that still leaves POOL_TARGET_WGS workgroups, not below
// 8 chunks (128-byte store segments) unless the row itself is shorter
static int pool_cpr(int B, int nchunks) {
  int cpr = 64;
  while (cpr > 8 && (long)B * cdiv(nchunks, cpr) < POOL_TARGET_WGS) cpr >>= 1;
  while (cpr > 1 && cpr / 2 >= nchunks) cpr >>= 1;
  return cpr;
}
static int pool_elem_bytes(int dtype) { return dtype == DRN_BF16 ? 2 : dtype == DRN_F32 ? 4 : 0; }

extern "C" int64_t drn_pool_props_lds_rows(int B, int D, int dtype) {
  const int es = pool_elem_bytes(dtype);
  if (es == 0 || B < 1 || D < 1 || ((long)D * es) % 16) return 0;
  return POOL_LDS_BYTES / (16 * pool_cpr(B, (int)((long)D * es / 16)));
}

extern "C" int drn_pool_props(const DrnPoolProps* d, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(d, "drn_pool_props: null descriptor");
  const int es = pool_elem_bytes(d->dtype);
  DRN_CHECK_ARG(es, "drn_pool_props: bad dtype %d (0 = float32, 1 = bfloat16)", (int)d->dtype);
  DRN_CHECK_ARG(d->Nv >= 0 && d->B >= 0 && d->T >= 0 && d->D >= 1 && d->max_rows >= 0,
                "drn_pool_props: negative count (Nv %d, B %d, T %d, D %d, max_rows %d)", (int)d->Nv, (int)d->B, (int)d->T, (int)d->D, (int)d->max_rows);
  DRN_CHECK_ARG(d->feats && d->seg_off && d->prop_off && d->win && d->pse && d->vids && d->out && d->out_pse, "drn_pool_props: null pointer");
  DRN_CHECK_ARG(d->B <= 65535, "drn_pool_props: more than 65535 clips");
  DRN_CHECK_ARG(((((uintptr_t)d->pse) | ((uintptr_t)d->out_pse)) & 15) == 0 && (((uintptr_t)d->win) & 7) == 0,
                "drn_pool_props: pse / out_pse must be 16-byte aligned, win 8-byte aligned");
  DRN_CHECK_ARG((((uintptr_t)d->feats) | ((uintptr_t)d->out)) % es == 0, "drn_pool_props: feats / out not aligned to their element");
  if (d->vids_host)
    for (int b = 0; b < d->B; ++b)
      DRN_CHECK_ARG(d->vids_host[b] >= 0 && d->vids_host[b] < d->Nv, "drn_pool_props: clip %d reads video %d of %d", b, (int)d->vids_host[b], (int)d->Nv);
  if (d->counts_host)
    for (int b = 0; b < d->B; ++b)
      DRN_CHECK_ARG(d->counts_host[b] >= 0 && d->counts_host[b] <= d->T, "drn_pool_props: clip %d has %d proposals, T = %d", b, (int)d->counts_host[b], (int)d->T);
  if (d->B == 0 || d->T == 0) return DRN_OK;
  PoolArgs a = {d->feats, (const long long*)d->seg_off, d->prop_off, d->win, d->pse, d->vids, d->out, d->out_pse, d->Nv, d->B, d->T, d->D};
  hipStream_t s = (hipStream_t)stream;
  const long row_bytes = (long)d->D * es;
  if (row_bytes % 16 == 0 && ((((uintptr_t)d->feats) | ((uintptr_t)d->out)) & 15) == 0) {
    const int nchunks = (int)(row_bytes / 16), cpr = pool_cpr(d->B, nchunks), ncb = cdiv(nchunks, cpr);
    DRN_CHECK_ARG((long)ncb * d->B <= 0x7fffffffL, "drn_pool_props: grid too large");
    const int cap = POOL_LDS_BYTES / (16 * cpr);
    const int lds_rows = d->max_rows > 0 && d->max_rows < cap ? d->max_rows : cap;
    const size_t lds = (size_t)lds_rows * cpr * 16;
    if (es == 2) pool_props_kernel<short><<<ncb * d->B, POOL_THREADS, lds, s>>>(a, cpr, ncb, nchunks, lds_rows);
    else pool_props_kernel<int><<<ncb * d->B, POOL_THREADS, lds, s>>>(a, cpr, ncb, nchunks, lds_rows);
  } else {
    const long total = (long)d->T * d->D;
    const dim3 grid((unsigned)(total < 64L * POOL_THREADS ? (total + POOL_THREADS - 1) / POOL_THREADS : 64), (unsigned)d->B);
    if (es == 2) pool_props_elem_kernel<short><<<grid, POOL_THREADS, 0, s>>>(a);
    else pool_props_elem_kernel<int><<<grid, POOL_THREADS, 0, s>>>(a);
  }
  return drn_launch_status("drn_pool_props");
}
