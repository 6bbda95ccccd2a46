// A search index in block-scaled FP8 (drn_amd.SearchIndex(quantize="mxfp8")): the prop_fc columns of a projected row as OCP e4m3fn
// codes with one power-of-two scale per 32 columns (the MX layout), quantised once at build time (drn_quantize_rows_mx8) and
// dequantised inside the one launch that builds conv0's input (drn_gate_gather_packed_q8).
//
// The format, per block of 32 columns (drn_amd/index.py mx8_quantize is the definition, this file its device twin):
//   amax = max |x| in fp32 = m * 2^x with m in [0.5, 1);  e = x - 9 if m <= 0.875 else x - 8 (the smallest e with amax <= 448 * 2^e),
//   e = -110 for a zero block, e clamped to [-110, 127];  scale byte = e + 127 (an e8m0 exponent = the fp32 exponent field of 2^e);
//   code = e4m3fn(x * 2^-e), round to nearest even, the sign kept where the value rounds to zero;  value = float(code) * 2^e.
// 2^e is a power of two and a code has 3 mantissa bits, so the value is exact in fp32 and in bf16.
#include "mx8.h"

// ---------------------------------------------------------------- quantise rows
// x (n, C) -> codes (n, C) u8, scales (n, C / 32) u8.  One lane owns 16 neighbouring columns of one row -- 16-byte loads of x (two
// for bf16, four for fp32), ONE 16-byte store of codes -- and the two lanes of a block (lane, lane ^ 1: C / 16 is even, so they sit
// in the same row and the same wave) exchange their maxima with one wave shuffle; the even lane stores the block's scale byte.
// No LDS, no atomics.  Every address is a function of the work-item number alone: no input value, finite or not, moves an access.
template <typename T>
__global__ __launch_bounds__(256) void quantize_rows_mx8_kernel(const T* __restrict__ x, int ld_x, long total, int gpr /* C / 16 */,
                                                                uint8_t* __restrict__ codes, int ld_codes, uint8_t* __restrict__ scales,
                                                                int ld_scales) {
  constexpr int N = V16<T>::N, NV = 16 / N;
  // (a workgroup-uniform trip count: both lanes of a block reach the shuffle together)
  for (long b = (long)blockIdx.x * 256; b < total; b += (long)gridDim.x * 256) {
    const long i = b + threadIdx.x;
    const bool active = i < total;
    const long row = active ? i / gpr : 0;
    const int g = active ? (int)(i - row * gpr) : 0;
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = 0.f;
    if (active) {
      const T* xp = x + row * ld_x + g * 16;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        float t[N];
        V16<T>::load(xp + j * N, t);
#pragma unroll
        for (int k = 0; k < N; ++k) v[j * N + k] = t[k];
      }
    }
    u32x4 w;
    const int e = mx8_quantize16(v, w);          // (the arithmetic, shared with conv0's gated weights: mx8.h)
    if (!active) continue;
    *(u32x4*)(codes + row * ld_codes + g * 16) = w;
    if ((g & 1) == 0) scales[row * ld_scales + (g >> 1)] = (uint8_t)(e + 127);
  }
}

extern "C" int drn_quantize_rows_mx8(const void* x, int ld_x, int n, int C, uint8_t* codes, int ld_codes, uint8_t* scales, int ld_scales,
                                     int dtype, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(x && codes && scales, "drn_quantize_rows_mx8: null pointer");
  DRN_CHECK_ARG(n > 0 && C > 0, "drn_quantize_rows_mx8: bad args (n %d, C %d)", n, C);
  DRN_CHECK_ARG(C % MX8_BLOCK == 0, "drn_quantize_rows_mx8: C = %d is not a multiple of the block of %d columns", C, MX8_BLOCK);
  DRN_CHECK_ARG(ld_x >= C && ld_codes >= C && ld_scales >= C / MX8_BLOCK, "drn_quantize_rows_mx8: a row stride is shorter than its row");
  DISPATCH_DT(dtype, "drn_quantize_rows_mx8", {
    constexpr int N = V16<T>::N;
    DRN_CHECK_ARG(ld_x % N == 0 && ld_codes % 16 == 0 && ((((uintptr_t)x) | ((uintptr_t)codes)) & 15) == 0,
                  "drn_quantize_rows_mx8: x / codes and their row strides must be 16-byte multiples");
    const long total = (long)n * (C / 16);
    quantize_rows_mx8_kernel<T><<<ew_blocks(total, 256, 8192), 256, 0, (hipStream_t)stream>>>((const T*)x, ld_x, total, C / 16, codes, ld_codes,
                                                                                           scales, ld_scales);
  });
  return drn_launch_status("drn_quantize_rows_mx8");
}

// ---------------------------------------------------------------- query gate over a quantised packed index
// gate_gather_packed_kernel (elementwise.hip) with the gated columns read as codes and scales: the same pair / slot / video / pad-row
// addressing and clamps, one WAVE = U rows of one pair x 64 output vectors, the lookups wave-uniform (scalar loads), the gate vector
// loaded once for the U rows.  A lane still STORES 16 bytes (N = 8 bf16 or 4 fp32 columns) -- this is a store-bandwidth kernel, see
// there -- and reads N code bytes and one scale byte per row for them: N divides 32 and c0 is a multiple of N, so a lane's columns lie
// inside one block.  2^e is the scale byte placed in the fp32 exponent field; code -> fp32 by v_cvt_pk_f32_fp8 (OCP on gfx950).
//   out[p,t,c] = T(float(code[src,c]) * 2^e[src,c/32] * gate[pq[p],c]) for c < C        out[p,t,C+j] = pos[src,j], copied as loaded
template <int N> struct Codes;
template <> struct Codes<8> {
  typedef u32x2 raw_t;
  static __device__ __forceinline__ void cvt(const raw_t& r, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[j], true);
      v[4 * j] = lo[0]; v[4 * j + 1] = lo[1]; v[4 * j + 2] = hi[0]; v[4 * j + 3] = hi[1];
    }
  }
};
template <> struct Codes<4> {
  typedef unsigned raw_t;
  static __device__ __forceinline__ void cvt(const raw_t& r, float (&v)[4]) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r, true);
    v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
  }
};

template <typename T, int U>
__global__ __launch_bounds__(256) void gate_gather_packed_q8_kernel(const uint8_t* __restrict__ codes, int ld_codes,
                                                                    const uint8_t* __restrict__ scales, int ld_scales,
                                                                    const T* __restrict__ pos, int ld_pos, int n_rows, int pad_row,
                                                                    const int* __restrict__ prop_off, int Nv, const float* __restrict__ gate,
                                                                    int ldg, int S, const int* __restrict__ pq, const int* __restrict__ pv,
                                                                    const int* __restrict__ vids, int Vc, T* __restrict__ out, int ld_out,
                                                                    int Q, int L, int C, int P) {
  constexpr int N = V16<T>::N;
  typedef typename Codes<N>::raw_t code_t;
  const int cvec = C / N, nvec = (C + P) / N;
  const int ncc = (nvec + 63) / 64, ngr = (L + U - 1) / U;
  const long total = (long)Q * ngr * ncc;
  const int lane = threadIdx.x & 63;
  const long wave0 = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long w = wave0; w < total; w += (long)gridDim.x * 4) {
    const int cc = (int)(w % ncc);
    const long rg = w / ncc;
    const int p = (int)(rg / ngr), t0 = (int)(rg % ngr) * U;
    const int q = min(max(pq[p], 0), S - 1), slot = pv[p];
    const int vd = (slot >= 0 && slot < Vc) ? vids[slot] : -1;
    int base = 0, cnt = 0;
    if (vd >= 0 && vd < Nv) {
      base = prop_off[vd];
      cnt = prop_off[vd + 1] - base;
    }
    const int v = cc * 64 + lane;
    if (v >= nvec) continue;
    const int c0 = v * N;
    if (v < cvec) {
      code_t r[U];
      unsigned sb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = min(t0 + u, L - 1);
        const long src = min(max(t < cnt ? base + t : pad_row, 0), n_rows - 1);
        r[u] = *(const code_t*)(codes + src * ld_codes + c0);
        sb[u] = scales[src * ld_scales + c0 / MX8_BLOCK];
      }
      float g[N];
      const float* gp = gate + (long)q * ldg + c0;
#pragma unroll
      for (int k = 0; k < N; ++k) g[k] = gp[k];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t >= L) break;
        const float sc = __uint_as_float(sb[u] << 23);
        float x[N];
        Codes<N>::cvt(r[u], x);
#pragma unroll
        for (int k = 0; k < N; ++k) x[k] = (x[k] * sc) * g[k];
        V16<T>::store(out + ((long)p * L + t) * ld_out + c0, x);
      }
    } else {
      typename V16<T>::raw_t r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = min(t0 + u, L - 1);
        const long src = min(max(t < cnt ? base + t : pad_row, 0), n_rows - 1);
        r[u] = V16<T>::ldraw(pos + src * ld_pos + (c0 - C));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t >= L) break;
        *(typename V16<T>::raw_t*)(out + ((long)p * L + t) * ld_out + c0) = r[u];
      }
    }
  }
}

extern "C" int drn_gate_gather_packed_q8(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos,
                                         int ld_pos, int n_rows, int pad_row, const int32_t* prop_off, int Nv, const float* gate, int ldg,
                                         int S, const int32_t* pq, const int32_t* pq_host, const int32_t* pv, const int32_t* vids, int Vc,
                                         void* out, int ld_out, int Q, int L, int C, int P, int dtype, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(codes && scales && prop_off && gate && pq && pv && vids && out && (P == 0 || pos), "drn_gate_gather_packed_q8: null pointer");
  DRN_CHECK_ARG(n_rows > 0 && pad_row >= 0 && pad_row < n_rows && Nv > 0 && S > 0 && Vc > 0 && Q > 0 && L > 0 && C > 0 && P >= 0,
                "drn_gate_gather_packed_q8: bad args (n_rows %d, pad_row %d, Nv %d, S %d, Vc %d, Q %d, L %d, C %d, P %d)", n_rows, pad_row,
                Nv, S, Vc, Q, L, C, P);
  DRN_CHECK_ARG(C % MX8_BLOCK == 0, "drn_gate_gather_packed_q8: C = %d is not a multiple of the block of %d columns", C, MX8_BLOCK);
  DRN_CHECK_ARG((long)Q * L <= 0x7fffffffL, "drn_gate_gather_packed_q8: more than 2^31 rows");
  if (pq_host)
    for (int p = 0; p < Q; ++p)
      DRN_CHECK_ARG(pq_host[p] >= 0 && pq_host[p] < S, "drn_gate_gather_packed_q8: pair %d reads sentence %d of %d", p, (int)pq_host[p], S);
  DISPATCH_DT(dtype, "drn_gate_gather_packed_q8", {
    constexpr int N = V16<T>::N;
    DRN_CHECK_ARG(P % N == 0 && ld_codes % 16 == 0 && ld_out % N == 0 && ldg % 4 == 0 && (P == 0 || ld_pos % N == 0) &&
                      ((((uintptr_t)codes) | ((uintptr_t)out) | ((uintptr_t)gate) | ((uintptr_t)(P ? pos : nullptr))) & 15) == 0,
                  "drn_gate_gather_packed_q8: C / P / ld must be 16-byte multiples");
    DRN_CHECK_ARG(ld_codes >= C && ld_scales >= C / MX8_BLOCK && (P == 0 || ld_pos >= P) && ld_out >= C + P && ldg >= C,
                  "drn_gate_gather_packed_q8: a row stride is shorter than its row");
    constexpr int U = 8;
    const long waves = (long)Q * cdiv(L, U) * cdiv((C + P) / N, 64);
    gate_gather_packed_q8_kernel<T, U><<<ew_blocks(waves * 64, 256, 8192), 256, 0, (hipStream_t)stream>>>(
        codes, ld_codes, scales, ld_scales, (const T*)pos, ld_pos, n_rows, pad_row, prop_off, Nv, gate, ldg, S, pq, pv, vids, Vc, (T*)out,
        ld_out, Q, L, C, P);
  });
  return drn_launch_status("drn_gate_gather_packed_q8");
}
