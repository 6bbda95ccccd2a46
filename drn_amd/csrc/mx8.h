// The quantising arithmetic of the block-scaled FP8 format (drn_amd/index.py mx8_quantize is the definition), shared by the kernels that
// write it: quantize_rows_mx8_kernel (qindex.hip, the index's rows) and gate_quantize_weights_mx8_kernel (qconv.hip, conv0's gated weights).
#pragma once
#include "vec.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

#define MX8_BLOCK 32
#define MX8_EMIN (-110)

// One lane's 16 neighbouring columns of a block of 32 -> the block's exponent e and the lane's 16 code bytes.  The two lanes of a block
// (lane, lane ^ 1) exchange their maxima with one wave shuffle, so BOTH must call this together (inactive lanes pass zeros).
// frexp on the bits: amax = (1 + frac / 2^23) * 2^(E - 127) = m * 2^(E - 126), m <= 0.875 <=> frac <= 0.75 * 2^23.  Zero and the fp32
// subnormals have E = 0 and fall below the clamp, as the definition has them.
__device__ __forceinline__ int mx8_quantize16(const float (&v)[16], u32x4& w) {
  float amax = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) amax = fmaxf(amax, fabsf(v[k]));
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  const unsigned bits = __float_as_uint(amax);
  int e = (int)(bits >> 23) - 126 - 9 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = min(max(e, MX8_EMIN), 127);
  const float inv = __uint_as_float((unsigned)(127 - e) << 23);       // 2^-e (e <= 121 for any fp32 amax: a normal number)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int p = 0;
    p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j] * inv, v[4 * j + 1] * inv, p, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j + 2] * inv, v[4 * j + 3] * inv, p, true);
    w[j] = (unsigned)p;
  }
  return e;
}
