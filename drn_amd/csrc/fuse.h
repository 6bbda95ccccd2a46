// What the two fusing translation units share (retrieve_fuse.hip: the fold of weighted scores; retrieve_rrf.hip: the fold of reciprocal
// ranks): an fp32 product and an fp32 sum that are rounded on their own, and the refusals about an optional packed mask.
#pragma once
#include "common.h"

// One fp32 product / one fp32 sum, ROUNDED ON ITS OWN.  hipcc contracts a + b * c into one FMA by default, and __fmul_rn / __fadd_rn are
// plain operators in its headers, which contract all the same once inlined: the two helpers switch contraction off where the operators
// stand.
__device__ __forceinline__ float fu_mul(const float a, const float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float fu_add(const float a, const float b) {
#pragma clang fp contract(off)
  return a + b;
}

// What a fusing entry refuses about an optional packed mask over V videos.
static inline int fu_check_allow(const char* what, const int32_t* allow, int allow_stride, int V) {
  if (allow) {
    DRN_CHECK_ARG(allow_stride == 0 || allow_stride == cdiv(V, 32),
                  "%s: allow_stride = %d is neither 0 (one mask for all sentences) nor ceil(V / 32) = %d (one row per sentence)", what,
                  allow_stride, cdiv(V, 32));
    DRN_CHECK_ARG(((uintptr_t)allow & 3) == 0, "%s: the mask must be 4-byte aligned", what);
  }
  return DRN_OK;
}
