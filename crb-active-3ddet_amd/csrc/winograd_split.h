// The exact three-way bf16 split of an f32 value that the split-bf16 Winograd kernels share (winograd_conv4.hip: forward / input
// gradient, winograd_wgrad4.hip: weight gradient), and the bf16 vector types of their MFMA operands.
//     x = x1 + x2 + x3,  x1 = x & 0xffff0000, x2 = (x - x1) & 0xffff0000, x3 = x - x1 - x2
// Both subtractions are exact and x3 has at most 8 significant bits: no rounding instruction anywhere. Inf gives NaN pieces
// (inf - inf), pieces below ~2^-110 of a tiny value are flushed.
#pragma once
#include <hip/hip_runtime.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the remainders as f32 values: the bf16 pieces are the high halves of x, r1, r2
__device__ __forceinline__ void split3f(float x, float& r1, float& r2) {
  r1 = x - __uint_as_float(__float_as_uint(x) & 0xffff0000u);
  r2 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
}

// the bf16 bit patterns (high halves) of x1, x2, x3
__device__ __forceinline__ void split3(float x, unsigned& h1, unsigned& h2, unsigned& h3) {
  float r1, r2;
  split3f(x, r1, r2);
  h1 = __float_as_uint(x) >> 16;
  h2 = __float_as_uint(r1) >> 16;
  h3 = __float_as_uint(r2) >> 16;
}
