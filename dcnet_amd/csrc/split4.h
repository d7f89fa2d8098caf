// The f16 two-piece split form gemm3.hip reads, four values at a time: same bytes and strides as the fp32 row, each run of 8
// consecutive elements replaced by [8 f16 high | 8 f16 low] of s*x (s = the tensor's power-of-two scale).  A lane that owns four
// consecutive columns (col % 4 == 0) owns half of such a run: 8 bytes of the high piece, 8 bytes of the low piece.  The layout is
// written here and by presplit_kernel (gemm3.hip: whole runs) only.
#pragma once
#include "common.h"

typedef _Float16 split_f16x4 __attribute__((ext_vector_type(4)));

// the power-of-two scale of an abs-max word (float bits): brings the maximum below 2^14 (= igemm.hip pow2_scale; zero / non-finite -> 1)
__device__ __forceinline__ float split_pow2_scale(unsigned amax_bits) {
  const int be = (int)((amax_bits >> 23) & 0xFF);
  int e = (be == 0 || be == 255) ? 0 : 14 - (be - 126);
  e = e > 100 ? 100 : (e < -100 ? -100 : e);
  return __uint_as_float((unsigned)(e + 127) << 23);
}
constexpr float SPLIT_SCALE_ONE = 8192.f;         // = split_pow2_scale of the constant word 1.0 (unit-norm features, E <= 1)

__device__ __forceinline__ unsigned char* split4_run(const float* row_base, int col) {
  return reinterpret_cast<unsigned char*>(const_cast<float*>(row_base) + (col & ~7)) + (col & 4) * 2;
}
// ts = s * x of columns col .. col + 3 of the row at row_base
__device__ __forceinline__ void split4_store(float* row_base, int col, f32x4 ts) {
  const split_f16x4 h = {(_Float16)ts[0], (_Float16)ts[1], (_Float16)ts[2], (_Float16)ts[3]};
  const split_f16x4 l = {(_Float16)(ts[0] - (float)h[0]), (_Float16)(ts[1] - (float)h[1]), (_Float16)(ts[2] - (float)h[2]),
                         (_Float16)(ts[3] - (float)h[3])};
  unsigned char* run = split4_run(row_base, col);
  *reinterpret_cast<split_f16x4*>(run) = h;
  *reinterpret_cast<split_f16x4*>(run + 16) = l;
}
// h + l of columns col .. col + 3: s * x to 22 bits
__device__ __forceinline__ f32x4 split4_load(const float* row_base, int col) {
  const unsigned char* run = split4_run(row_base, col);
  const split_f16x4 h = *reinterpret_cast<const split_f16x4*>(run), l = *reinterpret_cast<const split_f16x4*>(run + 16);
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (float)h[k] + (float)l[k];
  return v;
}
