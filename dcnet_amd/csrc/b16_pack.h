// bf16 storage: 8 consecutive channels of a pixel as ONE 16-byte access on a bf16 tensor (two on an fp32 one), shared by the streaming
// passes of b16.hip and the bf16 bank passes of video.hip.  The mode has one fp32 -> bf16 conversion, the compiler's (__bf16)x: round to
// nearest even, NaN stays NaN — every pass that writes bf16 goes through st8<__bf16>, so they all round alike.
#pragma once
#include "common.h"

namespace b16io {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
struct F8 { float v[8]; };

__device__ __forceinline__ __bf16 to_bf16(float x) { return (__bf16)x; }      // round to nearest even
// four channels of a lane that owns an f32x4 (8 bytes)
__device__ __forceinline__ bf16x4_t pack4(const f32x4& x) { return bf16x4_t{to_bf16(x[0]), to_bf16(x[1]), to_bf16(x[2]), to_bf16(x[3])}; }

template <typename T> __device__ __forceinline__ F8 ld8(const T* p);
template <> __device__ __forceinline__ F8 ld8<float>(const float* p) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  return F8{{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}};
}
template <> __device__ __forceinline__ F8 ld8<__bf16>(const __bf16* p) {
  const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(p);
  F8 r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = (float)a[k];
  return r;
}
template <typename T> __device__ __forceinline__ void st8(T* p, const F8& x);
template <> __device__ __forceinline__ void st8<float>(float* p, const F8& x) {
  *reinterpret_cast<f32x4*>(p) = f32x4{x.v[0], x.v[1], x.v[2], x.v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{x.v[4], x.v[5], x.v[6], x.v[7]};
}
template <> __device__ __forceinline__ void st8<__bf16>(__bf16* p, const F8& x) {
  bf16x8_t a;
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = to_bf16(x.v[k]);
  *reinterpret_cast<bf16x8_t*>(p) = a;
}

}  // namespace b16io
