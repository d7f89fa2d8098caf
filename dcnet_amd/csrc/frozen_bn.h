// Backward of out = act(scale * conv + shift) with BatchNorm folded from its RUNNING statistics (frozen-BatchNorm fine-tuning and the
// eval-mode backward), one streaming pass shared by bn.hip (fp32 tensors) and b16.hip (bf16 storage).
//
// Per element, from the saved activation a (before a shortcut add) and the incoming gradient dout:
//   dz = dout * (a <= 0 ? slope : 1)          (act_bwd_kernel's rule; DCN_ACT_NONE: dz = dout)
//   dy = dz * scale                           (two products, each rounded once: nothing to contract)
// and, with SUMS, the per-channel partial sums of the affine gradients in channel_partials_kernel's layout [row blocks][2][c],
// 128 rows per partial, to be finished by dcn_bn_bwd_sums:
//   slot 0: sum dz                            (dbeta)
//   slot 1: sum dz * (z - beta) / gamma       (dgamma: (z - beta) / gamma = (conv - running_mean) * rsqrt(running_var + eps))
// z = scale * conv + shift is recovered from a where the activation is invertible: a > 0 ? a : a / slope for LeakyReLU, a itself for
// ReLU (slope 0: the clipped part has dz = 0) and for no activation.  gamma == 0 divides by 1 instead (the channel's normalised input
// cannot be recovered from a; the rule of the torch glue this kernel replaces).  The division by gamma is taken once per partial, on
// the 128-row sum, and a / slope is a * (1 / slope): both within an ulp or two of the per-element divisions, at none of their cost.
//
// Roofline: HBM — fp32 12 B / element (a, dout read, dy written), bf16 storage 6 B; the partials are 1 / 64 of that.
// Grid (rows / 128, c / (16 V)); 256 threads = 16 row lanes x 16 channel groups of V channels, 8 rows per thread: all 16 loads of a
// thread (one 16-byte access each on fp32 and on bf16 with V = 8) are issued before the first is used, 64 KB in flight per workgroup.
// Fixed summation order (8 rows per thread, then the 16 row lanes through LDS): no atomics, bitwise repeatable; the sums are taken
// from the unrounded fp32 dz whatever the type of dy.  The per-channel vectors are read once per thread, as one vector each when
// they are 16-byte aligned (`paligned`) and element by element when not (a channel slice of a wider parameter).
#pragma once
#include "common.h"

namespace frozen_bn {

template <typename T, int V> struct VecOf { typedef T type __attribute__((ext_vector_type(V))); };

template <int V> __device__ __forceinline__ void ld_param(const float* p, bool aligned, float (&o)[V]) {
  if (aligned) {
#pragma unroll
    for (int q = 0; q < V; q += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + q);
      o[q] = t[0]; o[q + 1] = t[1]; o[q + 2] = t[2]; o[q + 3] = t[3];
    }
  } else {
#pragma unroll
    for (int q = 0; q < V; ++q) o[q] = p[q];
  }
}

template <typename TA, typename TD, typename TO, int V, bool SUMS>
__global__ __launch_bounds__(256) void frozen_bn_act_bwd_kernel(const TA* __restrict__ a, const TD* __restrict__ dout, int lddo,
                                                                const float* __restrict__ scale, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, int paligned, int act, float slope,
                                                                int64_t rows, int c, TO* __restrict__ dy, float* __restrict__ stats,
                                                                unsigned* __restrict__ amax) {
  typedef typename VecOf<TA, V>::type va_t;
  typedef typename VecOf<TD, V>::type vd_t;
  typedef typename VecOf<TO, V>::type vo_t;
  constexpr int CW = 16 * V;                              // channels per workgroup
  __shared__ float red[SUMS ? 2 : 1][16][SUMS ? CW : 1];
  __shared__ float red_amax[4];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int ch = blockIdx.y * CW + tx * V;
  const int64_t r0 = (int64_t)blockIdx.x * 128;
  float s[V], ss[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { s[e] = 0.f; ss[e] = 0.f; }
  float vmax = 0.f;
  if (ch < c) {                                           // (c % V == 0: a group lies inside the tensor or outside it)
    float sc[V], b[V];
    ld_param<V>(scale + ch, paligned != 0, sc);
    if (SUMS) ld_param<V>(beta + ch, paligned != 0, b);
    const bool leaky = act == DCN_ACT_LEAKY;
    const float inv_slope = (leaky && slope != 0.f) ? 1.f / slope : 1.f;
    va_t av[8]; vd_t dv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t r = r0 + ty + 16 * k;
      if (r < rows) {
        av[k] = *reinterpret_cast<const va_t*>(a + r * c + ch);      // (the next layer's held weight gradient may still read a)
        dv[k] = __builtin_nontemporal_load(reinterpret_cast<const vd_t*>(dout + r * lddo + ch));      // last read of dout
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t r = r0 + ty + 16 * k;
      if (r >= rows) continue;
      vo_t o;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float x = (float)av[k][e];
        float dz = (float)dv[k][e];
        if (leaky && x <= 0.f) dz *= slope;
        const float t = dz * sc[e];
        o[e] = (TO)t;                                     // (bf16: round to nearest even)
        vmax = fmaxf(vmax, fabsf(t));
        if (SUMS) {
          const float z = (leaky && x <= 0.f) ? x * inv_slope : x;
          s[e] += dz;
          ss[e] += dz * (z - b[e]);
        }
      }
      *reinterpret_cast<vo_t*>(dy + r * c + ch) = o;
    }
  }
  if (SUMS) {
#pragma unroll
    for (int e = 0; e < V; ++e) { red[0][ty][tx * V + e] = s[e]; red[1][ty][tx * V + e] = ss[e]; }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * CW; i += 256) {
      const int which = i / CW, t = i - which * CW, cc = blockIdx.y * CW + t;
      if (cc < c) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc += red[which][k][t];
        if (which == 1) {
          const float g = gamma[cc];
          acc /= (g == 0.f ? 1.f : g);                    // gamma == 0 uses 1 (see the head of this file)
        }
        stats[((size_t)blockIdx.x * 2 + which) * c + cc] = acc;
      }
    }
  }
  if (amax) amax_update_block(amax, vmax, red_amax);      // order-independent maxima, as bn_act_bwd_apply_kernel (amax is grid-uniform)
}

// grid of the pass for [rows][c] with V channels per thread
inline dim3 frozen_grid(int64_t rows, int c, int v) { return dim3(cdiv(rows, 128), cdiv(c, 16 * v)); }

}  // namespace frozen_bn
