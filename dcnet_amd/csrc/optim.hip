// Fused multi-tensor optimiser steps — the three optimisers the reference's driver offers (train_DCNet.py:527-534): one pass over
// parameter, gradient and state instead of the element-wise passes of torch's foreach implementations.  HBM-bound:
//   RMSprop (momentum = 0, centered = False)      12 B read + 8 B written per parameter
//   Adam (amsgrad = False, maximize = False)      16 B read + 12 B written
//   SGD with momentum (dampening = 0, no Nesterov) 12 B read + 8 B written
#include "common.h"

namespace {

constexpr int RMS_CHUNK = 32;                 // tensors per launch (pointers travel as kernel arguments: no table upload)
struct RmsChunk {
  float* p[RMS_CHUNK]; const float* g[RMS_CHUNK]; float* v[RMS_CHUNK]; long long n[RMS_CHUNK];
};

// (no FMA contraction: the 16-byte path and the scalar path of a misaligned tensor — a view into a flat gradient buffer — must
//  round alike, or a data-parallel run with bound gradients drifts away from the single-GPU run by an ulp per step)
__device__ __forceinline__ void rms_update(float& p, const float g0, float& v, float lr, float alpha, float eps, float wd) {
#pragma clang fp contract(off)
  const float g = wd != 0.f ? g0 + wd * p : g0;          // grad = grad.add(param, alpha=weight_decay)
  v = v * alpha + (1.f - alpha) * g * g;                 // square_avg.mul_(alpha).addcmul_(grad, grad, value=1-alpha)
  p = p - lr * (g / (sqrtf(v) + eps));                   // param.addcdiv_(grad, square_avg.sqrt().add_(eps), value=-lr)
}

// ---- gradient clipping: the control block ---------------------------------------------------------------------------------------
// Four 32-bit words on the device (include/dcnet_hip.h, dcn_grad_clip_coef): [0] float norm, [1] float coef, [2] int32 apply,
// [3] int32 skips.  The clipped form of an update kernel (CLIP) returns at once when apply is 0 and otherwise takes g0 * coef for
// the gradient — one rounding, contraction off, in front of the weight-decay term: torch's in-place grad.mul_(coef) followed by
// the optimiser.  The plain form (CLIP = false) is the kernel as it was: it never looks at `ctl`.
constexpr int CTL_NORM = 0, CTL_COEF = 1, CTL_APPLY = 2, CTL_SKIPS = 3;
__device__ __forceinline__ float clip_mul(const float g0, const float coef) {
#pragma clang fp contract(off)
  return g0 * coef;
}

template <bool CLIP>
__device__ __forceinline__ void rmsprop_body(const RmsChunk& c, float lr, const float* __restrict__ lr_dev, float alpha, float eps, float wd,
                                             const float* __restrict__ ctl) {
  float coef = 1.f;
  if (CLIP) {
    if (reinterpret_cast<const int*>(ctl)[CTL_APPLY] == 0) return;
    coef = ctl[CTL_COEF];
  }
  if (lr_dev) lr = lr_dev[0];                 // a captured step (hipGraph) reads its learning rate from device memory
  const int t = blockIdx.y;
  float* __restrict__ p = c.p[t]; const float* __restrict__ g = c.g[t]; float* __restrict__ v = c.v[t];
  const long long n = c.n[t];
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)v) & 15) == 0);
  const long long n4 = vec ? n / 4 : 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = pp[e], b = vv[e];
      rms_update(a, CLIP ? clip_mul(gg[e], coef) : gg[e], b, lr, alpha, eps, wd);
      pp[e] = a; vv[e] = b;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    rms_update(p[i], CLIP ? clip_mul(g[i], coef) : g[i], v[i], lr, alpha, eps, wd);
}

__global__ __launch_bounds__(256) void rmsprop_kernel(const RmsChunk c, float lr, const float* __restrict__ lr_dev, float alpha, float eps, float wd) {
  rmsprop_body<false>(c, lr, lr_dev, alpha, eps, wd, nullptr);
}
__global__ __launch_bounds__(256) void rmsprop_clip_kernel(const RmsChunk c, float lr, const float* __restrict__ lr_dev, float alpha, float eps, float wd,
                                                           const float* __restrict__ ctl) {
  rmsprop_body<true>(c, lr, lr_dev, alpha, eps, wd, ctl);
}

// ---- Adam ---------------------------------------------------------------------------------------------------------------------
// Adam's bias corrections depend on the step count t, and a replayed hipGraph must advance t without the host: every tensor has a
// device step word, and adam_prepare_kernel — one launch in front of the update, eager or captured alike — advances it and forms the
// two scalars of the step from it: scal[0] = lr / (1 - beta1^t), scal[1] = 1 / sqrt(1 - beta2^t), in double as torch's Python does.
constexpr int STEP_CHUNK = 128;
struct StepChunk { int* step[STEP_CHUNK]; float* scal[STEP_CHUNK]; };

__device__ __forceinline__ void adam_prepare_body(const StepChunk& c, float lr, const float* __restrict__ lr_dev, double beta1, double beta2) {
  if (threadIdx.x != 0) return;
  if (lr_dev) lr = lr_dev[0];
  const int t = c.step[blockIdx.x][0] + 1;
  c.step[blockIdx.x][0] = t;
  const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
  c.scal[blockIdx.x][0] = (float)((double)lr / bc1);          // step_size = lr / bias_correction1
  c.scal[blockIdx.x][1] = (float)(1.0 / sqrt(bc2));           // torch divides sqrt(v) by the scalar sqrt(bc2): a multiplication by its inverse
}

__global__ __launch_bounds__(64) void adam_prepare_kernel(const StepChunk c, float lr, const float* __restrict__ lr_dev, double beta1, double beta2) {
  adam_prepare_body(c, lr, lr_dev, beta1, beta2);
}
// (a skipped step — apply = 0 — leaves the step words and the scalars alone: the next applied step is step t + 1, not t + 2)
__global__ __launch_bounds__(64) void adam_prepare_clip_kernel(const StepChunk c, float lr, const float* __restrict__ lr_dev, double beta1, double beta2,
                                                               const int* __restrict__ ctl) {
  if (ctl[CTL_APPLY] == 0) return;
  adam_prepare_body(c, lr, lr_dev, beta1, beta2);
}

// AdamW: a third scalar per tensor, scal[2] = 1 - lr * weight_decay, formed in double from the step's learning rate (the device
// scalar under lr_dev) and rounded once — torch forms it in Python and hands param.mul_ the double.  ctl = NULL: the plain form.
__global__ __launch_bounds__(64) void adamw_prepare_kernel(const StepChunk c, float lr, const float* __restrict__ lr_dev, double beta1, double beta2,
                                                           double wd, const int* __restrict__ ctl) {
  if (ctl && ctl[CTL_APPLY] == 0) return;
  adam_prepare_body(c, lr, lr_dev, beta1, beta2);
  if (threadIdx.x != 0) return;
  if (lr_dev) lr = lr_dev[0];
  c.scal[blockIdx.x][2] = (float)(1.0 - (double)lr * wd);
}

struct AdamChunk {
  float* p[RMS_CHUNK]; const float* g[RMS_CHUNK]; float* m[RMS_CHUNK]; float* v[RMS_CHUNK]; const float* s[RMS_CHUNK]; long long n[RMS_CHUNK];
};

// w1 = 1 - beta1, w2 = 1 - beta2 (rounded from double, as torch rounds the Python scalars it hands to lerp_ / addcmul_)
__device__ __forceinline__ void adam_update(float& p, const float g0, float& m, float& v, float step_size, float inv_bc2_sqrt, float w1,
                                            float beta2, float w2, float eps, float wd) {
#pragma clang fp contract(off)
  const float g = wd != 0.f ? g0 + wd * p : g0;          // grad = grad.add(param, alpha=weight_decay)
  const float d = g - m;
  m = w1 < 0.5f ? m + w1 * d : g - d * (1.f - w1);       // exp_avg.lerp_(grad, 1 - beta1)
  v = v * beta2 + w2 * g * g;                            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
  const float denom = sqrtf(v) * inv_bc2_sqrt + eps;     // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p = p - step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// AdamW (decoupled_weight_decay = True), torch 2.10's single-tensor order: param.mul_(1 - lr * weight_decay) first, then Adam's
// update on the unmodified gradient.  `decay` = the factor, rounded once from double (adamw_prepare_kernel; scalar slot [2]); with
// weight_decay = 0 it is exactly 1 and p * 1 keeps p's bits, which is torch skipping the multiplication.
__device__ __forceinline__ void adamw_update(float& p, const float g, float& m, float& v, float step_size, float inv_bc2_sqrt, float decay,
                                             float w1, float beta2, float w2, float eps) {
#pragma clang fp contract(off)
  const float q = p * decay;                             // param.mul_(1 - lr * weight_decay)
  const float d = g - m;
  m = w1 < 0.5f ? m + w1 * d : g - d * (1.f - w1);       // exp_avg.lerp_(grad, 1 - beta1)
  v = v * beta2 + w2 * g * g;                            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
  const float denom = sqrtf(v) * inv_bc2_sqrt + eps;     // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p = q - step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// DECOUPLED = false is Adam as it was (two scalars per tensor, `wd` added to the gradient); true is AdamW (three scalars, `wd` unused)
template <bool CLIP, bool DECOUPLED = false>
__device__ __forceinline__ void adam_body(const AdamChunk& c, float w1, float beta2, float w2, float eps, float wd, const float* __restrict__ ctl) {
  float coef = 1.f;
  if (CLIP) {
    if (reinterpret_cast<const int*>(ctl)[CTL_APPLY] == 0) return;
    coef = ctl[CTL_COEF];
  }
  const int t = blockIdx.y;
  float* __restrict__ p = c.p[t]; const float* __restrict__ g = c.g[t]; float* __restrict__ m = c.m[t]; float* __restrict__ v = c.v[t];
  const float step_size = c.s[t][0], inv_bc2_sqrt = c.s[t][1];          // (adam_prepare_kernel wrote them in the launch before this one)
  const float decay = DECOUPLED ? c.s[t][2] : 1.f;
  const long long n = c.n[t];
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  const long long n4 = vec ? n / 4 : 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i], mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = pp[e], b = mm[e], d = vv[e];
      const float ge = CLIP ? clip_mul(gg[e], coef) : gg[e];
      if (DECOUPLED) adamw_update(a, ge, b, d, step_size, inv_bc2_sqrt, decay, w1, beta2, w2, eps);
      else adam_update(a, ge, b, d, step_size, inv_bc2_sqrt, w1, beta2, w2, eps, wd);
      pp[e] = a; mm[e] = b; vv[e] = d;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(m)[i] = mm; reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float ge = CLIP ? clip_mul(g[i], coef) : g[i];
    if (DECOUPLED) adamw_update(p[i], ge, m[i], v[i], step_size, inv_bc2_sqrt, decay, w1, beta2, w2, eps);
    else adam_update(p[i], ge, m[i], v[i], step_size, inv_bc2_sqrt, w1, beta2, w2, eps, wd);
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(const AdamChunk c, float w1, float beta2, float w2, float eps) {
  adam_body<false, true>(c, w1, beta2, w2, eps, 0.f, nullptr);
}
__global__ __launch_bounds__(256) void adamw_clip_kernel(const AdamChunk c, float w1, float beta2, float w2, float eps, const float* __restrict__ ctl) {
  adam_body<true, true>(c, w1, beta2, w2, eps, 0.f, ctl);
}

__global__ __launch_bounds__(256) void adam_kernel(const AdamChunk c, float w1, float beta2, float w2, float eps, float wd) {
  adam_body<false>(c, w1, beta2, w2, eps, wd, nullptr);
}
__global__ __launch_bounds__(256) void adam_clip_kernel(const AdamChunk c, float w1, float beta2, float w2, float eps, float wd,
                                                        const float* __restrict__ ctl) {
  adam_body<true>(c, w1, beta2, w2, eps, wd, ctl);
}

// ---- SGD with momentum --------------------------------------------------------------------------------------------------------
// (same shape as RmsChunk: parameter, gradient, one state tensor)
__device__ __forceinline__ void sgd_update(float& p, const float g0, float& buf, float lr, float mu, float wd) {
#pragma clang fp contract(off)
  const float g = wd != 0.f ? g0 + wd * p : g0;          // grad = grad.add(param, alpha=weight_decay)
  buf = buf * mu + g;                                    // buf.mul_(momentum).add_(grad)   (first step: buf = grad, which a zero buffer gives)
  p = p - lr * buf;                                      // param.add_(buf, alpha=-lr)
}

template <bool CLIP>
__device__ __forceinline__ void sgd_body(const RmsChunk& c, float lr, const float* __restrict__ lr_dev, float mu, float wd, const float* __restrict__ ctl) {
  float coef = 1.f;
  if (CLIP) {
    if (reinterpret_cast<const int*>(ctl)[CTL_APPLY] == 0) return;
    coef = ctl[CTL_COEF];
  }
  if (lr_dev) lr = lr_dev[0];
  const int t = blockIdx.y;
  float* __restrict__ p = c.p[t]; const float* __restrict__ g = c.g[t]; float* __restrict__ b = c.v[t];
  const long long n = c.n[t];
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0);
  const long long n4 = vec ? n / 4 : 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i], bb = reinterpret_cast<f32x4*>(b)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = pp[e], d = bb[e];
      sgd_update(a, CLIP ? clip_mul(gg[e], coef) : gg[e], d, lr, mu, wd);
      pp[e] = a; bb[e] = d;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(b)[i] = bb;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    sgd_update(p[i], CLIP ? clip_mul(g[i], coef) : g[i], b[i], lr, mu, wd);
}

__global__ __launch_bounds__(256) void sgd_kernel(const RmsChunk c, float lr, const float* __restrict__ lr_dev, float mu, float wd) {
  sgd_body<false>(c, lr, lr_dev, mu, wd, nullptr);
}
__global__ __launch_bounds__(256) void sgd_clip_kernel(const RmsChunk c, float lr, const float* __restrict__ lr_dev, float mu, float wd,
                                                       const float* __restrict__ ctl) {
  sgd_body<true>(c, lr, lr_dev, mu, wd, ctl);
}

// ---- exponential moving average of the weights, and the in-place swap ------------------------------------------------------------
// shadow <- lerp(shadow, src, w) over every shadowed tensor: 8 B read + 4 B written per value.  The weight w = 1 - d_t depends on the
// count t of updates applied, which — like Adam's — lives on the device so that a replayed step advances it: ema_prepare_kernel (one
// thread, in front of the update) advances the step word and forms w in double; a skipped step (apply = 0) leaves both words alone.
__global__ __launch_bounds__(64) void ema_prepare_kernel(int* __restrict__ step, float* __restrict__ w, double decay, double tau,
                                                         const int* __restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (ctl && ctl[CTL_APPLY] == 0) return;
  const int t = step[0] + 1;
  step[0] = t;
  const double d = tau > 0.0 ? decay * (1.0 - exp(-(double)t / tau)) : decay;
  w[0] = (float)(1.0 - d);
}

struct EmaChunk { float* s[RMS_CHUNK]; const float* x[RMS_CHUNK]; long long n[RMS_CHUNK]; };
struct SwapChunk { float* a[RMS_CHUNK]; float* b[RMS_CHUNK]; long long n[RMS_CHUNK]; };

// torch's fp32 lerp (the form adam_update uses for exp_avg).  x == s gives d = 0 and keeps s bit for bit in either form, but for
// s = -0.0 under w < 0.5 (-0 + 0 is +0): the select keeps that one too, so a tensor nobody trains never changes a bit.
__device__ __forceinline__ float ema_lerp(const float s, const float x, const float w) {
#pragma clang fp contract(off)
  const float d = x - s;
  const float r = w < 0.5f ? s + w * d : x - d * (1.f - w);
  return d == 0.f ? s : r;
}
__device__ __forceinline__ f32x4 ema_lerp4(f32x4 s, const f32x4 x, const float w) {
#pragma unroll
  for (int e = 0; e < 4; ++e) s[e] = ema_lerp(s[e], x[e], w);
  return s;
}

__global__ __launch_bounds__(256) void ema_update_kernel(const EmaChunk c, const float* __restrict__ wp, const int* __restrict__ ctl) {
  if (ctl && ctl[CTL_APPLY] == 0) return;
  const float w = wp[0];                      // (ema_prepare_kernel wrote it in the launch before this one)
  const int t = blockIdx.y;
  float* __restrict__ s = c.s[t]; const float* __restrict__ x = c.x[t];
  const long long n = c.n[t];
  const bool vec = ((((uintptr_t)s | (uintptr_t)x) & 15) == 0);
  const long long n4 = vec ? n / 4 : 0;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  // two trips at once: four 16-byte loads in flight per thread (the pass has two streams where the optimiser updates have three or four)
  for (; i + stride < n4; i += 2 * stride) {
    const f32x4 s0 = reinterpret_cast<f32x4*>(s)[i], s1 = reinterpret_cast<f32x4*>(s)[i + stride];
    const f32x4 x0 = reinterpret_cast<const f32x4*>(x)[i], x1 = reinterpret_cast<const f32x4*>(x)[i + stride];
    reinterpret_cast<f32x4*>(s)[i] = ema_lerp4(s0, x0, w);
    reinterpret_cast<f32x4*>(s)[i + stride] = ema_lerp4(s1, x1, w);
  }
  for (; i < n4; i += stride)
    reinterpret_cast<f32x4*>(s)[i] = ema_lerp4(reinterpret_cast<f32x4*>(s)[i], reinterpret_cast<const f32x4*>(x)[i], w);
  for (i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
    s[i] = ema_lerp(s[i], x[i], w);
}

// a <-> b: 8 B read + 8 B written per value; every value is moved by exactly one thread
__global__ __launch_bounds__(256) void tensor_swap_kernel(const SwapChunk c) {
  const int t = blockIdx.y;
  float* __restrict__ a = c.a[t]; float* __restrict__ b = c.b[t];
  const long long n = c.n[t];
  const bool vec = ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
  const long long n4 = vec ? n / 4 : 0;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const f32x4 a0 = reinterpret_cast<f32x4*>(a)[i], a1 = reinterpret_cast<f32x4*>(a)[i + stride];
    const f32x4 b0 = reinterpret_cast<f32x4*>(b)[i], b1 = reinterpret_cast<f32x4*>(b)[i + stride];
    reinterpret_cast<f32x4*>(a)[i] = b0; reinterpret_cast<f32x4*>(a)[i + stride] = b1;
    reinterpret_cast<f32x4*>(b)[i] = a0; reinterpret_cast<f32x4*>(b)[i + stride] = a1;
  }
  for (; i < n4; i += stride) {
    const f32x4 a0 = reinterpret_cast<f32x4*>(a)[i], b0 = reinterpret_cast<f32x4*>(b)[i];
    reinterpret_cast<f32x4*>(a)[i] = b0; reinterpret_cast<f32x4*>(b)[i] = a0;
  }
  for (i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float a0 = a[i], b0 = b[i];
    a[i] = b0; b[i] = a0;
  }
}

// blocks along x for a chunk whose longest tensor has `biggest` values (grid-stride beyond 128)
inline unsigned blocks_for(long long biggest) {
  const long long bx = (biggest / 4 + 255) / 256;
  return (unsigned)(bx < 1 ? 1 : (bx > 128 ? 128 : bx));
}

// ---- global gradient norm ---------------------------------------------------------------------------------------------------------
// One more read of the gradients: every block sums the squares of its share of one tensor in double (the product of two floats is
// exact in double, so contraction cannot change a bit) and writes ONE double into its own slot — slot (chunk, tensor in chunk,
// blockIdx.x), every launched block writes, 0.0 when it had no work.  grad_clip_coef_kernel adds the slots in a fixed order.  No
// atomics, no arrival counters: the norm is the same bits in every run, eager or replayed.  A thread takes the same four
// consecutive values per trip whether the pointer is 16-byte aligned (one 16-byte load) or not (four 4-byte loads), so a view
// into a flat gradient buffer gives the same bits as an aligned tensor.
struct NormChunk { const float* g[RMS_CHUNK]; long long n[RMS_CHUNK]; };
struct ScaleChunk { float* g[RMS_CHUNK]; long long n[RMS_CHUNK]; };

// sum over the WAVES x 64 threads of a block, in a fixed order; `red` = WAVES doubles of shared memory.  Every thread must call.
template <int WAVES>
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) s += red[w];
  return s;
}

// four consecutive gradient values: one 16-byte load where the tensor is 16-byte aligned, four 4-byte loads otherwise
__device__ __forceinline__ f32x4 load4(const float* __restrict__ g, long long i, bool vec) {
  if (vec) return reinterpret_cast<const f32x4*>(g)[i];
  f32x4 r;
  r[0] = g[4 * i]; r[1] = g[4 * i + 1]; r[2] = g[4 * i + 2]; r[3] = g[4 * i + 3];
  return r;
}
__device__ __forceinline__ double add_squares(double acc, const f32x4 gg) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { const double x = (double)gg[e]; acc += x * x; }
  return acc;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const NormChunk c, double* __restrict__ partials) {
  __shared__ double red[4];
  const int t = blockIdx.y;
  const float* __restrict__ g = c.g[t];
  const long long n = c.n[t], n4 = n / 4;
  const bool vec = (((uintptr_t)g) & 15) == 0;
  const long long stride = (long long)gridDim.x * 256;
  double acc = 0.0;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  // four loads in flight per thread (one load per trip leaves HBM half idle); the squares are added in the order of the plain loop
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const f32x4 a = load4(g, i, vec), b = load4(g, i + stride, vec), d = load4(g, i + 2 * stride, vec), e = load4(g, i + 3 * stride, vec);
    acc = add_squares(add_squares(add_squares(add_squares(acc, a), b), d), e);
  }
  for (; i < n4; i += stride) acc = add_squares(acc, load4(g, i, vec));
  for (i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const double x = (double)g[i]; acc += x * x;
  }
  const double s = block_sum_f64<4>(acc, red);
  if (threadIdx.x == 0) partials[(long long)t * gridDim.x + blockIdx.x] = s;
}

// clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1 — in fp32, each operation rounded once
__device__ __forceinline__ float clip_coef(const float norm, const float max_norm) {
#pragma clang fp contract(off)
  const float coef = max_norm / (norm + 1e-6f);
  return coef > 1.f ? 1.f : coef;                        // torch.clamp(clip_coef, max=1.0): a NaN stays a NaN
}

// one workgroup of 1024: thread i adds slots i, i + 1024, ... — four running sums (trip k into sum k mod 4: four loads in flight, the
// sum is latency-bound), folded in a fixed order — then the block sum; thread 0 writes the control block
__global__ __launch_bounds__(1024) void grad_clip_coef_kernel(const double* __restrict__ partials, long long slots, float max_norm, int skip_nonfinite,
                                                              float* __restrict__ ctl) {
  __shared__ double red[16];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  long long i = threadIdx.x;
  for (; i + 3 * 1024 < slots; i += 4 * 1024) {
    const double p0 = partials[i], p1 = partials[i + 1024], p2 = partials[i + 2 * 1024], p3 = partials[i + 3 * 1024];
    a0 += p0; a1 += p1; a2 += p2; a3 += p3;
  }
  if (i < slots) a0 += partials[i];
  if (i + 1024 < slots) a1 += partials[i + 1024];
  if (i + 2 * 1024 < slots) a2 += partials[i + 2 * 1024];
  const double s = block_sum_f64<16>((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(s);
  const int apply = (skip_nonfinite && !__builtin_isfinite(s)) ? 0 : 1;
  ctl[CTL_NORM] = norm;
  ctl[CTL_COEF] = clip_coef(norm, max_norm);
  int* w = reinterpret_cast<int*>(ctl);
  w[CTL_APPLY] = apply;
  if (!apply) w[CTL_SKIPS] = w[CTL_SKIPS] + 1;
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const ScaleChunk c, const float* __restrict__ ctl) {
  const float coef = ctl[CTL_COEF];
  const int t = blockIdx.y;
  float* __restrict__ g = c.g[t];
  const long long n = c.n[t];
  const long long n4 = ((((uintptr_t)g) & 15) == 0) ? n / 4 : 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 gg = reinterpret_cast<f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) gg[e] = clip_mul(gg[e], coef);
    reinterpret_cast<f32x4*>(g)[i] = gg;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    g[i] = clip_mul(g[i], coef);
}

// slots of the partials buffer for `count` tensors: per chunk of 32, blocks_for(its longest tensor) x tensors in the chunk
inline long long sumsq_slots(const int64_t* numel, int count) {
  long long total = 0;
  for (int base = 0; base < count; base += RMS_CHUNK) {
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i)
      if (numel[base + i] > biggest) biggest = numel[base + i];
    total += (long long)blocks_for(biggest) * m;
  }
  return total;
}

}  // namespace

extern "C" int64_t dcn_grad_sumsq_slots(const int64_t* numel, int count) {
  if (!numel || count <= 0) { dcn_set_error("grad_sumsq_slots: bad argument"); return -1; }
  for (int i = 0; i < count; ++i)
    if (numel[i] < 0) { dcn_set_error("grad_sumsq_slots: negative element count of tensor %d", i); return -1; }
  return sumsq_slots(numel, count);
}

extern "C" int dcn_grad_sumsq(const float* const* grads, const int64_t* numel, int count, double* partials, int64_t slots, void* stream) {
  DCN_CHECK_ARG(grads && numel && partials && count > 0, "grad_sumsq: bad argument");
  for (int i = 0; i < count; ++i)
    DCN_CHECK_ARG(grads[i] && numel[i] >= 0, "grad_sumsq: null tensor %d", i);
  DCN_CHECK_ARG(slots == sumsq_slots(numel, count), "grad_sumsq: the partials buffer has %lld slots, these tensors need %lld (dcn_grad_sumsq_slots)",
                (long long)slots, sumsq_slots(numel, count));
  long long at = 0;
  for (int base = 0; base < count; base += RMS_CHUNK) {
    NormChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      c.g[i] = grads[base + i]; c.n[i] = numel[base + i];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    const unsigned bx = blocks_for(biggest);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(bx, m), dim3(256), 0, (hipStream_t)stream, c, partials + at);
    DCN_CHECK_LAUNCH("grad_sumsq");
    at += (long long)bx * m;
  }
  return DCN_OK;
}

extern "C" int dcn_grad_clip_coef(const double* partials, int64_t slots, float max_norm, int skip_nonfinite, void* ctrl, void* stream) {
  DCN_CHECK_ARG(partials && ctrl && slots > 0, "grad_clip_coef: bad argument");
  DCN_CHECK_ARG(max_norm > 0.f, "grad_clip_coef: max_norm %g is not a positive number", (double)max_norm);
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, (long long)slots, max_norm, skip_nonfinite,
                     (float*)ctrl);
  DCN_CHECK_LAUNCH("grad_clip_coef");
  return DCN_OK;
}

extern "C" int dcn_grad_scale(float* const* grads, const int64_t* numel, int count, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(grads && numel && ctrl && count > 0, "grad_scale: bad argument");
  for (int i = 0; i < count; ++i)
    DCN_CHECK_ARG(grads[i] && numel[i] >= 0, "grad_scale: null tensor %d", i);
  for (int base = 0; base < count; base += RMS_CHUNK) {
    ScaleChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      c.g[i] = grads[base + i]; c.n[i] = numel[base + i];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    hipLaunchKernelGGL(grad_scale_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, (const float*)ctrl);
    DCN_CHECK_LAUNCH("grad_scale");
  }
  return DCN_OK;
}

// The update entry points come in two forms over one body each: the plain one launches the kernels it always launched, the
// `_clipped` one (ctl = the control block dcn_grad_clip_coef wrote, non-NULL) their clipped forms.
static int rmsprop_step(const char* who, float* const* params, const float* const* grads, float* const* square_avgs, const int64_t* numel,
                        int count, float lr, const float* lr_dev, float alpha, float eps, float weight_decay, const float* ctl, void* stream) {
  DCN_CHECK_ARG(params && grads && square_avgs && numel && count > 0, "%s: bad argument", who);
  for (int base = 0; base < count; base += RMS_CHUNK) {
    RmsChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      DCN_CHECK_ARG(params[base + i] && grads[base + i] && square_avgs[base + i] && numel[base + i] >= 0, "%s: null tensor %d", who, base + i);
      c.p[i] = params[base + i]; c.g[i] = grads[base + i]; c.v[i] = square_avgs[base + i]; c.n[i] = numel[base + i];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    if (ctl)
      hipLaunchKernelGGL(rmsprop_clip_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, lr, lr_dev, alpha, eps, weight_decay, ctl);
    else
      hipLaunchKernelGGL(rmsprop_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, lr, lr_dev, alpha, eps, weight_decay);
    DCN_CHECK_LAUNCH(who);
  }
  return DCN_OK;
}

extern "C" int dcn_rmsprop_step(float* const* params, const float* const* grads, float* const* square_avgs, const int64_t* numel,
                                int count, float lr, const float* lr_dev, float alpha, float eps, float weight_decay, void* stream) {
  return rmsprop_step("rmsprop_step", params, grads, square_avgs, numel, count, lr, lr_dev, alpha, eps, weight_decay, nullptr, stream);
}

extern "C" int dcn_rmsprop_step_clipped(float* const* params, const float* const* grads, float* const* square_avgs, const int64_t* numel,
                                        int count, float lr, const float* lr_dev, float alpha, float eps, float weight_decay, const void* ctrl,
                                        void* stream) {
  DCN_CHECK_ARG(ctrl, "rmsprop_step_clipped: no control block");
  return rmsprop_step("rmsprop_step_clipped", params, grads, square_avgs, numel, count, lr, lr_dev, alpha, eps, weight_decay, (const float*)ctrl, stream);
}

static int adam_prepare(const char* who, int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                        const int* ctl, void* stream) {
  DCN_CHECK_ARG(steps && scal && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
  for (int base = 0; base < count; base += STEP_CHUNK) {
    StepChunk c{};
    const int m = count - base < STEP_CHUNK ? count - base : STEP_CHUNK;
    for (int i = 0; i < m; ++i) {
      DCN_CHECK_ARG(steps[base + i] && scal[base + i], "%s: null tensor %d", who, base + i);
      c.step[i] = steps[base + i]; c.scal[i] = scal[base + i];
    }
    if (ctl)
      hipLaunchKernelGGL(adam_prepare_clip_kernel, dim3(m), dim3(64), 0, (hipStream_t)stream, c, lr, lr_dev, beta1, beta2, ctl);
    else
      hipLaunchKernelGGL(adam_prepare_kernel, dim3(m), dim3(64), 0, (hipStream_t)stream, c, lr, lr_dev, beta1, beta2);
    DCN_CHECK_LAUNCH(who);
  }
  return DCN_OK;
}

extern "C" int dcn_adam_prepare(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                void* stream) {
  return adam_prepare("adam_prepare", steps, scal, count, lr, lr_dev, beta1, beta2, nullptr, stream);
}

extern "C" int dcn_adam_prepare_clipped(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                        const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adam_prepare_clipped: no control block");
  return adam_prepare("adam_prepare_clipped", steps, scal, count, lr, lr_dev, beta1, beta2, (const int*)ctrl, stream);
}

static int adam_step(const char* who, float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                     const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps, float weight_decay,
                     const float* ctl, void* stream) {
  DCN_CHECK_ARG(params && grads && exp_avgs && exp_avg_sqs && scal && numel && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
  DCN_CHECK_ARG(eps >= 0.f && weight_decay >= 0.f, "%s: negative eps or weight_decay", who);
  for (int base = 0; base < count; base += RMS_CHUNK) {
    AdamChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      const int k = base + i;
      DCN_CHECK_ARG(params[k] && grads[k] && exp_avgs[k] && exp_avg_sqs[k] && scal[k] && numel[k] >= 0, "%s: null tensor %d", who, k);
      c.p[i] = params[k]; c.g[i] = grads[k]; c.m[i] = exp_avgs[k]; c.v[i] = exp_avg_sqs[k]; c.s[i] = scal[k]; c.n[i] = numel[k];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    if (ctl)
      hipLaunchKernelGGL(adam_clip_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, (float)(1.0 - beta1), (float)beta2,
                         (float)(1.0 - beta2), eps, weight_decay, ctl);
    else
      hipLaunchKernelGGL(adam_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, (float)(1.0 - beta1), (float)beta2,
                         (float)(1.0 - beta2), eps, weight_decay);
    DCN_CHECK_LAUNCH(who);
  }
  return DCN_OK;
}

extern "C" int dcn_adam_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                             const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                             float weight_decay, void* stream) {
  return adam_step("adam_step", params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, weight_decay, nullptr, stream);
}

extern "C" int dcn_adam_step_clipped(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                     const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                                     float weight_decay, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adam_step_clipped: no control block");
  return adam_step("adam_step_clipped", params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, weight_decay, (const float*)ctrl,
                   stream);
}

static int sgd_step(const char* who, float* const* params, const float* const* grads, float* const* momentum_bufs, const int64_t* numel, int count,
                    float lr, const float* lr_dev, float momentum, float weight_decay, const float* ctl, void* stream) {
  DCN_CHECK_ARG(params && grads && momentum_bufs && numel && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(momentum >= 0.f && weight_decay >= 0.f, "%s: negative momentum or weight_decay", who);
  for (int base = 0; base < count; base += RMS_CHUNK) {
    RmsChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      const int k = base + i;
      DCN_CHECK_ARG(params[k] && grads[k] && momentum_bufs[k] && numel[k] >= 0, "%s: null tensor %d", who, k);
      c.p[i] = params[k]; c.g[i] = grads[k]; c.v[i] = momentum_bufs[k]; c.n[i] = numel[k];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    if (ctl)
      hipLaunchKernelGGL(sgd_clip_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, lr, lr_dev, momentum, weight_decay, ctl);
    else
      hipLaunchKernelGGL(sgd_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, lr, lr_dev, momentum, weight_decay);
    DCN_CHECK_LAUNCH(who);
  }
  return DCN_OK;
}

extern "C" int dcn_sgd_step(float* const* params, const float* const* grads, float* const* momentum_bufs, const int64_t* numel, int count,
                            float lr, const float* lr_dev, float momentum, float weight_decay, void* stream) {
  return sgd_step("sgd_step", params, grads, momentum_bufs, numel, count, lr, lr_dev, momentum, weight_decay, nullptr, stream);
}

extern "C" int dcn_sgd_step_clipped(float* const* params, const float* const* grads, float* const* momentum_bufs, const int64_t* numel, int count,
                                    float lr, const float* lr_dev, float momentum, float weight_decay, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "sgd_step_clipped: no control block");
  return sgd_step("sgd_step_clipped", params, grads, momentum_bufs, numel, count, lr, lr_dev, momentum, weight_decay, (const float*)ctrl, stream);
}

// AdamW (decoupled weight decay): its own entry points, three scalars per tensor — Adam's keep theirs and their two.
static int adamw_prepare(const char* who, int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                         double weight_decay, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(steps && scal && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
  DCN_CHECK_ARG(weight_decay >= 0.0, "%s: negative weight_decay", who);
  for (int base = 0; base < count; base += STEP_CHUNK) {
    StepChunk c{};
    const int m = count - base < STEP_CHUNK ? count - base : STEP_CHUNK;
    for (int i = 0; i < m; ++i) {
      DCN_CHECK_ARG(steps[base + i] && scal[base + i], "%s: null tensor %d", who, base + i);
      c.step[i] = steps[base + i]; c.scal[i] = scal[base + i];
    }
    hipLaunchKernelGGL(adamw_prepare_kernel, dim3(m), dim3(64), 0, (hipStream_t)stream, c, lr, lr_dev, beta1, beta2, weight_decay, (const int*)ctrl);
    DCN_CHECK_LAUNCH(who);
  }
  return DCN_OK;
}

extern "C" int dcn_adamw_prepare(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                 double weight_decay, void* stream) {
  return adamw_prepare("adamw_prepare", steps, scal, count, lr, lr_dev, beta1, beta2, weight_decay, nullptr, stream);
}

extern "C" int dcn_adamw_prepare_clipped(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                         double weight_decay, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adamw_prepare_clipped: no control block");
  return adamw_prepare("adamw_prepare_clipped", steps, scal, count, lr, lr_dev, beta1, beta2, weight_decay, ctrl, stream);
}

static int adamw_step(const char* who, float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                      const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps, const void* ctrl,
                      void* stream) {
  DCN_CHECK_ARG(params && grads && exp_avgs && exp_avg_sqs && scal && numel && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
  DCN_CHECK_ARG(eps >= 0.f, "%s: negative eps", who);
  for (int base = 0; base < count; base += RMS_CHUNK) {
    AdamChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      const int k = base + i;
      DCN_CHECK_ARG(params[k] && grads[k] && exp_avgs[k] && exp_avg_sqs[k] && scal[k] && numel[k] >= 0, "%s: null tensor %d", who, k);
      c.p[i] = params[k]; c.g[i] = grads[k]; c.m[i] = exp_avgs[k]; c.v[i] = exp_avg_sqs[k]; c.s[i] = scal[k]; c.n[i] = numel[k];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    if (ctrl)
      hipLaunchKernelGGL(adamw_clip_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, (float)(1.0 - beta1), (float)beta2,
                         (float)(1.0 - beta2), eps, (const float*)ctrl);
    else
      hipLaunchKernelGGL(adamw_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, (float)(1.0 - beta1), (float)beta2,
                         (float)(1.0 - beta2), eps);
    DCN_CHECK_LAUNCH(who);
  }
  return DCN_OK;
}

extern "C" int dcn_adamw_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                              const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps, void* stream) {
  return adamw_step("adamw_step", params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, nullptr, stream);
}

extern "C" int dcn_adamw_step_clipped(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                      const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                                      const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adamw_step_clipped: no control block");
  return adamw_step("adamw_step_clipped", params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, ctrl, stream);
}

// ---- weight EMA and swap: any count (0 launches nothing), tensors of 0 values allowed (their pointers may be NULL) -----------------
extern "C" int dcn_ema_prepare(int* step, float* w, double decay, double tau, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(step && w, "ema_prepare: bad argument");
  DCN_CHECK_ARG(decay >= 0.0 && decay < 1.0, "ema_prepare: decay %g outside [0, 1)", decay);
  DCN_CHECK_ARG(tau >= 0.0, "ema_prepare: tau %g is negative", tau);          // (a NaN fails both tests)
  hipLaunchKernelGGL(ema_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, w, decay, tau, (const int*)ctrl);
  DCN_CHECK_LAUNCH("ema_prepare");
  return DCN_OK;
}

extern "C" int dcn_ema_update(float* const* shadow, const float* const* src, const int64_t* numel, int count, const float* w, const void* ctrl,
                              void* stream) {
  DCN_CHECK_ARG(count >= 0 && w && (count == 0 || (shadow && src && numel)), "ema_update: bad argument");
  for (int i = 0; i < count; ++i)
    DCN_CHECK_ARG(numel[i] >= 0 && (numel[i] == 0 || (shadow[i] && src[i])), "ema_update: null tensor %d", i);
  for (int base = 0; base < count; base += RMS_CHUNK) {
    EmaChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      c.s[i] = shadow[base + i]; c.x[i] = src[base + i]; c.n[i] = numel[base + i];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    if (biggest == 0) continue;                // a chunk of empty tensors
    hipLaunchKernelGGL(ema_update_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, w, (const int*)ctrl);
    DCN_CHECK_LAUNCH("ema_update");
  }
  return DCN_OK;
}

extern "C" int dcn_tensor_swap(float* const* a, float* const* b, const int64_t* numel, int count, void* stream) {
  DCN_CHECK_ARG(count >= 0 && (count == 0 || (a && b && numel)), "tensor_swap: bad argument");
  for (int i = 0; i < count; ++i)
    DCN_CHECK_ARG(numel[i] >= 0 && (numel[i] == 0 || (a[i] && b[i])), "tensor_swap: null tensor %d", i);
  for (int base = 0; base < count; base += RMS_CHUNK) {
    SwapChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      c.a[i] = a[base + i]; c.b[i] = b[base + i]; c.n[i] = numel[base + i];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    if (biggest == 0) continue;
    hipLaunchKernelGGL(tensor_swap_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c);
    DCN_CHECK_LAUNCH("tensor_swap");
  }
  return DCN_OK;
}
