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

__global__ __launch_bounds__(256) void rmsprop_kernel(const RmsChunk c, float lr, const float* __restrict__ lr_dev, float alpha, float eps, float wd) {
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
    for (int e = 0; e < 4; ++e) { float a = pp[e], b = vv[e]; rms_update(a, gg[e], b, lr, alpha, eps, wd); pp[e] = a; vv[e] = b; }
    reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    rms_update(p[i], g[i], v[i], lr, alpha, eps, wd);
}

// ---- Adam ---------------------------------------------------------------------------------------------------------------------
// Adam's bias corrections depend on the step count t, and a replayed hipGraph must advance t without the host: every tensor has a
// device step word, and adam_prepare_kernel — one launch in front of the update, eager or captured alike — advances it and forms the
// two scalars of the step from it: scal[0] = lr / (1 - beta1^t), scal[1] = 1 / sqrt(1 - beta2^t), in double as torch's Python does.
constexpr int STEP_CHUNK = 128;
struct StepChunk { int* step[STEP_CHUNK]; float* scal[STEP_CHUNK]; };

__global__ __launch_bounds__(64) void adam_prepare_kernel(const StepChunk c, float lr, const float* __restrict__ lr_dev, double beta1, double beta2) {
  if (threadIdx.x != 0) return;
  if (lr_dev) lr = lr_dev[0];
  const int t = c.step[blockIdx.x][0] + 1;
  c.step[blockIdx.x][0] = t;
  const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
  c.scal[blockIdx.x][0] = (float)((double)lr / bc1);          // step_size = lr / bias_correction1
  c.scal[blockIdx.x][1] = (float)(1.0 / sqrt(bc2));           // torch divides sqrt(v) by the scalar sqrt(bc2): a multiplication by its inverse
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

__global__ __launch_bounds__(256) void adam_kernel(const AdamChunk c, float w1, float beta2, float w2, float eps, float wd) {
  const int t = blockIdx.y;
  float* __restrict__ p = c.p[t]; const float* __restrict__ g = c.g[t]; float* __restrict__ m = c.m[t]; float* __restrict__ v = c.v[t];
  const float step_size = c.s[t][0], inv_bc2_sqrt = c.s[t][1];          // (adam_prepare_kernel wrote them in the launch before this one)
  const long long n = c.n[t];
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  const long long n4 = vec ? n / 4 : 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i], mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = pp[e], b = mm[e], d = vv[e];
      adam_update(a, gg[e], b, d, step_size, inv_bc2_sqrt, w1, beta2, w2, eps, wd);
      pp[e] = a; mm[e] = b; vv[e] = d;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(m)[i] = mm; reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    adam_update(p[i], g[i], m[i], v[i], step_size, inv_bc2_sqrt, w1, beta2, w2, eps, wd);
}

// ---- SGD with momentum --------------------------------------------------------------------------------------------------------
// (same shape as RmsChunk: parameter, gradient, one state tensor)
__device__ __forceinline__ void sgd_update(float& p, const float g0, float& buf, float lr, float mu, float wd) {
#pragma clang fp contract(off)
  const float g = wd != 0.f ? g0 + wd * p : g0;          // grad = grad.add(param, alpha=weight_decay)
  buf = buf * mu + g;                                    // buf.mul_(momentum).add_(grad)   (first step: buf = grad, which a zero buffer gives)
  p = p - lr * buf;                                      // param.add_(buf, alpha=-lr)
}

__global__ __launch_bounds__(256) void sgd_kernel(const RmsChunk c, float lr, const float* __restrict__ lr_dev, float mu, float wd) {
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
    for (int e = 0; e < 4; ++e) { float a = pp[e], d = bb[e]; sgd_update(a, gg[e], d, lr, mu, wd); pp[e] = a; bb[e] = d; }
    reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(b)[i] = bb;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    sgd_update(p[i], g[i], b[i], lr, mu, wd);
}

// blocks along x for a chunk whose longest tensor has `biggest` values (grid-stride beyond 128)
inline unsigned blocks_for(long long biggest) {
  const long long bx = (biggest / 4 + 255) / 256;
  return (unsigned)(bx < 1 ? 1 : (bx > 128 ? 128 : bx));
}

}  // namespace

extern "C" int dcn_rmsprop_step(float* const* params, const float* const* grads, float* const* square_avgs, const int64_t* numel,
                                int count, float lr, const float* lr_dev, float alpha, float eps, float weight_decay, void* stream) {
  DCN_CHECK_ARG(params && grads && square_avgs && numel && count > 0, "rmsprop_step: bad argument");
  for (int base = 0; base < count; base += RMS_CHUNK) {
    RmsChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      DCN_CHECK_ARG(params[base + i] && grads[base + i] && square_avgs[base + i] && numel[base + i] >= 0, "rmsprop_step: null tensor %d", base + i);
      c.p[i] = params[base + i]; c.g[i] = grads[base + i]; c.v[i] = square_avgs[base + i]; c.n[i] = numel[base + i];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    hipLaunchKernelGGL(rmsprop_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, lr, lr_dev, alpha, eps, weight_decay);
    DCN_CHECK_LAUNCH("rmsprop_step");
  }
  return DCN_OK;
}

extern "C" int dcn_adam_prepare(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                void* stream) {
  DCN_CHECK_ARG(steps && scal && count > 0, "adam_prepare: bad argument");
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_prepare: betas (%g, %g) outside [0, 1)", beta1, beta2);
  for (int base = 0; base < count; base += STEP_CHUNK) {
    StepChunk c{};
    const int m = count - base < STEP_CHUNK ? count - base : STEP_CHUNK;
    for (int i = 0; i < m; ++i) {
      DCN_CHECK_ARG(steps[base + i] && scal[base + i], "adam_prepare: null tensor %d", base + i);
      c.step[i] = steps[base + i]; c.scal[i] = scal[base + i];
    }
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(m), dim3(64), 0, (hipStream_t)stream, c, lr, lr_dev, beta1, beta2);
    DCN_CHECK_LAUNCH("adam_prepare");
  }
  return DCN_OK;
}

extern "C" int dcn_adam_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                             const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                             float weight_decay, void* stream) {
  DCN_CHECK_ARG(params && grads && exp_avgs && exp_avg_sqs && scal && numel && count > 0, "adam_step: bad argument");
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_step: betas (%g, %g) outside [0, 1)", beta1, beta2);
  DCN_CHECK_ARG(eps >= 0.f && weight_decay >= 0.f, "adam_step: negative eps or weight_decay");
  for (int base = 0; base < count; base += RMS_CHUNK) {
    AdamChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      const int k = base + i;
      DCN_CHECK_ARG(params[k] && grads[k] && exp_avgs[k] && exp_avg_sqs[k] && scal[k] && numel[k] >= 0, "adam_step: null tensor %d", k);
      c.p[i] = params[k]; c.g[i] = grads[k]; c.m[i] = exp_avgs[k]; c.v[i] = exp_avg_sqs[k]; c.s[i] = scal[k]; c.n[i] = numel[k];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    hipLaunchKernelGGL(adam_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), eps, weight_decay);
    DCN_CHECK_LAUNCH("adam_step");
  }
  return DCN_OK;
}

extern "C" int dcn_sgd_step(float* const* params, const float* const* grads, float* const* momentum_bufs, const int64_t* numel, int count,
                            float lr, const float* lr_dev, float momentum, float weight_decay, void* stream) {
  DCN_CHECK_ARG(params && grads && momentum_bufs && numel && count > 0, "sgd_step: bad argument");
  DCN_CHECK_ARG(momentum >= 0.f && weight_decay >= 0.f, "sgd_step: negative momentum or weight_decay");
  for (int base = 0; base < count; base += RMS_CHUNK) {
    RmsChunk c{};
    const int m = count - base < RMS_CHUNK ? count - base : RMS_CHUNK;
    long long biggest = 0;
    for (int i = 0; i < m; ++i) {
      const int k = base + i;
      DCN_CHECK_ARG(params[k] && grads[k] && momentum_bufs[k] && numel[k] >= 0, "sgd_step: null tensor %d", k);
      c.p[i] = params[k]; c.g[i] = grads[k]; c.v[i] = momentum_bufs[k]; c.n[i] = numel[k];
      if (c.n[i] > biggest) biggest = c.n[i];
    }
    hipLaunchKernelGGL(sgd_kernel, dim3(blocks_for(biggest), m), dim3(256), 0, (hipStream_t)stream, c, lr, lr_dev, momentum, weight_decay);
    DCN_CHECK_LAUNCH("sgd_step");
  }
  return DCN_OK;
}
