// Fused multi-tensor optimiser steps — the three optimisers the reference's driver offers (train_DCNet.py:527-534): one pass over
// parameter, gradient and state instead of the element-wise passes of torch's foreach implementations.  HBM-bound:
//   RMSprop (momentum = 0, centered = False)      12 B read + 8 B written per parameter
//   Adam (amsgrad = False, maximize = False)      16 B read + 12 B written
//   SGD with momentum (dampening = 0, no Nesterov) 12 B read + 8 B written
//
// How the file is put together.  Tensors travel to the kernels as pointer chunks of 32 in the kernel arguments (Chunk<K>: no table
// upload); block (x, y) works on tensor y of its chunk.  The element walk is written once: `walk` (16-byte body where every pointer
// of the tensor is 16-byte aligned, scalar tail, grid-stride) and around it `update_walk` (tensor selection and the clipped form's
// prologue), so an update kernel is its update function (`rms_update`, `adam_update`, `adamw_update`, `sgd_update`) in a lambda,
// with the values of the launch and of the tensor (the device learning rate, Adam's scalars) read in front of the walk.  `walk2` is
// the two-trips-at-once form of the two-stream passes (EMA, swap); `grad_sumsq_kernel` keeps its own four-deep loop; the gradient-
// accumulation pass (`grad_accumulate_kernel`) is three lambdas on `walk`, chosen by a phase word on the device.  On the host
// every entry point checks all its tensors (`check_tensors`) and then goes through one launcher (`launch_chunks`, on `for_chunks`).
// A new optimiser is an update function, a kernel pair of a few lines and an entry-point pair.
#include "common.h"

namespace {

constexpr int RMS_CHUNK = 32;                 // tensors per launch (pointers travel as kernel arguments: no table upload)
// K pointer tables and the element counts of up to 32 tensors.  The update kernels: table 0 the parameter, 1 the gradient, 2 ... the
// state tensors (Adam: 4 the tensor's scalars); the others say which is which where they read them.
template <int K> struct Chunk { float* t[K][RMS_CHUNK]; long long n[RMS_CHUNK]; };

// The element walk over one tensor of `n` values, blocks of 256 along x: W tensors that are read and written, w[0 .. W), and under
// READ one that is only read, g.  f(a, ge) updates the W values a[] of one element, ge = g's value there (0 without READ).  Four
// elements per thread and trip through 16-byte accesses where every pointer is 16-byte aligned, else (a view into a flat buffer)
// and for the last n % 4 values one element at a time: f must round alike on both paths (contraction off in the update functions).
template <int W, bool READ, class F>
__device__ __forceinline__ void walk(float* const (&w)[W], const float* __restrict__ g, const long long n, F f) {
  uintptr_t bits = READ ? (uintptr_t)g : 0;
#pragma unroll
  for (int k = 0; k < W; ++k) bits |= (uintptr_t)w[k];
  const long long n4 = (bits & 15) == 0 ? n / 4 : 0;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 x[W];
#pragma unroll
    for (int k = 0; k < W; ++k) x[k] = reinterpret_cast<const f32x4*>(w[k])[i];
    const f32x4 gg = READ ? reinterpret_cast<const f32x4*>(g)[i] : f32x4{};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a[W];
#pragma unroll
      for (int k = 0; k < W; ++k) a[k] = x[k][e];
      f(a, gg[e]);
#pragma unroll
      for (int k = 0; k < W; ++k) x[k][e] = a[k];
    }
#pragma unroll
    for (int k = 0; k < W; ++k) reinterpret_cast<f32x4*>(w[k])[i] = x[k];
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float a[W];
#pragma unroll
    for (int k = 0; k < W; ++k) a[k] = w[k][i];
    f(a, READ ? g[i] : 0.f);
#pragma unroll
    for (int k = 0; k < W; ++k) w[k][i] = a[k];
  }
}

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

// The walk of an update kernel: tensor blockIdx.y of the chunk, parameter and NS state tensors read and written, the gradient read;
// f(a, g) with a[0] the parameter's value, a[1 .. NS] the state's, g the gradient's (times the coefficient under CLIP).
template <bool CLIP, int NS, int K, class F>
__device__ __forceinline__ void update_walk(const Chunk<K>& c, const float* __restrict__ ctl, F f) {
  static_assert(K >= 2 + NS, "parameter, gradient and NS state tables");
  float coef = 1.f;
  if (CLIP) {
    if (reinterpret_cast<const int*>(ctl)[CTL_APPLY] == 0) return;
    coef = ctl[CTL_COEF];
  }
  const int t = blockIdx.y;
  float* w[1 + NS];
  w[0] = c.t[0][t];
#pragma unroll
  for (int k = 0; k < NS; ++k) w[1 + k] = c.t[2 + k][t];
  walk<1 + NS, true>(w, c.t[1][t], c.n[t], [=](float (&a)[1 + NS], const float g0) { f(a, CLIP ? clip_mul(g0, coef) : g0); });
}

template <bool CLIP>
__device__ __forceinline__ void rmsprop_body(const Chunk<3>& c, float lr, const float* __restrict__ lr_dev, float alpha, float eps, float wd,
                                             const float* __restrict__ ctl) {
  if (lr_dev) lr = lr_dev[0];                 // a captured step (hipGraph) reads its learning rate from device memory
  update_walk<CLIP, 1>(c, ctl, [=](float (&a)[2], const float g) { rms_update(a[0], g, a[1], lr, alpha, eps, wd); });
}

__global__ __launch_bounds__(256) void rmsprop_kernel(const Chunk<3> c, float lr, const float* __restrict__ lr_dev, float alpha, float eps, float wd) {
  rmsprop_body<false>(c, lr, lr_dev, alpha, eps, wd, nullptr);
}
__global__ __launch_bounds__(256) void rmsprop_clip_kernel(const Chunk<3> c, float lr, const float* __restrict__ lr_dev, float alpha, float eps, float wd,
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
__device__ __forceinline__ void adam_body(const Chunk<5>& c, float w1, float beta2, float w2, float eps, float wd, const float* __restrict__ ctl) {
  const float* __restrict__ s = c.t[4][blockIdx.y];                     // (adam_prepare_kernel wrote them in the launch before this one)
  const float step_size = s[0], inv_bc2_sqrt = s[1], decay = DECOUPLED ? s[2] : 1.f;
  update_walk<CLIP, 2>(c, ctl, [=](float (&a)[3], const float g) {
    if (DECOUPLED) adamw_update(a[0], g, a[1], a[2], step_size, inv_bc2_sqrt, decay, w1, beta2, w2, eps);
    else adam_update(a[0], g, a[1], a[2], step_size, inv_bc2_sqrt, w1, beta2, w2, eps, wd);
  });
}

__global__ __launch_bounds__(256) void adamw_kernel(const Chunk<5> c, float w1, float beta2, float w2, float eps) {
  adam_body<false, true>(c, w1, beta2, w2, eps, 0.f, nullptr);
}
__global__ __launch_bounds__(256) void adamw_clip_kernel(const Chunk<5> c, float w1, float beta2, float w2, float eps, const float* __restrict__ ctl) {
  adam_body<true, true>(c, w1, beta2, w2, eps, 0.f, ctl);
}

__global__ __launch_bounds__(256) void adam_kernel(const Chunk<5> c, float w1, float beta2, float w2, float eps, float wd) {
  adam_body<false>(c, w1, beta2, w2, eps, wd, nullptr);
}
__global__ __launch_bounds__(256) void adam_clip_kernel(const Chunk<5> c, float w1, float beta2, float w2, float eps, float wd,
                                                        const float* __restrict__ ctl) {
  adam_body<true>(c, w1, beta2, w2, eps, wd, ctl);
}

// ---- SGD with momentum --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sgd_update(float& p, const float g0, float& buf, float lr, float mu, float wd) {
#pragma clang fp contract(off)
  const float g = wd != 0.f ? g0 + wd * p : g0;          // grad = grad.add(param, alpha=weight_decay)
  buf = buf * mu + g;                                    // buf.mul_(momentum).add_(grad)   (first step: buf = grad, which a zero buffer gives)
  p = p - lr * buf;                                      // param.add_(buf, alpha=-lr)
}

template <bool CLIP>
__device__ __forceinline__ void sgd_body(const Chunk<3>& c, float lr, const float* __restrict__ lr_dev, float mu, float wd, const float* __restrict__ ctl) {
  if (lr_dev) lr = lr_dev[0];
  update_walk<CLIP, 1>(c, ctl, [=](float (&a)[2], const float g) { sgd_update(a[0], g, a[1], lr, mu, wd); });
}

__global__ __launch_bounds__(256) void sgd_kernel(const Chunk<3> c, float lr, const float* __restrict__ lr_dev, float mu, float wd) {
  sgd_body<false>(c, lr, lr_dev, mu, wd, nullptr);
}
__global__ __launch_bounds__(256) void sgd_clip_kernel(const Chunk<3> c, float lr, const float* __restrict__ lr_dev, float mu, float wd,
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

// The walk of the two-stream passes over tensor blockIdx.y of the chunk, a = table 0 and b = table 1: f(x, y) on the values of one
// element; a is written back, b under WB.  `walk`'s paths, but two trips at once — four 16-byte loads in flight per thread (these
// passes have two streams where the optimiser updates have three or four).  Every value is handled by exactly one thread.
template <bool WB, class F>
__device__ __forceinline__ void walk2(const Chunk<2>& c, F f) {
  const int t = blockIdx.y;
  float* __restrict__ a = c.t[0][t]; float* __restrict__ b = c.t[1][t];
  const long long n = c.n[t];
  const long long n4 = ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) ? n / 4 : 0;
  const long long stride = (long long)gridDim.x * 256;
  f32x4* __restrict__ a4 = reinterpret_cast<f32x4*>(a); f32x4* __restrict__ b4 = reinterpret_cast<f32x4*>(b);
  const auto f4 = [&](f32x4& x, f32x4& y) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xe = x[e], ye = y[e];
      f(xe, ye);
      x[e] = xe; y[e] = ye;
    }
  };
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    f32x4 x0 = a4[i], x1 = a4[i + stride], y0 = b4[i], y1 = b4[i + stride];
    f4(x0, y0); f4(x1, y1);
    a4[i] = x0; a4[i + stride] = x1;
    if (WB) { b4[i] = y0; b4[i + stride] = y1; }
  }
  for (; i < n4; i += stride) {
    f32x4 x0 = a4[i], y0 = b4[i];
    f4(x0, y0);
    a4[i] = x0;
    if (WB) b4[i] = y0;
  }
  for (i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float x = a[i], y = b[i];
    f(x, y);
    a[i] = x;
    if (WB) b[i] = y;
  }
}

// torch's fp32 lerp (the form adam_update uses for exp_avg).  x == s gives d = 0 and keeps s bit for bit in either form, but for
// s = -0.0 under w < 0.5 (-0 + 0 is +0): the select keeps that one too, so a tensor nobody trains never changes a bit.
__device__ __forceinline__ float ema_lerp(const float s, const float x, const float w) {
#pragma clang fp contract(off)
  const float d = x - s;
  const float r = w < 0.5f ? s + w * d : x - d * (1.f - w);
  return d == 0.f ? s : r;
}

// (tables: 0 the shadow, 1 the source)
__global__ __launch_bounds__(256) void ema_update_kernel(const Chunk<2> c, const float* __restrict__ wp, const int* __restrict__ ctl) {
  if (ctl && ctl[CTL_APPLY] == 0) return;
  const float w = wp[0];                      // (ema_prepare_kernel wrote it in the launch before this one)
  walk2<false>(c, [=](float& s, float& x) { s = ema_lerp(s, x, w); });
}

// a <-> b: 8 B read + 8 B written per value
__global__ __launch_bounds__(256) void tensor_swap_kernel(const Chunk<2> c) {
  walk2<true>(c, [](float& a, float& b) { const float a0 = a; a = b; b = a0; });
}

// ---- global gradient norm ---------------------------------------------------------------------------------------------------------
// One more read of the gradients: every block sums the squares of its share of one tensor in double (the product of two floats is
// exact in double, so contraction cannot change a bit) and writes ONE double into its own slot — slot (chunk, tensor in chunk,
// blockIdx.x), every launched block writes, 0.0 when it had no work.  grad_clip_coef_kernel adds the slots in a fixed order.  No
// atomics, no arrival counters: the norm is the same bits in every run, eager or replayed.  A thread takes the same four
// consecutive values per trip whether the pointer is 16-byte aligned (one 16-byte load) or not (four 4-byte loads), so a view
// into a flat gradient buffer gives the same bits as an aligned tensor.

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

// (table 0: the gradients, read only)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const Chunk<1> c, double* __restrict__ partials) {
  __shared__ double red[4];
  const int t = blockIdx.y;
  const float* __restrict__ g = c.t[0][t];
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
__device__ __forceinline__ void clip_coef_body(const double* __restrict__ partials, long long slots, float max_norm, int skip_nonfinite,
                                               float* __restrict__ ctl, double* red) {
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

__global__ __launch_bounds__(1024) void grad_clip_coef_kernel(const double* __restrict__ partials, long long slots, float max_norm, int skip_nonfinite,
                                                              float* __restrict__ ctl) {
  __shared__ double red[16];
  clip_coef_body(partials, slots, max_norm, skip_nonfinite, ctl, red);
}

// ---- gradient accumulation over K calls ---------------------------------------------------------------------------------------------
// The accumulation block, four 32-bit words on the device (include/dcnet_hip.h, dcn_accum_prepare): [0] int32 pos, the calls made in
// the open window (0 once a window has closed), [1] int32 phase of the current call, [2] float inv_k, [3] int32 windows closed.  Like
// Adam's step words the position lives on the device, so a replayed step walks through the window without the host:
// accum_prepare_kernel — one thread, in front of the pass — advances it; the pass and the gated coefficient kernel read the phase.
constexpr int ACC_POS = 0, ACC_PHASE = 1, ACC_INV_K = 2, ACC_WINDOWS = 3;
constexpr int ACC_FIRST = 0, ACC_MIDDLE = 1, ACC_BOUNDARY = 2, ACC_ALONE = 3;      // ALONE: a window of one call (k = 1), the gradient is the mean

__global__ __launch_bounds__(64) void accum_prepare_kernel(int* __restrict__ blk, int k) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int pos = blk[ACC_POS] + 1;
  const bool closes = pos >= k;
  blk[ACC_POS] = closes ? 0 : pos;
  blk[ACC_PHASE] = closes ? (pos == 1 ? ACC_ALONE : ACC_BOUNDARY) : (pos == 1 ? ACC_FIRST : ACC_MIDDLE);
  reinterpret_cast<float*>(blk)[ACC_INV_K] = (float)(1.0 / k);
  if (closes) blk[ACC_WINDOWS] = blk[ACC_WINDOWS] + 1;
}

// fp32 additions in call order, one final multiplication: ((g1 + g2) + ... + gK) * inv_k, every operation rounded once
__device__ __forceinline__ float accum_add(const float acc, const float g) {
#pragma clang fp contract(off)
  return acc + g;
}
__device__ __forceinline__ float accum_mean(const float acc, const float g, const float inv_k) {
#pragma clang fp contract(off)
  const float s = acc + g;
  return s * inv_k;
}

// (tables: 0 the accumulation buffer, 1 the gradient)  One walk per block, chosen by the phase — the same for every block of the
// launch: first acc = g (acc is not read: 8 B per value), middle acc += g (12 B), boundary g = (acc + g) * inv_k (12 B; acc is not
// written, the next window's first call overwrites it).  The walk's alignment test covers both pointers in every phase.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(const Chunk<2> c, const int* __restrict__ blk) {
  const int phase = blk[ACC_PHASE];           // (accum_prepare_kernel wrote it in the launch before this one)
  const int t = blockIdx.y;
  float* const acc[1] = {c.t[0][t]};
  float* const g[1] = {c.t[1][t]};
  const long long n = c.n[t];
  if (phase == ACC_FIRST) {
    walk<1, true>(acc, g[0], n, [](float (&a)[1], const float ge) { a[0] = ge; });
  } else if (phase == ACC_MIDDLE) {
    walk<1, true>(acc, g[0], n, [](float (&a)[1], const float ge) { a[0] = accum_add(a[0], ge); });
  } else if (phase == ACC_BOUNDARY) {
    const float inv_k = reinterpret_cast<const float*>(blk)[ACC_INV_K];
    walk<1, true>(g, acc[0], n, [=](float (&a)[1], const float ae) { a[0] = accum_mean(ae, a[0], inv_k); });
  }
}

// grad_clip_coef_kernel behind the window: off the boundary apply = 0 and nothing else is touched (norm, coefficient and skips keep
// the last closed window's values), on it exactly what grad_clip_coef_kernel writes.  partials = NULL (no norm was asked for):
// coef = 1, apply = boundary, launched with one wave.
__global__ __launch_bounds__(1024) void accum_clip_coef_kernel(const double* __restrict__ partials, long long slots, float max_norm, int skip_nonfinite,
                                                               const int* __restrict__ blk, float* __restrict__ ctl) {
  __shared__ double red[16];
  const int phase = blk[ACC_PHASE];
  const bool boundary = phase == ACC_BOUNDARY || phase == ACC_ALONE;
  if (!boundary || !partials) {
    if (threadIdx.x != 0) return;
    if (!partials) ctl[CTL_COEF] = 1.f;
    reinterpret_cast<int*>(ctl)[CTL_APPLY] = boundary ? 1 : 0;
    return;
  }
  clip_coef_body(partials, slots, max_norm, skip_nonfinite, ctl, red);
}

// (table 0: the gradients, scaled in place whatever `apply` says — the stand-alone clip_grad_norm_)
__global__ __launch_bounds__(256) void grad_scale_kernel(const Chunk<1> c, const float* __restrict__ ctl) {
  const float coef = ctl[CTL_COEF];
  float* const w[1] = {c.t[0][blockIdx.y]};
  walk<1, false>(w, nullptr, c.n[blockIdx.y], [=](float (&a)[1], float) { a[0] = clip_mul(a[0], coef); });
}

// ---- host: the chunked launches -----------------------------------------------------------------------------------------------------
// blocks along x for a chunk whose longest tensor has `biggest` values (grid-stride beyond 128)
inline unsigned blocks_for(long long biggest) {
  const long long bx = (biggest / 4 + 255) / 256;
  return (unsigned)(bx < 1 ? 1 : (bx > 128 ? 128 : bx));
}
inline long long longest(const int64_t* numel, int m) {
  long long biggest = 0;
  for (int i = 0; i < m; ++i)
    if (numel[i] > biggest) biggest = numel[i];
  return biggest;
}

// The chunk loop: f(base, m) for the tensors [base, base + m) of every chunk of at most `cap`, until one does not return DCN_OK.
template <class F>
inline int for_chunks(int count, int cap, F f) {
  for (int base = 0; base < count; base += cap) {
    const int e = f(base, count - base < cap ? count - base : cap);
    if (e != DCN_OK) return e;
  }
  return DCN_OK;
}

// slots of the partials buffer for `count` tensors: per chunk of 32, blocks_for(its longest tensor) x tensors in the chunk
inline long long sumsq_slots(const int64_t* numel, int count) {
  long long total = 0;
  for_chunks(count, RMS_CHUNK, [&](int base, int m) {
    total += (long long)blocks_for(longest(numel + base, m)) * m;
    return DCN_OK;
  });
  return total;
}

// The K pointer tables of an entry point, in its kernel's table order.
template <int K> using Tables = const float* const* const (&)[K];

// Every tensor is looked at before the first launch: no null pointer, no negative count.  `empties`: a tensor of 0 values may be NULL.
template <int K>
int check_tensors(const char* who, Tables<K> tab, const int64_t* numel, int count, bool empties = false) {
  for (int k = 0; k < count; ++k) {
    bool there = true;
    for (int j = 0; j < K; ++j) there = there && tab[j][k];
    DCN_CHECK_ARG(numel[k] >= 0 && (there || (empties && numel[k] == 0)), "%s: null tensor %d", who, k);
  }
  return DCN_OK;
}

// The one chunked launch: 32 tensors per launch, launch(chunk, grid) with grid = (blocks_for(the chunk's longest tensor), tensors in
// the chunk).  `empties` (EMA, swap): a chunk of empty tensors launches nothing.
template <int K, class L>
int launch_chunks(const char* who, Tables<K> tab, const int64_t* numel, int count, bool empties, L launch) {
  return for_chunks(count, RMS_CHUNK, [&](int base, int m) -> int {
    Chunk<K> c{};
    for (int i = 0; i < m; ++i) {
      for (int j = 0; j < K; ++j) c.t[j][i] = const_cast<float*>(tab[j][base + i]);
      c.n[i] = numel[base + i];
    }
    const long long biggest = longest(numel + base, m);
    if (empties && biggest == 0) return DCN_OK;
    launch(c, dim3(blocks_for(biggest), m));
    DCN_CHECK_LAUNCH(who);
    return DCN_OK;
  });
}

#define OPTIM_LAUNCH(kernel, ...) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__)

}  // namespace

extern "C" int64_t dcn_grad_sumsq_slots(const int64_t* numel, int count) {
  if (!numel || count <= 0) { dcn_set_error("grad_sumsq_slots: bad argument"); return -1; }
  for (int i = 0; i < count; ++i)
    if (numel[i] < 0) { dcn_set_error("grad_sumsq_slots: negative element count of tensor %d", i); return -1; }
  return sumsq_slots(numel, count);
}

extern "C" int dcn_grad_sumsq(const float* const* grads, const int64_t* numel, int count, double* partials, int64_t slots, void* stream) {
  DCN_CHECK_ARG(grads && numel && partials && count > 0, "grad_sumsq: bad argument");
  if (const int e = check_tensors<1>("grad_sumsq", {grads}, numel, count)) return e;
  DCN_CHECK_ARG(slots == sumsq_slots(numel, count), "grad_sumsq: the partials buffer has %lld slots, these tensors need %lld (dcn_grad_sumsq_slots)",
                (long long)slots, sumsq_slots(numel, count));
  long long at = 0;
  return launch_chunks<1>("grad_sumsq", {grads}, numel, count, false, [&](const Chunk<1>& c, dim3 grid) {
    OPTIM_LAUNCH(grad_sumsq_kernel, c, partials + at);
    at += (long long)grid.x * grid.y;
  });
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
  if (const int e = check_tensors<1>("grad_scale", {grads}, numel, count)) return e;
  return launch_chunks<1>("grad_scale", {grads}, numel, count, false,
                          [&](const Chunk<1>& c, dim3 grid) { OPTIM_LAUNCH(grad_scale_kernel, c, (const float*)ctrl); });
}

// The update entry points come in two forms over one body each: the plain one launches the kernels it always launched, the
// `_clipped` one (ctl = the control block dcn_grad_clip_coef wrote, non-NULL) their clipped forms.
static int rmsprop_step(const char* who, float* const* params, const float* const* grads, float* const* square_avgs, const int64_t* numel,
                        int count, float lr, const float* lr_dev, float alpha, float eps, float weight_decay, const float* ctl, void* stream) {
  DCN_CHECK_ARG(params && grads && square_avgs && numel && count > 0, "%s: bad argument", who);
  if (const int e = check_tensors<3>(who, {params, grads, square_avgs}, numel, count)) return e;
  return launch_chunks<3>(who, {params, grads, square_avgs}, numel, count, false, [&](const Chunk<3>& c, dim3 grid) {
    if (ctl) OPTIM_LAUNCH(rmsprop_clip_kernel, c, lr, lr_dev, alpha, eps, weight_decay, ctl);
    else OPTIM_LAUNCH(rmsprop_kernel, c, lr, lr_dev, alpha, eps, weight_decay);
  });
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

// Adam and AdamW (`decoupled`: its own entry points, three scalars per tensor — Adam's keep theirs and their two) differ in the
// weight-decay check, in `weight_decay` (Adam: an argument of the update; AdamW: of the prepare launch, the third scalar) and in the kernels.
static int adam_prepare(const char* who, bool decoupled, int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1,
                        double beta2, double weight_decay, const int* ctl, void* stream) {
  DCN_CHECK_ARG(steps && scal && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
  DCN_CHECK_ARG(!decoupled || weight_decay >= 0.0, "%s: negative weight_decay", who);
  for (int k = 0; k < count; ++k)
    DCN_CHECK_ARG(steps[k] && scal[k], "%s: null tensor %d", who, k);
  return for_chunks(count, STEP_CHUNK, [&](int base, int m) -> int {
    StepChunk c{};
    for (int i = 0; i < m; ++i) { c.step[i] = steps[base + i]; c.scal[i] = scal[base + i]; }
    const dim3 grid(m), block(64);
    if (decoupled) hipLaunchKernelGGL(adamw_prepare_kernel, grid, block, 0, (hipStream_t)stream, c, lr, lr_dev, beta1, beta2, weight_decay, ctl);
    else if (ctl) hipLaunchKernelGGL(adam_prepare_clip_kernel, grid, block, 0, (hipStream_t)stream, c, lr, lr_dev, beta1, beta2, ctl);
    else hipLaunchKernelGGL(adam_prepare_kernel, grid, block, 0, (hipStream_t)stream, c, lr, lr_dev, beta1, beta2);
    DCN_CHECK_LAUNCH(who);
    return DCN_OK;
  });
}

extern "C" int dcn_adam_prepare(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                void* stream) {
  return adam_prepare("adam_prepare", false, steps, scal, count, lr, lr_dev, beta1, beta2, 0.0, nullptr, stream);
}

extern "C" int dcn_adam_prepare_clipped(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                        const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adam_prepare_clipped: no control block");
  return adam_prepare("adam_prepare_clipped", false, steps, scal, count, lr, lr_dev, beta1, beta2, 0.0, (const int*)ctrl, stream);
}

extern "C" int dcn_adamw_prepare(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                 double weight_decay, void* stream) {
  return adam_prepare("adamw_prepare", true, steps, scal, count, lr, lr_dev, beta1, beta2, weight_decay, nullptr, stream);
}

extern "C" int dcn_adamw_prepare_clipped(int* const* steps, float* const* scal, int count, float lr, const float* lr_dev, double beta1, double beta2,
                                         double weight_decay, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adamw_prepare_clipped: no control block");
  return adam_prepare("adamw_prepare_clipped", true, steps, scal, count, lr, lr_dev, beta1, beta2, weight_decay, (const int*)ctrl, stream);
}

static int adam_step(const char* who, bool decoupled, float* const* params, const float* const* grads, float* const* exp_avgs,
                     float* const* exp_avg_sqs, const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                     float weight_decay, const float* ctl, void* stream) {
  DCN_CHECK_ARG(params && grads && exp_avgs && exp_avg_sqs && scal && numel && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
  if (decoupled) DCN_CHECK_ARG(eps >= 0.f, "%s: negative eps", who);
  else DCN_CHECK_ARG(eps >= 0.f && weight_decay >= 0.f, "%s: negative eps or weight_decay", who);
  if (const int e = check_tensors<5>(who, {params, grads, exp_avgs, exp_avg_sqs, scal}, numel, count)) return e;
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  return launch_chunks<5>(who, {params, grads, exp_avgs, exp_avg_sqs, scal}, numel, count, false, [&](const Chunk<5>& c, dim3 grid) {
    if (decoupled && ctl) OPTIM_LAUNCH(adamw_clip_kernel, c, w1, b2, w2, eps, ctl);
    else if (decoupled) OPTIM_LAUNCH(adamw_kernel, c, w1, b2, w2, eps);
    else if (ctl) OPTIM_LAUNCH(adam_clip_kernel, c, w1, b2, w2, eps, weight_decay, ctl);
    else OPTIM_LAUNCH(adam_kernel, c, w1, b2, w2, eps, weight_decay);
  });
}

extern "C" int dcn_adam_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                             const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                             float weight_decay, void* stream) {
  return adam_step("adam_step", false, params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, weight_decay, nullptr, stream);
}

extern "C" int dcn_adam_step_clipped(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                     const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                                     float weight_decay, const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adam_step_clipped: no control block");
  return adam_step("adam_step_clipped", false, params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, weight_decay,
                   (const float*)ctrl, stream);
}

extern "C" int dcn_adamw_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                              const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps, void* stream) {
  return adam_step("adamw_step", true, params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, 0.f, nullptr, stream);
}

extern "C" int dcn_adamw_step_clipped(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                      const float* const* scal, const int64_t* numel, int count, double beta1, double beta2, float eps,
                                      const void* ctrl, void* stream) {
  DCN_CHECK_ARG(ctrl, "adamw_step_clipped: no control block");
  return adam_step("adamw_step_clipped", true, params, grads, exp_avgs, exp_avg_sqs, scal, numel, count, beta1, beta2, eps, 0.f, (const float*)ctrl,
                   stream);
}

static int sgd_step(const char* who, float* const* params, const float* const* grads, float* const* momentum_bufs, const int64_t* numel, int count,
                    float lr, const float* lr_dev, float momentum, float weight_decay, const float* ctl, void* stream) {
  DCN_CHECK_ARG(params && grads && momentum_bufs && numel && count > 0, "%s: bad argument", who);
  DCN_CHECK_ARG(momentum >= 0.f && weight_decay >= 0.f, "%s: negative momentum or weight_decay", who);
  if (const int e = check_tensors<3>(who, {params, grads, momentum_bufs}, numel, count)) return e;
  return launch_chunks<3>(who, {params, grads, momentum_bufs}, numel, count, false, [&](const Chunk<3>& c, dim3 grid) {
    if (ctl) OPTIM_LAUNCH(sgd_clip_kernel, c, lr, lr_dev, momentum, weight_decay, ctl);
    else OPTIM_LAUNCH(sgd_kernel, c, lr, lr_dev, momentum, weight_decay);
  });
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
  if (const int e = check_tensors<2>("ema_update", {shadow, src}, numel, count, true)) return e;
  return launch_chunks<2>("ema_update", {shadow, src}, numel, count, true,
                          [&](const Chunk<2>& c, dim3 grid) { OPTIM_LAUNCH(ema_update_kernel, c, w, (const int*)ctrl); });
}

extern "C" int dcn_tensor_swap(float* const* a, float* const* b, const int64_t* numel, int count, void* stream) {
  DCN_CHECK_ARG(count >= 0 && (count == 0 || (a && b && numel)), "tensor_swap: bad argument");
  if (const int e = check_tensors<2>("tensor_swap", {a, b}, numel, count, true)) return e;
  return launch_chunks<2>("tensor_swap", {a, b}, numel, count, true, [&](const Chunk<2>& c, dim3 grid) { OPTIM_LAUNCH(tensor_swap_kernel, c); });
}

// ---- gradient accumulation: the window's position, the pass, the gated coefficient --------------------------------------------------
extern "C" int dcn_accum_prepare(void* accum, int k, void* stream) {
  DCN_CHECK_ARG(accum, "accum_prepare: no accumulation block");
  DCN_CHECK_ARG(k >= 1, "accum_prepare: k = %d, a window has at least one call", k);
  hipLaunchKernelGGL(accum_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (int*)accum, k);
  DCN_CHECK_LAUNCH("accum_prepare");
  return DCN_OK;
}

extern "C" int dcn_grad_accumulate(float* const* acc, float* const* grads, const int64_t* numel, int count, const void* accum, void* stream) {
  DCN_CHECK_ARG(count >= 0 && (count == 0 || (acc && grads && numel)), "grad_accumulate: bad argument");
  DCN_CHECK_ARG(accum, "grad_accumulate: no accumulation block");
  if (const int e = check_tensors<2>("grad_accumulate", {acc, grads}, numel, count, true)) return e;
  return launch_chunks<2>("grad_accumulate", {acc, grads}, numel, count, true,
                          [&](const Chunk<2>& c, dim3 grid) { OPTIM_LAUNCH(grad_accumulate_kernel, c, (const int*)accum); });
}

extern "C" int dcn_accum_clip_coef(const double* partials, int64_t slots, float max_norm, int skip_nonfinite, const void* accum, void* ctrl,
                                   void* stream) {
  DCN_CHECK_ARG(ctrl && slots >= 0 && (partials != nullptr) == (slots > 0), "accum_clip_coef: bad argument");
  DCN_CHECK_ARG(accum, "accum_clip_coef: no accumulation block");
  DCN_CHECK_ARG(!partials || max_norm > 0.f, "accum_clip_coef: max_norm %g is not a positive number", (double)max_norm);
  hipLaunchKernelGGL(accum_clip_coef_kernel, dim3(1), dim3(partials ? 1024 : 64), 0, (hipStream_t)stream, partials, (long long)slots, max_norm,
                     skip_nonfinite, (const int*)accum, (float*)ctrl);
  DCN_CHECK_LAUNCH("accum_clip_coef");
  return DCN_OK;
}
