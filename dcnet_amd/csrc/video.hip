// Whole-video grounding (dcnet_amd/video.py): every frame is encoded once into a per-scale FEATURE BANK, frame-major, and the
// windows of the inference model (model/test_DCNet_model.py:299-332; the window rule of test_DCNet.py's getChunk) read it through
// strides — the pairs of distance d are f1 = bank[a0 : a0 + n], f2 = bank[a0 + d : a0 + d + n], same batch stride.
//
//   dcn_bank_write        F.normalize of the mapped features (test_DCNet_model.py:299-301) into bank rows AND their f16 two-piece
//                         split form (gemm3.hip) in one pass: the windowed form normalises once per window and splits both
//                         operands of every co-attention call, 2 (K - 1) times per frame.
//   dcn_coattn_bank_fwd   co-attention (test_DCNet_model.py:259-274) of a run of pairs with the operands taken from the split bank:
//                         one affinity, then either or both attended features.  The sequence dcn_coattn_fwd runs behind its pre-split
//                         (coattn.h: coattn_fwd_operands); shapes gemm3.hip does not take read the fp32 rows instead.
//   dcn_bank_write_b16    bf16 storage ("bf16s"): the same pass with the row in bf16 as a third output, bank / split each on request;
//   dcn_bank_concat_b16   corr_conv's bf16 input [f_centre | f_attn] from those rows and the fp32 attended features, one pass (instead of
//                         a copy of the centre rows, a strided fp32 write of the attended half and a cast pass);
//   dcn_coattn_bank_form  which of bank / split dcn_coattn_bank_fwd reads for a shape (a scale keeps only that one).
//   dcn_post_fusion_bank  post_processing.py:246-278 straight from the candidate bank of the centres: window b reads the entries of
//                         centres b - R/2 ... b - R/2 + R - 1 through an index; an entry outside the run is MISSING (:189-193: the
//                         centre's own entry substituted, its weight zeroed after the softmax, :266-269).
#include <math.h>
#include "igemm.h"
#include "prof.h"
#include "coattn.h"
#include "split4.h"
#include "b16_pack.h"

namespace {

constexpr int VF_MAXK = 64;                       // post.hip PK_MAXK
constexpr int VF_MAXR = 32;                       // post.hip PF_MAXR

// One wave per row, the arithmetic of score.hip's l2norm_score_fwd_kernel (same fma chain, same wave reduction: bitwise its result),
// V4 16-byte loads per lane.  A lane's four channels are half of an 8-element run of the split form: 8 bytes of the high piece,
// 8 bytes of the low piece (split4.h, as exp_sums_kernel writes E).
template <int V4>
__global__ __launch_bounds__(256) void bank_write_kernel(const float* __restrict__ x, int ldx, float* __restrict__ bank,
                                                         float* __restrict__ split, int64_t rows, int c) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  f32x4 v[V4];
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    const int ch = (lane + 64 * k) * 4;
    v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ch < c) v[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + row * ldx + ch));
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < V4; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) s = fmaf(v[k][j], v[k][j], s);
  const float inv = 1.f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    const int ch = (lane + 64 * k) * 4;
    if (ch < c) {
      const f32x4 o = v[k] * inv;
      *reinterpret_cast<f32x4*>(bank + row * c + ch) = o;
      split4_store(split + row * c, ch, o * SPLIT_SCALE_ONE);
    }
  }
}

// bf16 storage: bank_write_kernel with a third output, the row in bf16 (what corr_conv reads as the centre half of its input).  Same lane
// pattern, same fma chain and wave reduction, so o is bitwise the value bank_write_kernel stores: rows16 = bf16(o) (b16_pack.h's
// conversion, 8 bytes per lane), split and bank — each only if asked for — its bits.
template <int V4>
__global__ __launch_bounds__(256) void bank_write_b16_kernel(const float* __restrict__ x, int ldx, __bf16* __restrict__ rows16,
                                                             float* __restrict__ bank, float* __restrict__ split, int64_t rows, int c) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  f32x4 v[V4];
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    const int ch = (lane + 64 * k) * 4;
    v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ch < c) v[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + row * ldx + ch));
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < V4; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) s = fmaf(v[k][j], v[k][j], s);
  const float inv = 1.f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    const int ch = (lane + 64 * k) * 4;
    if (ch < c) {
      const f32x4 o = v[k] * inv;
      *reinterpret_cast<b16io::bf16x4_t*>(rows16 + row * c + ch) = b16io::pack4(o);
      if (bank) *reinterpret_cast<f32x4*>(bank + row * c + ch) = o;
      if (split) split4_store(split + row * c, ch, o * SPLIT_SCALE_ONE);
    }
  }
}

// cat [n][hw][2c] bf16 = [rows16 of the centres | bf16(attn)]: a thread moves 8 values per trip — one 16-byte bf16 load or two 16-byte fp32
// loads, one 16-byte store; c / 8 groups of either half, so a wave lies in one half whenever c >= 512.  Grid-stride, 64-bit offsets.  The
// attended features are scratch that nothing reads again (non-temporal); the bank rows are read by every contribution of their frame.
__global__ __launch_bounds__(256) void bank_concat_b16_kernel(const __bf16* __restrict__ rows16, int64_t bs16, const float* __restrict__ attn,
                                                              int ld_attn, int64_t bs_attn, __bf16* __restrict__ cat, int hw, int c,
                                                              int64_t total) {
  const int c8 = c >> 3, g = 2 * c8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / g; const int j = (int)(i - row * g);
    const int64_t f = row / hw; const int64_t p = row - f * hw;
    __bf16* dst = cat + row * 2 * c + (int64_t)j * 8;
    if (j < c8) {
      *reinterpret_cast<b16io::bf16x8_t*>(dst) = *reinterpret_cast<const b16io::bf16x8_t*>(rows16 + f * bs16 + p * c + j * 8);
    } else {
      const float* src = attn + f * bs_attn + p * ld_attn + (j - c8) * 8;
      const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src));
      const f32x4 b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + 4));
      b16io::st8<__bf16>(dst, b16io::F8{{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}});
    }
  }
}

// post.hip's post_fusion_kernel with the window gathered through an index: block (centre candidate c, window b), the same lane
// pattern and operation order, so that the result is bitwise dcn_post_fusion's on the gathered tensor.
__global__ __launch_bounds__(256) void post_fusion_bank_kernel(const float* __restrict__ feats, const float* __restrict__ scores, int n,
                                                               int K, int R, int E, float* __restrict__ fused) {
  __shared__ float sim[VF_MAXR * VF_MAXK];
  __shared__ float cvec[2048];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* cp = feats + ((size_t)b * K + c) * E;
  const bool staged = E <= 2048;
  if (staged) { for (int e = tid; e < E; e += 256) cvec[e] = cp[e]; }
  __syncthreads();
  for (int p = wave; p < R * K; p += 4) {
    const int r = p / K, i = p - r * K;
    int src = b - R / 2 + r;
    if (src < 0 || src >= n) src = b;                                     // missing: the centre's own entry (:189-193)
    const float* rp = feats + ((size_t)src * K + i) * E;
    float acc = 0.f;
    for (int e = lane; e < E; e += 64) acc += (staged ? cvec[e] : cp[e]) * rp[e];
    acc = wave_sum(acc);
    if (lane == 0) sim[p] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    float smax[VF_MAXR], refer[VF_MAXR];
    float mx = -INFINITY;
    for (int r = 0; r < R; ++r) {
      int src = b - R / 2 + r;
      if (src < 0 || src >= n) src = b;
      float best = sim[r * K]; int arg = 0;
      for (int i = 1; i < K; ++i) if (sim[r * K + i] > best) { best = sim[r * K + i]; arg = i; }      // first maximum (:258)
      smax[r] = best; refer[r] = scores[(size_t)src * K + arg];
      mx = fmaxf(mx, best);
    }
    float den = 0.f;
    for (int r = 0; r < R; ++r) { smax[r] = expf(smax[r] - mx); den += smax[r]; }
    float f = 0.f;
    for (int r = 0; r < R; ++r) {
      const int src = b - R / 2 + r;
      float w = smax[r] / den;
      if (src < 0 || src >= n) w = 0.f;                                    // zeroed after the softmax (:266-269)
      f += w * refer[r];
    }
    fused[(size_t)b * K + c] = f;
  }
}

__global__ void bank_argmax_kernel(const float* __restrict__ fused, int B, int K, int64_t* __restrict__ best) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float v = fused[(size_t)b * K]; int arg = 0;
  for (int i = 1; i < K; ++i) if (fused[(size_t)b * K + i] > v) { v = fused[(size_t)b * K + i]; arg = i; }
  best[b] = arg;
}

}  // namespace

extern "C" int dcn_bank_write(const float* x, int ldx, float* bank, float* split, int64_t rows, int c, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DCN_CHECK_ARG(x && bank && split && rows > 0 && c > 0 && c % 8 == 0 && c <= 1024, "bank_write: bad argument (rows=%lld c=%d: c a multiple of 8, <= 1024)",
                (long long)rows, c);
  if (ldx <= 0) ldx = c;
  DCN_CHECK_ARG(ldx % 4 == 0 && ldx >= c && rows <= (int64_t)4 * 0x7FFFFFFF, "bank_write: ldx=%d", ldx);
  DCN_CHECK_ARG(((((uintptr_t)x | (uintptr_t)bank | (uintptr_t)split)) & 15) == 0, "bank_write: 16-byte aligned tensors");
  // (no profiling tag of its own: a tag belongs to one kernel file and is named by the benchmark driver)
  const dim3 grid(cdiv(rows, 4));
  if (c <= 256) hipLaunchKernelGGL(bank_write_kernel<1>, grid, dim3(256), 0, stream, x, ldx, bank, split, rows, c);
  else if (c <= 512) hipLaunchKernelGGL(bank_write_kernel<2>, grid, dim3(256), 0, stream, x, ldx, bank, split, rows, c);
  else hipLaunchKernelGGL(bank_write_kernel<4>, grid, dim3(256), 0, stream, x, ldx, bank, split, rows, c);
  DCN_CHECK_LAUNCH("bank_write");
  return DCN_OK;
}

extern "C" int dcn_bank_write_b16(const float* x, int ldx, void* rows16, float* bank, float* split, int64_t rows, int c, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DCN_CHECK_ARG(x && rows16 && rows > 0 && c > 0 && c % 8 == 0 && c <= 1024,
                "bank_write_b16: bad argument (rows=%lld c=%d: c a multiple of 8, <= 1024; x and rows16 required)", (long long)rows, c);
  if (ldx <= 0) ldx = c;
  DCN_CHECK_ARG(ldx % 4 == 0 && ldx >= c && rows <= (int64_t)4 * 0x7FFFFFFF, "bank_write_b16: ldx=%d", ldx);
  DCN_CHECK_ARG(((((uintptr_t)x | (uintptr_t)rows16 | (uintptr_t)bank | (uintptr_t)split)) & 15) == 0, "bank_write_b16: 16-byte aligned tensors");
  const dim3 grid(cdiv(rows, 4));
  __bf16* r16 = (__bf16*)rows16;
  if (c <= 256) hipLaunchKernelGGL(bank_write_b16_kernel<1>, grid, dim3(256), 0, stream, x, ldx, r16, bank, split, rows, c);
  else if (c <= 512) hipLaunchKernelGGL(bank_write_b16_kernel<2>, grid, dim3(256), 0, stream, x, ldx, r16, bank, split, rows, c);
  else hipLaunchKernelGGL(bank_write_b16_kernel<4>, grid, dim3(256), 0, stream, x, ldx, r16, bank, split, rows, c);
  DCN_CHECK_LAUNCH("bank_write_b16");
  return DCN_OK;
}

extern "C" int dcn_bank_concat_b16(const void* rows16, int64_t bs16, const float* attn, int ld_attn, int64_t bs_attn, void* cat, int n, int hw,
                                   int c, void* stream_) {
  DCN_CHECK_ARG(rows16 && attn && cat && n > 0 && hw > 0 && c > 0 && c % 8 == 0, "bank_concat_b16: bad argument (n=%d hw=%d c=%d: c a multiple of 8)",
                n, hw, c);
  if (bs16 <= 0) bs16 = (int64_t)hw * c;
  if (ld_attn <= 0) ld_attn = c;
  if (bs_attn <= 0) bs_attn = (int64_t)hw * ld_attn;
  DCN_CHECK_ARG(bs16 % 8 == 0 && bs16 >= (int64_t)hw * c && ld_attn % 4 == 0 && ld_attn >= c && bs_attn % 4 == 0 &&
                bs_attn >= (int64_t)(hw - 1) * ld_attn + c, "bank_concat_b16: strides (bs16=%lld ld_attn=%d bs_attn=%lld)", (long long)bs16, ld_attn,
                (long long)bs_attn);
  DCN_CHECK_ARG(((((uintptr_t)rows16 | (uintptr_t)attn | (uintptr_t)cat)) & 15) == 0, "bank_concat_b16: 16-byte aligned tensors");
  const int64_t total = (int64_t)n * hw * (c / 4);                     // 16-byte groups of cat
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(bank_concat_b16_kernel, dim3((int)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream_,
                     (const __bf16*)rows16, bs16, attn, ld_attn, bs_attn, (__bf16*)cat, hw, c, total);
  DCN_CHECK_LAUNCH("bank_concat_b16");
  return DCN_OK;
}

// which operands dcn_coattn_bank_fwd reads for an (hw, c) problem: the helper its own switch calls (batch does not enter above 0)
extern "C" int dcn_coattn_bank_form(int hw, int c) { return coattn_on_gemm3(1, hw, c) ? 1 : 0; }

extern "C" int dcn_coattn_bank_fwd(const float* f1, const float* f2, const float* f1s, const float* f2s, int64_t bsf,
                                   float* f1_attn, float* f2_attn, int ldo, int64_t bso, float* E, float* rinv, float* cinv, float* ws,
                                   int b, int hw, int c, float temperature, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DCN_CHECK_ARG(f1 && f2 && f1s && f2s && (f1_attn || f2_attn) && E && rinv && cinv && ws, "coattn_bank_fwd: null pointer");
  DCN_CHECK_ARG(b > 0 && hw > 0 && c > 0 && c % 32 == 0, "coattn_bank_fwd: bad shape (c=%d must be a multiple of 32)", c);
  if (bsf <= 0) bsf = (int64_t)hw * c;
  if (ldo <= 0) ldo = c;
  if (bso <= 0) bso = (int64_t)hw * ldo;
  DCN_CHECK_ARG(bsf % 4 == 0 && bsf >= (int64_t)hw * c && ldo % 4 == 0 && ldo >= c && bso % 4 == 0, "coattn_bank_fwd: strides (bsf=%lld ldo=%d bso=%lld)",
                (long long)bsf, ldo, (long long)bso);
  if (!f1_attn) {                 // only the second direction: the same problem with the operands exchanged (A -> A^T)
    const float* t_ = f1; f1 = f2; f2 = t_;
    t_ = f1s; f1s = f2s; f2s = t_;
    f1_attn = f2_attn; f2_attn = nullptr;
  }
  // dcn_coattn_fwd's sequence on operands that need no pre-split: the path that runs reads its own form of the bank
  unsigned* one = coattn_ws_amax(ws, b, hw);       // word 0: the constant 1 (unit-norm rows, E <= 1)
  const int rc = coattn_amax_init(one, stream);
  if (rc) return rc;
  return coattn_fwd_operands(CoOperand{f1, c, bsf, f1s, c, bsf, one}, CoOperand{f2, c, bsf, f2s, c, bsf, one}, f1_attn, f2_attn, ldo, bso,
                             E, rinv, cinv, ws, b, hw, c, temperature, stream);
}

extern "C" int dcn_post_fusion_bank(const float* feats, const float* scores, int n, int k, int r, int e, float* fused, int64_t* best,
                                    void* stream) {
  DCN_CHECK_ARG(feats && scores && fused && best && n > 0 && k > 0 && k <= VF_MAXK && r > 0 && r <= VF_MAXR && e > 0,
                "post_fusion_bank: bad argument (n=%d k=%d r=%d e=%d; k <= %d, r <= %d)", n, k, r, e, VF_MAXK, VF_MAXR);
  hipLaunchKernelGGL(post_fusion_bank_kernel, dim3(k, n), dim3(256), 0, (hipStream_t)stream, feats, scores, n, k, r, e, fused);
  DCN_CHECK_LAUNCH("post_fusion_bank");
  hipLaunchKernelGGL(bank_argmax_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, fused, n, k, best);
  DCN_CHECK_LAUNCH("post_argmax");
  return DCN_OK;
}
