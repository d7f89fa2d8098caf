// Centre-versus-neighbours co-attention of a window of frames (model/test_DCNet_model.py:259-274; its train branch :480-483).
//
//   clips [b][t][hw][c], unit norm over c; ctr = the centre frame; j = every other frame, ascending
//   A_j       = f_ctr . f_j^T
//   attn_j[i] = sum_k softmax_k(temp * A_j[i,k]) f_j[k]          — only the centre attends: ONE softmax direction
//
// The pair node (coattn.hip) needs both directions of one affinity and therefore row AND column sums, two dP products and two
// gradients per operand.  Here every affinity is used along its rows only: E_j = exp(temp*A_j - temp) and rinv_j = 1/rowsum(E_j) are all
// the forward keeps, and the backward is
//   del_j[i]  = <d_attn_j[i], attn_j[i]>                         (= the softmax-weighted mean of row i of dP_j)
//   dP_j      = d_attn_j . f_j^T                                 (NT)
//   dA_j      = temp * E_j * rinv_j[i] * (dP_j - del_j[i])       (over dP_j; pad columns -> 0)
//   d_f_ctr  += dA_j . f_j                                       (NN; the centre's rows collect every neighbour)
//   d_f_j     = dA_j^T . f_ctr + E_j^T . (rinv_j * d_attn_j)     (TN x2; each neighbour's rows belong to one j alone)
// — four products per neighbour where the pair kernels with a zero gradient for the unused f2_attn ran six, and one hw x ld buffer
// where they needed two.  The neighbours run as a host loop inside the entry points: a batched launch would need a second batch stride
// in every engine, and a product of one neighbour (b clips) already fills the machine at the shapes that matter.  What IS shared across
// the loop: the split form of clips (made once by the forward: t frames per clip, the centre once), the abs-max words, the dP buffer.
// The products run on the engines of coattn.hip, chosen by coattn_on_gemm3(b, hw, c) in both directions, and are timed there; the two
// streaming passes of this file carry no profiling tag (a tag belongs to one file, and the flagship workload never runs these).
#include "igemm.h"
#include "coattn.h"

int tn_gemm_batched(const float* A, int lda, long long a_bs, const float* B, int ldb, long long b_bs,
                    float* C, int ldc, long long c_bs, const float* row_scale,
                    int M, int m_ld, int N, int K, int batch, int accumulate, hipStream_t stream,
                    const unsigned* amax_a = nullptr, const unsigned* amax_b = nullptr);

namespace {

constexpr int EXP_ROWS = 32;
typedef _Float16 f16x4c_t __attribute__((ext_vector_type(4)));
constexpr float E_SPLIT_SCALE = 8192.f;           // brings 1.0 below 2^14 (the scale gemm3.hip derives from the constant abs-max word 1)

// E = exp(t*A - t) in place (pad columns -> 0) and rinv = 1 / row sums: the row-only form of coattn.hip's exp_sums_kernel (no column
// partials: nothing attends along the columns).  grid (ceil(hw/32), problems); each thread owns four consecutive columns (16-byte
// accesses) 4*tid, 4*tid + 1024, ... and walks the 32 rows.  SPLIT: E is written in the f16 two-piece form gemm3.hip reads ([8 h | 8 l]
// per 8 columns): a thread's four columns are half of such a run; the sums are those of the fp32 values.
template <bool SPLIT>
__global__ __launch_bounds__(256) void exp_rows_kernel(float* __restrict__ E, int hw, int ldE, float t, float* __restrict__ rinv) {
  __shared__ float red[4][EXP_ROWS];
  const int b = blockIdx.y, i0 = blockIdx.x * EXP_ROWS;
  float* e = E + ((size_t)b * hw + i0) * ldE;
  float racc[EXP_ROWS];
#pragma unroll
  for (int r = 0; r < EXP_ROWS; ++r) racc[r] = 0.f;
  const int nrow = min(EXP_ROWS, hw - i0);
  for (int j = threadIdx.x * 4; j < ldE; j += 1024) {
    f32x4 v[EXP_ROWS];
#pragma unroll
    for (int r = 0; r < EXP_ROWS; ++r)
      v[r] = r < nrow ? *reinterpret_cast<const f32x4*>(e + (size_t)r * ldE + j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < EXP_ROWS; ++r) {
      if (r < nrow) {
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (j + k < hw) ? expf(t * v[r][k] - t) : 0.f;
        if constexpr (SPLIT) {
          const f32x4 ts = o * E_SPLIT_SCALE;
          const f16x4c_t h = {(_Float16)ts[0], (_Float16)ts[1], (_Float16)ts[2], (_Float16)ts[3]};
          const f16x4c_t l = {(_Float16)(ts[0] - (float)h[0]), (_Float16)(ts[1] - (float)h[1]), (_Float16)(ts[2] - (float)h[2]),
                              (_Float16)(ts[3] - (float)h[3])};
          unsigned char* run = reinterpret_cast<unsigned char*>(e + (size_t)r * ldE + (j & ~7)) + (j & 4) * 2;
          *reinterpret_cast<f16x4c_t*>(run) = h;
          *reinterpret_cast<f16x4c_t*>(run + 16) = l;
        } else {
          *reinterpret_cast<f32x4*>(e + (size_t)r * ldE + j) = o;
        }
        racc[r] += (o[0] + o[1]) + (o[2] + o[3]);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < EXP_ROWS; ++r) {
    const float s = wave_sum(racc[r]);
    if (lane == 0) red[wave][r] = s;
  }
  __syncthreads();
  if (threadIdx.x < EXP_ROWS && i0 + threadIdx.x < hw)
    rinv[(size_t)b * hw + i0 + threadIdx.x] = 1.f / (red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// Abs-max words (DCN_AMAX_WORDS each, in the caller's workspace), one set per neighbour so that a neighbour's operands are scaled by
// their own maxima: slot 0 holds the constant 1 (unit-norm features, E <= 1), the others start at 0.
enum { AM_ONE = 0, AM_DO, AM_DOS, AM_DP, AM_DA, AM_SLOTS };
__global__ __launch_bounds__(256) void amax_init_kernel(unsigned* __restrict__ w, int total) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256)
    w[i] = (i % (AM_SLOTS * DCN_AMAX_WORDS)) < DCN_AMAX_WORDS ? 0x3F800000u : 0u;
}

// one wave per row: del[row] = <d[row], o[row]>, ds[row] = d[row] * rinv[row]; abs-max of d and ds
__global__ __launch_bounds__(256) void rowdot_scale_kernel(const float* __restrict__ d, int ldd, int64_t bsd,
                                                           const float* __restrict__ o, int ldo, int64_t bso, int hw,
                                                           const float* __restrict__ inv, int64_t rows, int c,
                                                           float* __restrict__ del, float* __restrict__ ds,
                                                           unsigned* __restrict__ amax_d, unsigned* __restrict__ amax_ds) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  float vmax = 0.f, s = 0.f;
  if (row < rows) {
    const int64_t bb = row / hw, i = row - bb * hw;
    s = inv[row];
    float acc = 0.f;
    for (int k = lane * 4; k < c; k += 256) {
      const f32x4 dv = *reinterpret_cast<const f32x4*>(d + bb * bsd + i * ldd + k);
      const f32x4 ov = *reinterpret_cast<const f32x4*>(o + bb * bso + i * ldo + k);
      acc += dv[0] * ov[0] + dv[1] * ov[1] + dv[2] * ov[2] + dv[3] * ov[3];
      *reinterpret_cast<f32x4*>(ds + row * c + k) = dv * s;
      vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(dv[0]), fabsf(dv[1]))), fmaxf(fabsf(dv[2]), fabsf(dv[3])));
    }
    acc = wave_sum(acc);
    if (lane == 0) del[row] = acc;
  }
  // (s > 0: the scaled tensor's maximum is bounded by max|d| * s over the block's rows)
  const float vs = wave_max(vmax * s);
  amax_update_block(amax_d, vmax, red);
  __syncthreads();
  amax_update_block(amax_ds, vs, red);
}

// dA = t * E * rinv[i] * (dP - del[i]), written over dP; pad columns -> 0.  The row-only form of coattn.hip's dA_kernel: one product
// buffer, no column terms.  Four consecutive columns (16 bytes) per lane and step.
// ESPLIT: E is read from the split form.  OSPLIT: dA is written in the split form as well, scaled by the word in amax_da, which then
// holds a BOUND (da_bound_kernel) instead of receiving the maximum.
template <bool ESPLIT, bool OSPLIT>
__global__ __launch_bounds__(256) void dA_rows_kernel(const float* __restrict__ E, float* __restrict__ dP, const float* __restrict__ rinv,
                                                      const float* __restrict__ del, int hw, int ldE, float t, int64_t total4,
                                                      unsigned* __restrict__ amax_da) {
  __shared__ float red[4];
  float vmax = 0.f;
  const int l4 = ldE >> 2;
  float s_out = 1.f;
  if constexpr (OSPLIT) {                         // (= gemm3.hip's power-of-two scale of the bound)
    const int be = (int)((amax_read(amax_da) >> 23) & 0xFF);
    int ex = (be == 0 || be == 255) ? 0 : 14 - (be - 126);
    ex = ex > 100 ? 100 : (ex < -100 ? -100 : ex);
    s_out = __uint_as_float((unsigned)(ex + 127) << 23);
  }
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / l4;                 // = clip * hw + i
    const int j = (int)(idx - row * l4) * 4;
    f32x4 e;
    if constexpr (ESPLIT) {                       // h + l of the split form: E to 22 bits
      const unsigned char* run = reinterpret_cast<const unsigned char*>(E + row * ldE + (j & ~7)) + (j & 4) * 2;
      const f16x4c_t h = *reinterpret_cast<const f16x4c_t*>(run), l = *reinterpret_cast<const f16x4c_t*>(run + 16);
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = ((float)h[k] + (float)l[k]) * (1.f / E_SPLIT_SCALE);
    } else {
      e = *reinterpret_cast<const f32x4*>(E + row * ldE + j);
    }
    const f32x4 p = *reinterpret_cast<const f32x4*>(dP + row * ldE + j);
    const float tr = t * rinv[row], di = del[row];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (j + k < hw) ? tr * e[k] * (p[k] - di) : 0.f;
    if constexpr (OSPLIT) {                       // (a lane pair shares a run of 8 columns: both have read their 16 bytes by now)
      const f32x4 ts = o * s_out;
      const f16x4c_t h = {(_Float16)ts[0], (_Float16)ts[1], (_Float16)ts[2], (_Float16)ts[3]};
      const f16x4c_t l = {(_Float16)(ts[0] - (float)h[0]), (_Float16)(ts[1] - (float)h[1]), (_Float16)(ts[2] - (float)h[2]),
                          (_Float16)(ts[3] - (float)h[3])};
      unsigned char* run = reinterpret_cast<unsigned char*>(dP + row * ldE + (j & ~7)) + (j & 4) * 2;
      *reinterpret_cast<f16x4c_t*>(run) = h;
      *reinterpret_cast<f16x4c_t*>(run + 16) = l;
    } else {
      *reinterpret_cast<f32x4*>(dP + row * ldE + j) = o;
      vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(o[0]), fabsf(o[1]))), fmaxf(fabsf(o[2]), fabsf(o[3])));
    }
  }
  if constexpr (!OSPLIT) amax_update_block(amax_da, vmax, red);
}

// |dA_ik| = t E_ik r_i |dP_ik - del_i| <= 2 t max|dP|: E_ik r_i <= 1 (an entry is one term of its row sum) and del_i is the
// softmax-weighted mean of row i of dP.  The f16 split needs a bound, not the maximum, so dA_rows_kernel writes the split form directly.
__global__ __launch_bounds__(64) void da_bound_kernel(const unsigned* __restrict__ a, float t, unsigned* __restrict__ out) {
  const float b = 2.f * t * __uint_as_float(amax_read(a));
  out[threadIdx.x & (DCN_AMAX_WORDS - 1)] = __float_as_uint(b);
}

void gemm_params(IgemmParams& p, const float* A, int lda, long long a_bs, const float* B, int ldb, long long b_bs,
                 float* C, int ldc, long long c_bs, int M, int N, int K, int batch) {
  p = IgemmParams{};
  p.osy = p.osx = p.isy = p.isx = 1; p.dense_out = 1;
  p.in = A; p.ldi = lda; p.in_bs = a_bs; p.wt = B; p.ldw = ldb; p.wt_bs = b_bs; p.out = C; p.ldo = ldc; p.out_bs = c_bs;
  p.ldr = ldc;
  p.N = 1; p.Hi = 1; p.Wi = M; p.Ho = 1; p.Wo = M; p.Hs = 1; p.Ws = M; p.M = M;
  p.Ci = K; p.Co = N; p.ntaps = 1; p.batch = batch;
}

int amax_init(unsigned* am, int sets, hipStream_t stream) {
  const int total = sets * AM_SLOTS * DCN_AMAX_WORDS;
  hipLaunchKernelGGL(amax_init_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, am, total);
  DCN_CHECK_LAUNCH("coattn_center amax_init");
  return DCN_OK;
}

// the frame of neighbour n (frames != ctr, ascending)
inline int frame_of(int n, int ctr) { return n < ctr ? n : n + 1; }

int check_shape(const char* who, int b, int t, int hw, int c, int ctr) {
  DCN_CHECK_ARG(b > 0 && hw > 0 && c > 0 && c % 32 == 0, "%s: bad shape (b=%d hw=%d; c=%d must be a multiple of 32)", who, b, hw, c);
  DCN_CHECK_ARG(t >= 2, "%s: a window needs t >= 2 frames (t=%d)", who, t);
  DCN_CHECK_ARG(ctr >= 0 && ctr < t, "%s: ctr=%d out of range [0, %d)", who, ctr, t);
  return DCN_OK;
}

}  // namespace

extern "C" int64_t dcn_coattn_center_saved_size(int b, int t, int hw, int c) {
  if (b <= 0 || t < 2 || hw <= 0 || c <= 0) return 0;
  return dcn_coattn_e_size(b * (t - 1), hw) + (coattn_on_gemm3(b, hw, c) ? (int64_t)b * t * hw * c : 0);
}
extern "C" int64_t dcn_coattn_center_fwd_ws(int b, int t, int hw, int c) {
  (void)b; (void)t; (void)hw; (void)c;
  return AM_SLOTS * DCN_AMAX_WORDS;
}

extern "C" int dcn_coattn_center_fwd(const float* clips, float* attn, int ldo, int64_t bso, int64_t nso, float* E, float* rinv, float* ws,
                                     int b, int t, int hw, int c, int ctr, float temperature, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DCN_CHECK_ARG(clips && attn && E && rinv && ws, "coattn_center_fwd: null pointer");
  int rc = check_shape("coattn_center_fwd", b, t, hw, c, ctr);
  if (rc) return rc;
  if (ldo <= 0) ldo = c;
  if (bso <= 0) bso = (int64_t)hw * ldo;
  if (nso <= 0) nso = (int64_t)b * bso;
  DCN_CHECK_ARG(ldo >= c && ldo % 4 == 0 && bso % 4 == 0 && nso % 4 == 0 && ((uintptr_t)attn & 15) == 0 && ((uintptr_t)clips & 15) == 0,
                "coattn_center_fwd: ldo >= c; ldo, the strides (floats) multiples of 4; 16-byte aligned tensors");
  const int ldE = coattn_ld_pad(hw), nn = t - 1, nrb = cdiv(hw, EXP_ROWS);
  const long long bsE = (long long)hw * ldE, bsf = (long long)t * hw * c, frame = (long long)hw * c;
  const bool g3 = coattn_on_gemm3(b, hw, c);
  unsigned* am = reinterpret_cast<unsigned*>(ws);
  if ((rc = amax_init(am, 1, stream))) return rc;
  const unsigned* one = am + AM_ONE * DCN_AMAX_WORDS;
  float* clips_s = E + dcn_coattn_e_size(b * nn, hw);          // (gemm3.hip: the split form of every frame, kept for the backward)
  IgemmParams p;
  // 1. A_j = f_ctr . f_j^T -> E_j                                          (NT)
  if (g3 && (rc = gemm3_presplit(clips, c, frame, clips_s, c, frame, b * t, hw, c, one, stream))) return rc;
  for (int n = 0; n < nn; ++n) {
    const long long fj = frame_of(n, ctr) * frame;
    float* En = E + (int64_t)n * b * bsE;
    if (g3) {
      rc = gemm3_launch(clips_s + ctr * frame, c, bsf, 0, clips_s + fj, c, bsf, 0, En, ldE, bsE, nullptr, 0, hw, hw, c, b, 0, one, one, stream);
    } else {
      gemm_params(p, clips + ctr * frame, c, bsf, clips + fj, c, bsf, En, ldE, bsE, hw, hw, c, b);
      p.amax_a = one; p.amax_b = one;
      rc = igemm_launch(p, stream);
    }
    if (rc) return rc;
  }
  // 2. E = exp(t*A - t) (gemm3.hip: in split form), rinv = 1 / row sums: every neighbour in one launch
  if (g3) hipLaunchKernelGGL(exp_rows_kernel<true>, dim3(nrb, b * nn), dim3(256), 0, stream, E, hw, ldE, temperature, rinv);
  else hipLaunchKernelGGL(exp_rows_kernel<false>, dim3(nrb, b * nn), dim3(256), 0, stream, E, hw, ldE, temperature, rinv);
  DCN_CHECK_LAUNCH("exp_rows");
  // 3. attn_j = diag(rinv_j) E_j f_j                                       (NN, K = keys)
  for (int n = 0; n < nn; ++n) {
    const long long fj = frame_of(n, ctr) * frame;
    float* En = E + (int64_t)n * b * bsE;
    const float* rn = rinv + (int64_t)n * b * hw;
    float* out = attn + n * nso;
    if (g3) {
      rc = gemm3_launch(En, ldE, bsE, 0, clips_s + fj, c, bsf, 1, out, ldo, bso, rn, hw, hw, c, hw, b, 0, one, one, stream);
    } else {
      gemm_params(p, En, ldE, bsE, clips + fj, c, bsf, out, ldo, bso, hw, c, ldE, b);
      p.bmode = 1; p.kvalid = hw; p.row_scale = rn; p.amax_a = one; p.amax_b = one;
      rc = igemm_launch(p, stream);
    }
    if (rc) return rc;
  }
  return DCN_OK;
}

// ws: dP [b][hw][ldE] | dOs [b][hw][c] | del [b][hw] | abs-max words of t-1 neighbours | (gemm3.hip) the split d_attn [b][hw][c], 16-byte aligned
extern "C" int64_t dcn_coattn_center_bwd_ws(int b, int t, int hw, int c) {
  if (b <= 0 || t < 2 || hw <= 0 || c <= 0) return 0;
  const int64_t rows = (int64_t)b * hw;
  return rows * coattn_ld_pad(hw) + rows * c + rows + (int64_t)(t - 1) * AM_SLOTS * DCN_AMAX_WORDS + (coattn_on_gemm3(b, hw, c) ? rows * c + 4 : 0);
}

extern "C" int dcn_coattn_center_bwd(const float* clips, const float* d_attn, int lddo, int64_t bsdo, int64_t nsdo,
                                     const float* attn, int ldo, int64_t bso, int64_t nso, const float* E, const float* rinv,
                                     float* d_clips, int accumulate, float* ws,
                                     int b, int t, int hw, int c, int ctr, float temperature, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DCN_CHECK_ARG(clips && d_attn && attn && E && rinv && d_clips && ws, "coattn_center_bwd: null pointer");
  int rc = check_shape("coattn_center_bwd", b, t, hw, c, ctr);
  if (rc) return rc;
  if (ldo <= 0) ldo = c;
  if (lddo <= 0) lddo = c;
  if (bso <= 0) bso = (int64_t)hw * ldo;
  if (bsdo <= 0) bsdo = (int64_t)hw * lddo;
  if (nso <= 0) nso = (int64_t)b * bso;
  if (nsdo <= 0) nsdo = (int64_t)b * bsdo;
  DCN_CHECK_ARG(ldo >= c && lddo >= c && ldo % 4 == 0 && lddo % 4 == 0 && bso % 4 == 0 && bsdo % 4 == 0 && nso % 4 == 0 && nsdo % 4 == 0 &&
                    (((uintptr_t)attn | (uintptr_t)d_attn | (uintptr_t)clips | (uintptr_t)d_clips | (uintptr_t)ws) & 15) == 0,
                "coattn_center_bwd: ldo, lddo >= c; row / batch / neighbour strides (floats) multiples of 4; 16-byte aligned tensors");
  const int ldE = coattn_ld_pad(hw), nn = t - 1;
  const long long rows = (long long)b * hw;
  const long long bsE = (long long)hw * ldE, bsf = (long long)t * hw * c, frame = (long long)hw * c;
  const bool g3 = coattn_on_gemm3(b, hw, c);
  float* dP = ws;
  float* dOs = dP + rows * ldE;
  float* del = dOs + rows * c;
  unsigned* am = reinterpret_cast<unsigned*>(del + rows);
  float* dOp = reinterpret_cast<float*>(((uintptr_t)(am + (size_t)nn * AM_SLOTS * DCN_AMAX_WORDS) + 15) & ~(uintptr_t)15);      // (b * hw may be odd)
  if ((rc = amax_init(am, nn, stream))) return rc;
  const float* clips_s = E + dcn_coattn_e_size(b * nn, hw);    // the forward's split form of every frame (unit norm: the constant abs-max word)
  const int64_t total4 = rows * (ldE / 4);
  int64_t g = (total4 + 255) / 256; if (g > 1024) g = 1024;    // (one abs-max atomic per workgroup)
  IgemmParams p;
  for (int n = 0; n < nn; ++n) {
    const int j = frame_of(n, ctr);
    const long long fj = j * frame, fc = ctr * frame;
    const float* En = E + (int64_t)n * b * bsE;
    const float* rn = rinv + (int64_t)n * rows;
    const float* dO = d_attn + n * nsdo;
    unsigned* amn = am + (size_t)n * AM_SLOTS * DCN_AMAX_WORDS;
    auto slot = [&](int i) { return amn + i * DCN_AMAX_WORDS; };
    const int acc_ctr = (n > 0 || accumulate) ? 1 : 0;
    // 1. del and the pre-scaled upstream gradient
    hipLaunchKernelGGL(rowdot_scale_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, dO, lddo, bsdo, attn + n * nso, ldo, bso, hw, rn, (int64_t)rows, c,
                       del, dOs, slot(AM_DO), slot(AM_DOS));
    DCN_CHECK_LAUNCH("coattn_center rowdot_scale");
    if (g3) {
      if ((rc = gemm3_presplit(dO, lddo, bsdo, dOp, c, frame, b, hw, c, slot(AM_DO), stream))) return rc;
      if ((rc = gemm3_presplit(dOs, c, frame, dOs, c, frame, b, hw, c, slot(AM_DOS), stream))) return rc;
      // 2. dP[i,k] = <dO_i, f_j[k]>                                         (NT)
      if ((rc = gemm3_launch(dOp, c, frame, 0, clips_s + fj, c, bsf, 0, dP, ldE, bsE, nullptr, 0, hw, hw, c, b, 0, slot(AM_DO), slot(AM_ONE), stream, slot(AM_DP)))) return rc;
      // 3. dA over dP (pads -> 0), in split form straight away, scaled by a bound from the maximum the product left
      hipLaunchKernelGGL(da_bound_kernel, dim3(1), dim3(64), 0, stream, slot(AM_DP), temperature, slot(AM_DA));
      DCN_CHECK_LAUNCH("coattn_center dA bound");
      hipLaunchKernelGGL((dA_rows_kernel<true, true>), dim3((int)g), dim3(256), 0, stream, En, dP, rn, del, hw, ldE, temperature, total4, slot(AM_DA));
      DCN_CHECK_LAUNCH("coattn_center dA");
      // 4. d_f_ctr (+)= dA f_j                                              (NN)
      if ((rc = gemm3_launch(dP, ldE, bsE, 0, clips_s + fj, c, bsf, 1, d_clips + fc, c, bsf, nullptr, 0, hw, c, hw, b, acc_ctr, slot(AM_DA), slot(AM_ONE), stream))) return rc;
      // 5. d_f_j = dA^T f_ctr + E^T (dO * rinv)                             (TN x2)
      if ((rc = gemm3_launch(dP, ldE, bsE, 1, clips_s + fc, c, bsf, 1, d_clips + fj, c, bsf, nullptr, 0, hw, c, hw, b, 0, slot(AM_DA), slot(AM_ONE), stream))) return rc;
      if ((rc = gemm3_launch(En, ldE, bsE, 1, dOs, c, frame, 1, d_clips + fj, c, bsf, nullptr, 0, hw, c, hw, b, 1, slot(AM_ONE), slot(AM_DOS), stream))) return rc;
      continue;
    }
    // 2. dP[i,k] = <dO_i, f_j[k]>                                           (NT)
    gemm_params(p, dO, lddo, bsdo, clips + fj, c, bsf, dP, ldE, bsE, hw, hw, c, b);
    p.amax_a = slot(AM_DO); p.amax_b = slot(AM_ONE);
    if ((rc = igemm_launch(p, stream))) return rc;
    // 3. dA over dP (pads -> 0)
    hipLaunchKernelGGL((dA_rows_kernel<false, false>), dim3((int)g), dim3(256), 0, stream, En, dP, rn, del, hw, ldE, temperature, total4, slot(AM_DA));
    DCN_CHECK_LAUNCH("coattn_center dA");
    // 4. d_f_ctr (+)= dA f_j                                                (NN)
    gemm_params(p, dP, ldE, bsE, clips + fj, c, bsf, d_clips + fc, c, bsf, hw, c, ldE, b);
    p.bmode = 1; p.kvalid = hw; p.accumulate = acc_ctr; p.amax_a = slot(AM_DA); p.amax_b = slot(AM_ONE);
    if ((rc = igemm_launch(p, stream))) return rc;
    // 5. d_f_j = dA^T f_ctr + E^T (dO * rinv)                               (TN x2)
    if ((rc = tn_gemm_batched(dP, ldE, bsE, clips + fc, c, bsf, d_clips + fj, c, bsf, nullptr, hw, ldE, c, hw, b, 0, stream, slot(AM_DA), slot(AM_ONE)))) return rc;
    if ((rc = tn_gemm_batched(En, ldE, bsE, dOs, c, frame, d_clips + fj, c, bsf, nullptr, hw, ldE, c, hw, b, 1, stream, slot(AM_ONE), slot(AM_DOS)))) return rc;
  }
  return DCN_OK;
}
