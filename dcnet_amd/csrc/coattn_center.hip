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
// This file is host code only: the products go through coattn.hip's product path (CoProducts: the engine chosen once by
// coattn_on_gemm3(b, hw, c), the same in both directions), the streaming passes are coattn.hip's kernels in their row-only forms
// (exp_sums_kernel / dA_kernel with COLS = false) behind its launchers, and all of them are timed there (tags 12, 31, 40).
#include "igemm.h"
#include "coattn.h"

namespace {

// Abs-max words (DCN_AMAX_WORDS each, in the caller's workspace), one set per neighbour so that a neighbour's operands are scaled by
// their own maxima: slot 0 holds the constant 1 (unit-norm features, E <= 1), the others start at 0 (coattn_amax_init_sets).
enum { AM_ONE = 0, AM_DO, AM_DOS, AM_DP, AM_DA, AM_SLOTS };

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
  const int ldE = coattn_ld_pad(hw), nn = t - 1;
  const long long bsE = (long long)hw * ldE, bsf = (long long)t * hw * c, frame = (long long)hw * c;
  const CoProducts P(b, hw, c, stream);
  unsigned* am = reinterpret_cast<unsigned*>(ws);
  if ((rc = coattn_amax_init_sets(am, 1, AM_SLOTS, stream))) return rc;
  const unsigned* one = am + AM_ONE * DCN_AMAX_WORDS;
  float* clips_s = E + dcn_coattn_e_size(b * nn, hw);          // (gemm3.hip: the split form of every frame, kept for the backward)
  auto frame_op = [&](int f) { return CoOperand{clips + f * frame, c, bsf, clips_s + f * frame, c, bsf, one}; };
  // 1. A_j = f_ctr . f_j^T -> E_j                                          (NT)
  if (P.g3 && (rc = gemm3_presplit(clips, c, frame, clips_s, c, frame, b * t, hw, c, one, stream))) return rc;
  for (int n = 0; n < nn; ++n)
    if ((rc = P.nt(frame_op(ctr), frame_op(frame_of(n, ctr)), E + (int64_t)n * b * bsE, ldE, bsE, nullptr, 0))) return rc;
  // 2. E = exp(t*A - t) (gemm3.hip: in split form), rinv = 1 / row sums: every neighbour in one launch
  if ((rc = coattn_exp_sums(E, b * nn, hw, temperature, rinv, nullptr, nullptr, P.g3, stream))) return rc;
  // 3. attn_j = diag(rinv_j) E_j f_j                                       (NN, K = keys)
  for (int n = 0; n < nn; ++n) {
    const CoOperand En = co_buffer(E + (int64_t)n * b * bsE, ldE, bsE, one);
    if ((rc = P.nn(En, frame_op(frame_of(n, ctr)), attn + n * nso, ldo, bso, rinv + (int64_t)n * b * hw, 0))) return rc;
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
  const CoProducts P(b, hw, c, stream);
  float* dP = ws;
  float* dOs = dP + rows * ldE;
  float* del = dOs + rows * c;
  unsigned* am = reinterpret_cast<unsigned*>(del + rows);
  float* dOp = reinterpret_cast<float*>(((uintptr_t)(am + (size_t)nn * AM_SLOTS * DCN_AMAX_WORDS) + 15) & ~(uintptr_t)15);      // (b * hw may be odd)
  if ((rc = coattn_amax_init_sets(am, nn, AM_SLOTS, stream))) return rc;
  const float* clips_s = E + dcn_coattn_e_size(b * nn, hw);    // the forward's split form of every frame (unit norm: the constant abs-max word)
  for (int n = 0; n < nn; ++n) {
    const long long fj = frame_of(n, ctr) * frame, fc = ctr * frame;
    const float* rn = rinv + (int64_t)n * rows;
    const float* dO = d_attn + n * nsdo;
    unsigned* amn = am + (size_t)n * AM_SLOTS * DCN_AMAX_WORDS;
    auto slot = [&](int i) { return amn + i * DCN_AMAX_WORDS; };
    const CoOperand Fj{clips + fj, c, bsf, clips_s + fj, c, bsf, slot(AM_ONE)}, Fc{clips + fc, c, bsf, clips_s + fc, c, bsf, slot(AM_ONE)};
    const CoOperand DO{dO, lddo, bsdo, dOp, c, frame, slot(AM_DO)}, DOS = co_buffer(dOs, c, frame, slot(AM_DOS));
    const CoOperand En = co_buffer(E + (int64_t)n * b * bsE, ldE, bsE, slot(AM_ONE)), DA = co_buffer(dP, ldE, bsE, slot(AM_DA));
    // 1. del and the pre-scaled upstream gradient
    if ((rc = coattn_rowdot_scale(dO, lddo, bsdo, attn + n * nso, ldo, bso, rn, b, hw, c, del, dOs, slot(AM_DO), slot(AM_DOS), stream))) return rc;
    if (P.g3) {      // the two narrow gradient operands are split once each, the scaled one in place
      if ((rc = gemm3_presplit(dO, lddo, bsdo, dOp, c, frame, b, hw, c, slot(AM_DO), stream))) return rc;
      if ((rc = gemm3_presplit(dOs, c, frame, dOs, c, frame, b, hw, c, slot(AM_DOS), stream))) return rc;
    }
    // 2. dP[i,k] = <dO_i, f_j[k]>                                           (NT)
    if ((rc = P.nt(DO, Fj, dP, ldE, bsE, nullptr, 0, slot(AM_DP)))) return rc;
    // 3. dA over dP (pads -> 0).  gemm3.hip: in split form straight away, scaled by a bound from the maximum the product left
    if (P.g3 && (rc = coattn_da_bound(slot(AM_DP), nullptr, temperature, slot(AM_DA), stream))) return rc;
    if ((rc = coattn_dA(En.f, dP, nullptr, rn, nullptr, del, nullptr, b, hw, temperature, slot(AM_DA), P.g3, stream))) return rc;
    // 4. d_f_ctr (+)= dA f_j                                                (NN)
    if ((rc = P.nn(DA, Fj, d_clips + fc, c, bsf, nullptr, (n > 0 || accumulate) ? 1 : 0))) return rc;
    // 5. d_f_j = dA^T f_ctr + E^T (dO * rinv)                               (TN x2)
    if ((rc = P.tn(DA, Fc, d_clips + fj, c, bsf, nullptr, 0))) return rc;
    if ((rc = P.tn(En, DOS, d_clips + fj, c, bsf, nullptr, 1))) return rc;
  }
  return DCN_OK;
}
