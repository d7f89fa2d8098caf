// Host-side pieces of coattn.hip that the other co-attention entry points drive on their own operands: the window of
// coattn_center.hip, the feature banks of video.hip (dcnet_amd/video.py).  One set of kernels and one product path for all three.
#pragma once
#include <hip/hip_runtime.h>

// floats of a row of E (hw padded to a multiple of 32)
int coattn_ld_pad(int hw);
// the products of a (b, hw, c) problem run on gemm3.hip?  (what dcn_coattn_fwd decides for the same shape)
bool coattn_on_gemm3(int b, int hw, int c);

// One operand of a product in the form either engine reads: the fp32 tensor (igemm.hip / wgrad.hip tiles) and its split form
// (gemm3.hip), each with row and batch stride in floats, and the abs-max word both scale by.  Only the form of the path that runs is
// read; E, dA and the scaled gradients live in ONE buffer that holds whichever form that path wrote (co_buffer).
struct CoOperand {
  const float* f; int ld; long long bs;
  const float* s; int lds; long long bss;
  const unsigned* amax;
};
inline CoOperand co_buffer(const float* p, int ld, long long bs, const unsigned* amax) { return CoOperand{p, ld, bs, p, ld, bs, amax}; }

// The three products of the co-attention of b problems of hw pixels x c channels, each sent to gemm3.hip or to the tiles of igemm.hip
// (NT, NN) / wgrad.hip (TN) by the one decision g3 = coattn_on_gemm3(b, hw, c).  C (+)= diag(row_scale) . product; row_scale [b][hw] or
// null.  amax_out (optional): abs-max word of what is stored — gemm3.hip's epilogue only, the one path with a reader (coattn_da_bound).
struct CoProducts {
  int b, hw, c; hipStream_t stream; bool g3;
  CoProducts(int b_, int hw_, int c_, hipStream_t s) : b(b_), hw(hw_), c(c_), stream(s), g3(coattn_on_gemm3(b_, hw_, c_)) {}
  // C [hw][hw] = A [hw][c] . B [hw][c]^T
  int nt(const CoOperand& A, const CoOperand& B, float* C, int ldc, long long c_bs, const float* row_scale, int accumulate,
         unsigned* amax_out = nullptr) const;
  // C [hw][c] = A [hw][hw] . B [hw][c]                 (K = the columns of A; its pad columns hold zeros)
  int nn(const CoOperand& A, const CoOperand& B, float* C, int ldc, long long c_bs, const float* row_scale, int accumulate,
         unsigned* amax_out = nullptr) const;
  // C [hw][c] = A [hw][hw]^T . B [hw][c]               (K = the rows of A)
  int tn(const CoOperand& A, const CoOperand& B, float* C, int ldc, long long c_bs, const float* row_scale, int accumulate,
         unsigned* amax_out = nullptr) const;
};

// Abs-max words (DCN_AMAX_WORDS each) in a caller's workspace, `sets` sets of `slots`: slot 0 of every set holds the constant 1
// (unit-norm features, E <= 1), the others start at 0 and are raised by the kernels that write or read the gradient operands.
int coattn_amax_init_sets(unsigned* am, int sets, int slots, hipStream_t stream);
// the one set of a dcn_coattn_fwd_ws workspace: where it lies, and its initialisation
unsigned* coattn_ws_amax(float* ws, int b, int hw);
int coattn_amax_init(unsigned* am, hipStream_t stream);
// The streaming steps (profiling tags 12 and 31), same kernels and launch shapes for pair, window and bank:
// E [nb][hw][ld_pad(hw)] holding A -> exp(t*A - t) (split: in the f16 two-piece form), rinv [nb][hw] = inverse row sums; cinv [nb][hw]
// = inverse column sums through the partials in ws (dcn_coattn_fwd_ws), or null: rows only, no ws.
int coattn_exp_sums(float* E, int nb, int hw, float temperature, float* rinv, float* cinv, float* ws, bool split, hipStream_t stream);
// delta[row] = <d[row], o[row]>, ds[row] (dense, c wide) = d[row] * inv[row]; abs-max of d and ds
int coattn_rowdot_scale(const float* d, int ldd, long long bsd, const float* o, int ldo, long long bso, const float* inv, int b, int hw,
                        int c, float* delta, float* ds, unsigned* amax_d, unsigned* amax_ds, hipStream_t stream);
// out = the bound 2 t (max a1 + max a2) on |dA| (a2 may be null), the word a split dA is scaled by
int coattn_da_bound(const unsigned* a1, const unsigned* a2, float temperature, unsigned* out, hipStream_t stream);
// dA over dP1 (pad columns -> 0).  dP2 / cinv / d2 null: the one-sided form.  split: E is read and dA written in the split form, scaled
// by the bound in amax_da; else amax_da receives the maximum.
int coattn_dA(const float* E, float* dP1, const float* dP2, const float* rinv, const float* cinv, const float* d1, const float* d2,
              int b, int hw, float temperature, unsigned* amax_da, bool split, hipStream_t stream);
// The pair forward behind its argument checks, abs-max words and pre-split: E, rinv, cinv, f1_attn and (optional) f2_attn from operands
// whose abs-max word is the constant 1 of ws (as dcn_coattn_fwd_ws, initialised by coattn_amax_init).
int coattn_fwd_operands(const CoOperand& F1, const CoOperand& F2, float* f1_attn, float* f2_attn, int ldo, long long bso, float* E,
                        float* rinv, float* cinv, float* ws, int b, int hw, int c, float temperature, hipStream_t stream);
