// Host-side pieces of coattn.hip that video.hip drives on its own operands (the feature banks of dcnet_amd/video.py).
#pragma once
#include <hip/hip_runtime.h>

// floats of a row of E (hw padded to a multiple of 32)
int coattn_ld_pad(int hw);
// the products of a (b, hw, c) problem run on gemm3.hip?  (what dcn_coattn_fwd decides for the same shape)
bool coattn_on_gemm3(int b, int hw, int c);
// the abs-max words of a dcn_coattn_fwd_ws workspace; word 0 = the constant 1 after coattn_amax_init
unsigned* coattn_ws_amax(float* ws, int b, int hw);
int coattn_amax_init(unsigned* am, hipStream_t stream);
// E [b][hw][ld_pad(hw)] holding A = f1 . f2^T  ->  exp(t*A - t) (split: in the f16 two-piece form), rinv / cinv [b][hw] = inverse
// row / column sums.  Steps 2 of dcn_coattn_fwd, same kernels, same launch shapes.
int coattn_exp_sums(float* E, int b, int hw, float temperature, float* rinv, float* cinv, float* ws, bool split, hipStream_t stream);
