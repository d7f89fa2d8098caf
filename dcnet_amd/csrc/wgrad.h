// Weight gradients: what wgrad.hip, wgrad3.hip and wgrad9.hip share on the host side — the split-K rule, the slab path and the one
// declaration of every function that crosses files (stem.hip, coattn.hip and gemm.hip call in as well).
#pragma once
#include "igemm.h"
#include "slabsum.h"

// ---- wgrad.hip ---------------------------------------------------------------------------------------------------------------------
// sums `splits` slabs of n4 16-byte vectors in slab order into dw (reduce_slabs_kernel)
int wgrad_reduce_slabs(const float* ws, float* dw, int64_t n4, int splits, hipStream_t stream);
int wgrad_slab_fold();       // the "Slabfold" knob
// C[b][m][n] (+)= row_scale[b][m] * sum_k A[b][k][m] * B[b][k][n]; both abs-max words present: the 128x128 tile takes the f16 two-piece split
int tn_gemm_batched(const float* A, int lda, long long a_bs, const float* B, int ldb, long long b_bs,
                    float* C, int ldc, long long c_bs, const float* row_scale,
                    int M, int m_ld, int N, int K, int batch, int accumulate, hipStream_t stream,
                    const unsigned* amax_a = nullptr, const unsigned* amax_b = nullptr);

// The launchers below take the operands as stored: esize 4 = fp32 tensors (with their abs-max words where the kernel splits), 2 = bf16
// tensors (no words).  Pixel strides in elements.
inline const char* wgrad_entry(int esize) { return esize == 2 ? "conv2d_bwd_weight_b16" : "conv2d_bwd_weight"; }

// ---- wgrad3.hip: 3x3 stride-1 layers, one filter row per workgroup (np: 2 = f16 two-piece split, 1 = bf16 operands) -------------------
bool wgrad3_shape_ok(int n, int h, int wd, int cin, int cout, int ksize, int stride);
bool wgrad3_b16_ok(int n, int h, int wd, int cin, int cout, int ksize, int stride);
int64_t wgrad3_ws(int n, int h, int wd, int cin, int cout);
int wgrad3_launch(int esize, const void* x, int ldx, const void* dy, int lddy, float* dw, float* ws, uint32_t* counters, int n, int h, int wd, int cin,
                  int cout, const uint32_t* amax_x, const uint32_t* amax_dy, int np, hipStream_t stream);

// ---- wgrad9.hip: the 32 -> 64 and 64 -> 128 3x3 layers, nine taps per workgroup (pre: fp32 only) ----------------------------------------
bool wgrad9_shape_ok(int n, int h, int wd, int cin, int cout, int ksize, int stride);
int64_t wgrad9_ws(int n, int h, int wd, int cin, int cout, int stride);
int wgrad9_launch(int esize, const void* x, int ldx, const void* dy, int lddy, float* dw, float* ws, int n, int h, int wd, int cin, int cout, int stride,
                  const uint32_t* amax_x, const uint32_t* amax_dy, const DcnPreAct* pre, hipStream_t stream);

// ---- split-K ---------------------------------------------------------------------------------------------------------------------------
// K (M positions) over `splits` workgroups per tile, each `kchunk` positions (a multiple of the kernel's K-step): base * splits
// workgroups aim at `target`, with at least 256 positions per split.  fit_round: never "a round plus a few" — splits shrink until
// base * splits fits the target (1026 workgroups cost a third round for 2 of them: -20 % on the 3x3 layers with the naive choice).
struct SplitK { int splits, kchunk; };
inline SplitK split_k(int M, int base, int target, int step, bool fit_round) {
  const int max_splits = M / 256 > 0 ? M / 256 : 1;
  int splits = target / base;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  for (;;) {
    const int kchunk = cdiv(cdiv(M, splits), step) * step;
    const SplitK s{cdiv(M, kchunk), kchunk};
    if (!fit_round || base * s.splits <= target || splits == 1 || base > target) return s;
    --splits;
  }
}
inline int64_t slab_floats(int splits, int64_t dw_floats) { return splits > 1 ? splits * dw_floats : 0; }

// ---- the slab path of a launch -------------------------------------------------------------------------------------------------------
// Where the kernel writes (dw, or the slabs in ws) and who sums the slabs: the last-arriving workgroup of a tile (fold.counters set,
// slabsum.h) or wgrad_reduce_slabs behind the launch.  groups = tile groups of the launch, tile_bytes = one workgroup's part of a
// slab; counters == nullptr: never folded.
struct SlabPath { float* out; SlabFold fold; };
inline int slab_path(SlabPath& s, const char* entry, float* dw, float* ws, uint32_t* counters, int groups, int splits, long long tile_bytes) {
  DCN_CHECK_ARG(splits == 1 || ws, "%s: workspace required (%d splits)", entry, splits);
  s.out = splits > 1 ? ws : dw;
  s.fold = slab_fold_ok(counters, groups, splits, tile_bytes, wgrad_slab_fold()) ? SlabFold{counters, dw} : SlabFold{};
  return DCN_OK;
}
inline int slab_sum(const SlabPath& s, float* dw, int64_t dw_floats, int splits, hipStream_t stream) {
  if (splits > 1 && !s.fold.counters) return wgrad_reduce_slabs(s.out, dw, dw_floats / 4, splits, stream);
  return DCN_OK;
}
