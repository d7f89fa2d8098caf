// Tube linking: one temporally consistent track per query through the top-k candidates of consecutive centres.
//
//   tube_nms          greedy non-maximum suppression in index order per centre (post_topk hands the candidates out sorted by score):
//                     candidate i is kept iff no kept j < i has iou(j, i) > thr.  A mask, nothing is compacted.
//   tube_transitions  W[t][i][j] = w_iou * iou(box[t-1,i], box[t,j]) + w_feat * <feat[t-1,i], feat[t,j]>
//   tube_forward      delta_t[j] = unary[t,j] + max_i (delta_{t-1}[i] + W[t][i][j]) over kept candidates, lowest arg-max as back-pointer
//   tube_backtrack    first arg-max of the last delta, then the back-pointers down to frame 0
//   tube_stream_step  tube_forward on the centres of one push, frame t - lag committed after step t
//   tube_stream_flush the last min(lag, n) frames of a stream and its score
//
// All arithmetic is fp32 on the vector ALU in every precision mode (like post_fusion_kernel; nothing goes through igemm_launch), every
// sum has one fixed order (bitwise repeatable), nothing synchronises the host and there are no atomics.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int TB_MAXK = 64;       // candidates per centre = lanes of a wave
constexpr int TB_EC = 64;         // feature columns per LDS chunk of tube_transitions
constexpr int TB_LD = TB_EC + 1;  // its row pitch (floats): rows 16 apart land on banks 16 apart, column reads are conflict-free
constexpr int TB_ROWS = 256;      // back-pointer rows per LDS tile of tube_backtrack
constexpr int TB_MAXLAG = 64;     // frames a streamed track may trail the newest one: 16 registers of survivor bytes per lane

// dcn_box_iou's formula with widths and heights clamped at 0: a degenerate or inverted box has IoU 0 with everything
__device__ __forceinline__ float tb_iou(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2, float by2) {
  const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  const float inter = iw * ih;
  const float aa = fmaxf(ax2 - ax1, 0.f) * fmaxf(ay2 - ay1, 0.f), ab = fmaxf(bx2 - bx1, 0.f) * fmaxf(by2 - by1, 0.f);
  return inter / (aa + ab - inter + 1e-16f);
}

__device__ __forceinline__ float tb_readlane(float v, int lane) {       // lane: wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One wave per centre, lane = candidate.  Round i: "is i still alive" is one bit of a ballot (wave-uniform); if so its box is
// broadcast and every later lane that overlaps it more than thr dies.
__global__ __launch_bounds__(256) void tube_nms_kernel(const float* __restrict__ boxes, int n, int k, float thr,
                                                       unsigned char* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n) return;                                                    // (whole waves leave: c is wave-uniform)
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  if (lane < k) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + ((size_t)c * k + lane) * 4);
    x1 = b[0]; y1 = b[1]; x2 = b[2]; y2 = b[3];
  }
  bool dead = false;
  for (int i = 0; i < k - 1; ++i) {
    const unsigned long long alive = __ballot(!dead);
    if (!((alive >> i) & 1ull)) continue;
    const float v = tb_iou(tb_readlane(x1, i), tb_readlane(y1, i), tb_readlane(x2, i), tb_readlane(y2, i), x1, y1, x2, y2);
    if (lane > i && v > thr) dead = true;
  }
  if (lane < k) keep[(size_t)c * k + lane] = dead ? 0 : 1;
}

// Block (frame t of the range, query q), 256 threads.  Thread (ti, tj) = (tid / 16, tid % 16) owns the outputs i = ti + 16 a,
// j = tj + 16 b (a, b < 4).  The feature rows of the two frames pass through LDS in chunks of TB_EC columns, each row read from
// global memory once; every output is summed by one thread with e ascending.
__global__ __launch_bounds__(256) void tube_transitions_kernel(const float* __restrict__ boxes, const float* __restrict__ feats, int n,
                                                               int k, int E, int t0, int R, float w_iou, float w_feat,
                                                               float* __restrict__ W) {
  __shared__ float fa[TB_MAXK * TB_LD], fb[TB_MAXK * TB_LD];
  __shared__ float ba[TB_MAXK * 4], bb[TB_MAXK * 4];
  const int r = blockIdx.x, q = blockIdx.y, t = t0 + r, tid = threadIdx.x;
  if (t == 0) return;                                                    // frame 0 has no predecessor: its row of W is unused
  const size_t prev = ((size_t)q * n + t - 1) * k, cur = ((size_t)q * n + t) * k;
  if (tid < 4 * k) { ba[tid] = boxes[prev * 4 + tid]; bb[tid] = boxes[cur * 4 + tid]; }
  for (int x = k * TB_LD + tid; x < TB_MAXK * TB_LD; x += 256) { fa[x] = 0.f; fb[x] = 0.f; }      // rows >= k: read, never stored
  const int ti = tid >> 4, tj = tid & 15;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  if (feats) {
    const float* pa = feats + prev * E;
    const float* pb = feats + cur * E;
    for (int e0 = 0; e0 < E; e0 += TB_EC) {
      const int len = min(TB_EC, E - e0);
      __syncthreads();
      for (int x = tid; x < k * TB_EC; x += 256) {
        const int row = x / TB_EC, e = x - row * TB_EC;
        const bool in = e < len;
        fa[row * TB_LD + e] = in ? pa[(size_t)row * E + e0 + e] : 0.f;
        fb[row * TB_LD + e] = in ? pb[(size_t)row * E + e0 + e] : 0.f;
      }
      __syncthreads();
      for (int e = 0; e < len; ++e) {
        float va[4], vb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) va[a] = fa[(ti + 16 * a) * TB_LD + e];
#pragma unroll
        for (int b = 0; b < 4; ++b) vb[b] = fb[(tj + 16 * b) * TB_LD + e];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(va[a], vb[b], acc[a][b]);
      }
    }
  }
  __syncthreads();
  float* out = W + ((size_t)q * R + r) * k * k;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = ti + 16 * a;
    if (i >= k) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = tj + 16 * b;
      if (j >= k) continue;
      const float v = tb_iou(ba[i * 4], ba[i * 4 + 1], ba[i * 4 + 2], ba[i * 4 + 3], bb[j * 4], bb[j * 4 + 1], bb[j * 4 + 2], bb[j * 4 + 3]);
      out[(size_t)i * k + j] = w_iou * v + w_feat * acc[a][b];
    }
  }
}

// One step of the recursion, shared by tube_forward_kernel and tube_stream_step_kernel.  Every wave holds delta_{t-1} in its registers
// (lane i = candidate i; the four copies are bitwise equal) and takes the predecessors i of its quarter [i0, i0 + ni), i ascending with
// a strict >; the four partial (max, arg) meet in LDS (pv, pa: this step's half) and every wave combines them in wave order with a
// strict >: the lowest arg-max.  One barrier; the caller alternates the halves of pv / pa from step to step.
__device__ __forceinline__ float tb_step(float delta, const float (&w_cur)[16], float u_cur, bool k_cur, int i0, int ni, int wave, int j,
                                         float (*pv)[TB_MAXK], int (*pa)[TB_MAXK], int& arg_out) {
  float best = -INFINITY;
  int arg = i0;
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) {
    if (ii < ni) {
      const float v = tb_readlane(delta, i0 + ii) + w_cur[ii];
      if (v > best) { best = v; arg = i0 + ii; }
    }
  }
  pv[wave][j] = best; pa[wave][j] = arg;
  __syncthreads();
  best = pv[0][j]; arg = pa[0][j];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float v = pv[w][j];
    if (v > best) { best = v; arg = pa[w][j]; }
  }
  arg_out = arg;
  return k_cur ? u_cur + best : -INFINITY;
}

// One workgroup of 4 waves per query, lane = j (tb_step).  The W rows, unary and keep of step t + 1 are loaded before step t is
// reduced, so a step waits for no memory.
__global__ __launch_bounds__(256) void tube_forward_kernel(const float* __restrict__ W, const float* __restrict__ unary,
                                                           const unsigned char* __restrict__ keep, const float* __restrict__ delta_in,
                                                           int n, int k, int t0, int t1, float* __restrict__ delta_out,
                                                           unsigned char* __restrict__ backptr) {
  __shared__ float pv[2][4][TB_MAXK];
  __shared__ int pa[2][4][TB_MAXK];
  const int q = blockIdx.x, j = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kq = (k + 3) >> 2, i0 = wave * kq, ni = max(0, min(kq, k - i0)), R = t1 - t0;
  const bool live = j < k;
  const float* Wq = W + (size_t)q * R * k * k;
  const float* uq = unary + (size_t)q * n * k;
  const unsigned char* kp = keep ? keep + (size_t)q * n * k : nullptr;
  unsigned char* bq = backptr + (size_t)q * n * k;
  float delta = -INFINITY;
  int t = t0;
  if (t0 == 0) {
    if (live) {
      delta = (!kp || kp[j]) ? uq[j] : -INFINITY;
      if (wave == 0) bq[j] = 0;
    }
    t = 1;
  } else if (live) {
    delta = delta_in[(size_t)q * k + j];
  }
  float w_nxt[16], u_nxt = 0.f;
  bool k_nxt = true;
  const int jc = min(j, k - 1);      // loads are unpredicated: lanes >= k and predecessors past the quarter read a valid, unused element
  unsigned off[16];                  // per-lane element offsets of W[.][i0 + ii][j] inside a frame's k x k block
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) off[ii] = (unsigned)(min(i0 + ii, k - 1) * k + jc);
  auto fetch = [&](int tt) {
    const float* wr = Wq + (size_t)(tt - t0) * k * k;
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) w_nxt[ii] = wr[off[ii]];
    u_nxt = uq[(size_t)tt * k + jc];
    k_nxt = live && (!kp || kp[(size_t)tt * k + jc]);
  };
  if (t < t1) fetch(t);
  for (; t < t1; ++t) {
    float w_cur[16];
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) w_cur[ii] = w_nxt[ii];
    const float u_cur = u_nxt;
    const bool k_cur = k_nxt;
    if (t + 1 < t1) fetch(t + 1);
    const int p = t & 1;             // (one barrier per step: the partials of step t + 1 go to the other half of pv / pa)
    int arg;
    delta = tb_step(delta, w_cur, u_cur, k_cur, i0, ni, wave, j, pv[p], pa[p], arg);
    if (wave == 0 && live) bq[(size_t)t * k + j] = (unsigned char)arg;
  }
  if (wave == 0 && live) delta_out[(size_t)q * k + j] = delta;
}

// One workgroup per query.  Lane 0 walks the back-pointers, which the whole workgroup stages into LDS a tile of TB_ROWS frames at
// a time (a walk of dependent global byte loads would pay a cache latency per frame); the tile's path leaves in one coalesced store.
__global__ __launch_bounds__(256) void tube_backtrack_kernel(const unsigned char* __restrict__ backptr, const float* __restrict__ delta,
                                                             int n, int k, int64_t* __restrict__ path, float* __restrict__ score) {
  __shared__ unsigned char tile[TB_ROWS * TB_MAXK];
  __shared__ int pth[TB_ROWS];
  __shared__ int s_p;
  const int q = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    const float* d = delta + (size_t)q * k;
    float best = d[0]; int arg = 0;
    for (int i = 1; i < k; ++i) if (d[i] > best) { best = d[i]; arg = i; }           // first arg-max
    score[q] = best;
    s_p = arg;
  }
  const unsigned char* bq = backptr + (size_t)q * n * k;
  for (int hi = n; hi > 0; hi -= TB_ROWS) {
    const int lo = max(0, hi - TB_ROWS), rows = hi - lo;
    __syncthreads();
    for (int x = tid; x < rows * k; x += 256) tile[x] = bq[(size_t)lo * k + x];
    __syncthreads();
    if (tid == 0) {
      int p = s_p;
      for (int r = rows - 1; r >= 0; --r) { pth[r] = p; if (lo + r > 0) p = min((int)tile[r * k + p], k - 1); }     // (min: a foreign table stays in the tile)
      s_p = p;
    }
    __syncthreads();
    for (int r = tid; r < rows; r += 256) path[(size_t)q * n + lo + r] = pth[r];
  }
}

// Streaming forward pass with commitment: tube_forward_kernel's recursion (tb_step) over the m centres
// t0 ... t0 + m - 1 of one push, plus the survivor memory that lets frame t - lag leave after step t.  Register exchange, as in a
// hardware Viterbi decoder: lane j keeps the last lag choices of its survivor as bytes (byte b of hist = the candidate of frame
// t - lag + b on the best path into candidate j of frame t) in NW = ceil(lag / 4) registers; the bytes from lag on stay 0.  A step
// fetches the words of lane arg with ds_bpermute (all NW in flight at once: NW is a template parameter, nothing branches), shifts
// them down a byte and puts arg in at byte lag - 1; byte 0 is the ancestor a[j] at frame t - lag.  If the live lanes (delta > -inf)
// agree on it (two ballots) it is committed; else the ancestor of the first arg-max of delta_t is, the lanes that disagree are set to
// -inf and the query's forced count grows by one.  All four waves keep the (bitwise equal) state, so the commitment needs no barrier
// of its own; wave 0 writes.  surv [q][lag][k] bytes carries hist from launch to launch, delta [q][k] the scores.
template <int NW>
__global__ __launch_bounds__(256) void tube_stream_step_kernel(const float* __restrict__ W, const float* __restrict__ unary,
                                                               const unsigned char* __restrict__ keep, int m, int k, int t0, int lag,
                                                               float* __restrict__ delta_io, unsigned char* __restrict__ surv,
                                                               int64_t* __restrict__ commit, int* __restrict__ forced) {
  __shared__ float pv[2][4][TB_MAXK];
  __shared__ int pa[2][4][TB_MAXK];
  const int q = blockIdx.x, j = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kq = (k + 3) >> 2, i0 = wave * kq, ni = max(0, min(kq, k - i0));
  const int sh = ((lag - 1) & 3) * 8;                                  // bit of byte lag - 1 in hist[NW - 1] (NW == ceil(lag / 4))
  const unsigned top_mask = 0xffffffffu >> (24 - sh);                   // the bytes of hist[NW - 1] below lag
  const bool live = j < k, writer = wave == 0 && j == 0;
  const float* Wq = W + (size_t)q * m * k * k;
  const float* uq = unary + (size_t)q * m * k;
  const unsigned char* kp = keep ? keep + (size_t)q * m * k : nullptr;
  unsigned char* sq = surv + (size_t)q * lag * k;
  int64_t* cq = commit + (size_t)q * m;
  const int jc = min(j, k - 1);
  unsigned hist[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) hist[w] = 0u;
  float delta = -INFINITY;
  int r = 0, nforced = 0;            // r: index within the push, t = t0 + r
  if (t0 == 0) {
    if (live) delta = (!kp || kp[j]) ? uq[j] : -INFINITY;
    if (writer) cq[0] = -1;
    r = 1;
  } else {
    if (live) delta = delta_io[(size_t)q * k + j];
#pragma unroll
    for (int w = 0; w < NW; ++w) {   // unpredicated (one wait for all of them): a byte past lag - 1 re-reads the last one and is masked off
#pragma unroll
      for (int b = 0; b < 4; ++b) hist[w] |= (unsigned)sq[(size_t)min(4 * w + b, lag - 1) * k + jc] << (8 * b);
    }
    hist[NW - 1] &= top_mask;
  }
  float w_nxt[16], u_nxt = 0.f;
  bool k_nxt = true;
  unsigned off[16];
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) off[ii] = (unsigned)(min(i0 + ii, k - 1) * k + jc);
  auto fetch = [&](int rr) {
    const float* wr = Wq + (size_t)rr * k * k;
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) w_nxt[ii] = wr[off[ii]];
    u_nxt = uq[(size_t)rr * k + jc];
    k_nxt = live && (!kp || kp[(size_t)rr * k + jc]);
  };
  if (r < m) fetch(r);
  for (; r < m; ++r) {
    float w_cur[16];
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) w_cur[ii] = w_nxt[ii];
    const float u_cur = u_nxt;
    const bool k_cur = k_nxt;
    if (r + 1 < m) fetch(r + 1);
    const int p = r & 1;
    int arg;
    delta = tb_step(delta, w_cur, u_cur, k_cur, i0, ni, wave, j, pv[p], pa[p], arg);
    unsigned pw[NW];                 // the survivor of j = that of arg without its oldest frame, and arg
#pragma unroll
    for (int w = 0; w < NW; ++w) pw[w] = (unsigned)__builtin_amdgcn_ds_bpermute(arg << 2, (int)hist[w]);
#pragma unroll
    for (int w = 0; w < NW - 1; ++w) hist[w] = (pw[w] >> 8) | (pw[w + 1] << 24);
    hist[NW - 1] = (pw[NW - 1] >> 8) | ((unsigned)arg << sh);
    long long c_out = -1;
    if (t0 + r >= lag) {
      const int a = (int)(hist[0] & 0xffu);
      const bool alive = delta > -INFINITY;
      const unsigned long long lm = __ballot(alive);
      int c = __builtin_amdgcn_readlane(a, lm ? __ffsll((long long)lm) - 1 : 0);
      if (__ballot(alive && a != c)) {                                   // (wave-uniform: some live survivor has another ancestor)
        float mx = delta;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        const unsigned long long am = __ballot(delta == mx);           // (lm != 0: mx is finite, lanes >= k hold -inf)
        c = __builtin_amdgcn_readlane(a, __ffsll((long long)am) - 1);  // the ancestor of the first arg-max
        if (a != c) delta = -INFINITY;
        ++nforced;
      }
      c_out = c;
    }
    if (writer) cq[r] = c_out;
  }
  if (wave == 0 && live) {
    delta_io[(size_t)q * k + j] = delta;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (w < NW - 1 || 4 * w + b < lag) sq[(size_t)(4 * w + b) * k + j] = (unsigned char)(hist[w] >> (8 * b));
    }
  }
  if (writer && nforced) forced[q] += nforced;                           // (the only writer of forced[q]: no atomic)
}

// End of a stream: the first arg-max of the last delta and its survivor, the frames that tube_stream_step_kernel has not committed.
// One wave per query.
__global__ __launch_bounds__(64) void tube_stream_flush_kernel(const float* __restrict__ delta, const unsigned char* __restrict__ surv,
                                                               int k, int n, int lag, int64_t* __restrict__ tail,
                                                               float* __restrict__ score) {
  const int q = blockIdx.x, j = threadIdx.x;
  const float d = j < k ? delta[(size_t)q * k + j] : -INFINITY;
  float mx = d;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  const int js = min(__ffsll((long long)__ballot(d == mx)) - 1, k - 1);  // first arg-max (lane 0 if every delta is -inf)
  const int m = min(lag, n);
  int64_t* tq = tail + (size_t)q * m;
  if (j == 0) { score[q] = mx; tq[m - 1] = js; }
  if (j < m - 1) tq[j] = surv[((size_t)q * lag + lag - m + 1 + j) * k + js];      // byte b of the survivor: frame n - 1 - lag + b
}

}  // namespace

extern "C" int dcn_post_nms(const float* boxes, int n, int k, float iou_thr, unsigned char* keep, void* stream) {
  DCN_CHECK_ARG(boxes && keep && n >= 1 && k >= 1 && k <= TB_MAXK, "post_nms: bad argument (n=%d k=%d)", n, k);
  hipLaunchKernelGGL(tube_nms_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, boxes, n, k, iou_thr, keep);
  DCN_CHECK_LAUNCH("post_nms");
  return DCN_OK;
}

extern "C" int dcn_tube_transitions(const float* boxes, const float* feats, int q, int n, int k, int e, int t0, int t1, float w_iou,
                                    float w_feat, float* W, void* stream) {
  DCN_CHECK_ARG(boxes && W && q >= 1 && q <= 65535 && n >= 1 && k >= 1 && k <= TB_MAXK && t0 >= 0 && t0 < t1 && t1 <= n,
                "tube_transitions: bad argument (q=%d n=%d k=%d t0=%d t1=%d)", q, n, k, t0, t1);
  DCN_CHECK_ARG(w_iou >= 0.f && w_feat >= 0.f, "tube_transitions: negative weight (w_iou=%g w_feat=%g)", (double)w_iou, (double)w_feat);
  DCN_CHECK_ARG(feats ? e >= 1 : w_feat == 0.f, "tube_transitions: %s", feats ? "e < 1" : "feats is NULL but w_feat != 0");
  hipLaunchKernelGGL(tube_transitions_kernel, dim3(t1 - t0, q), dim3(256), 0, (hipStream_t)stream, boxes, feats, n, k, e, t0, t1 - t0,
                     w_iou, w_feat, W);
  DCN_CHECK_LAUNCH("tube_transitions");
  return DCN_OK;
}

extern "C" int dcn_tube_forward(const float* W, const float* unary, const unsigned char* keep, const float* delta_in, int q, int n, int k,
                                int t0, int t1, float* delta_out, unsigned char* backptr, void* stream) {
  DCN_CHECK_ARG(W && unary && delta_out && backptr && q >= 1 && n >= 1 && k >= 1 && k <= TB_MAXK && t0 >= 0 && t0 < t1 && t1 <= n,
                "tube_forward: bad argument (q=%d n=%d k=%d t0=%d t1=%d)", q, n, k, t0, t1);
  DCN_CHECK_ARG((delta_in != nullptr) == (t0 > 0), "tube_forward: delta_in must be given iff t0 > 0 (t0=%d)", t0);
  hipLaunchKernelGGL(tube_forward_kernel, dim3(q), dim3(256), 0, (hipStream_t)stream, W, unary, keep, delta_in, n, k, t0, t1, delta_out,
                     backptr);
  DCN_CHECK_LAUNCH("tube_forward");
  return DCN_OK;
}

extern "C" int dcn_tube_backtrack(const unsigned char* backptr, const float* delta, int q, int n, int k, int64_t* path, float* score,
                                  void* stream) {
  DCN_CHECK_ARG(backptr && delta && path && score && q >= 1 && n >= 1 && k >= 1 && k <= TB_MAXK,
                "tube_backtrack: bad argument (q=%d n=%d k=%d)", q, n, k);
  hipLaunchKernelGGL(tube_backtrack_kernel, dim3(q), dim3(256), 0, (hipStream_t)stream, backptr, delta, n, k, path, score);
  DCN_CHECK_LAUNCH("tube_backtrack");
  return DCN_OK;
}

extern "C" int dcn_tube_stream_step(const float* W, const float* unary, const unsigned char* keep, int q, int m, int k, int t0, int lag,
                                    float* delta, unsigned char* surv, int64_t* commit, int* forced, void* stream) {
  DCN_CHECK_ARG(W && unary && delta && surv && commit && forced && q >= 1 && m >= 1 && k >= 1 && k <= TB_MAXK && t0 >= 0 &&
                    t0 <= INT_MAX - m,
                "tube_stream_step: bad argument (q=%d m=%d k=%d t0=%d)", q, m, k, t0);
  DCN_CHECK_ARG(lag >= 1 && lag <= TB_MAXLAG, "tube_stream_step: lag = %d outside 1 ... %d", lag, TB_MAXLAG);
#define TB_STREAM_CASE(NW)                                                                                                          \
  case NW:                                                                                                                          \
    hipLaunchKernelGGL(tube_stream_step_kernel<NW>, dim3(q), dim3(256), 0, (hipStream_t)stream, W, unary, keep, m, k, t0, lag, delta, \
                       surv, commit, forced);                                                                                       \
    break;
  switch ((lag + 3) >> 2) {          // registers of survivor bytes per lane
    TB_STREAM_CASE(1) TB_STREAM_CASE(2) TB_STREAM_CASE(3) TB_STREAM_CASE(4) TB_STREAM_CASE(5) TB_STREAM_CASE(6) TB_STREAM_CASE(7)
    TB_STREAM_CASE(8) TB_STREAM_CASE(9) TB_STREAM_CASE(10) TB_STREAM_CASE(11) TB_STREAM_CASE(12) TB_STREAM_CASE(13)
    TB_STREAM_CASE(14) TB_STREAM_CASE(15) TB_STREAM_CASE(16)
  }
#undef TB_STREAM_CASE
  DCN_CHECK_LAUNCH("tube_stream_step");
  return DCN_OK;
}

extern "C" int dcn_tube_stream_flush(const float* delta, const unsigned char* surv, int q, int k, int n, int lag, int64_t* tail,
                                     float* score, void* stream) {
  DCN_CHECK_ARG(delta && surv && tail && score && q >= 1 && n >= 1 && k >= 1 && k <= TB_MAXK,
                "tube_stream_flush: bad argument (q=%d n=%d k=%d)", q, n, k);
  DCN_CHECK_ARG(lag >= 1 && lag <= TB_MAXLAG, "tube_stream_flush: lag = %d outside 1 ... %d", lag, TB_MAXLAG);
  hipLaunchKernelGGL(tube_stream_flush_kernel, dim3(q), dim3(64), 0, (hipStream_t)stream, delta, surv, k, n, lag, tail, score);
  DCN_CHECK_LAUNCH("tube_stream_flush");
  return DCN_OK;
}
