// Clip preprocessing of the data pipeline: decoded uint8 frames -> the model's normalised fp32 NCHW input
// (dataset/vid_loader.py:333-395, utils/transforms.py:123-185; SURVEY.md §8(e) "input generation").
//
//   prep_letterbox   per letterbox pixel: flip (index), 8-bit RGB->HSV->RGB with V scaled by a_v, INTER_AREA resize
//                    (area box for downscale, 11-bit two-tap rule for upscale), constant pad -> RGBx uint8 workspace
//   prep_warp        per output pixel: inverse affine in fp64 rounded to 1/32 pixel, bilinear with 15-bit weights and a
//                    constant border, ToTensor + Normalize -> fp32 NCHW (and optionally the uint8 warped frame)
//
// One launch of each per batch, whatever its size: a ragged batch is a table of DcnPrepJob records over one packed byte
// buffer.  Every rule is integer- or IEEE-specified (DESIGN.md "Clip preprocessing") and restated in numpy by
// tests/prep_np.py; contraction is off so that every fp32 / fp64 product and sum rounds where the restatement's does.
#pragma clang fp contract(off)
#include <math.h>
#include <stddef.h>
#include "common.h"

static_assert(sizeof(DcnPrepJob) == 96, "DcnPrepJob is a 96-byte record (dcnet_amd/prep.py JOB_DTYPE)");
static_assert(offsetof(DcnPrepJob, a_v) == 40 && offsetof(DcnPrepJob, minv) == 48, "DcnPrepJob layout");

namespace {

constexpr int PT_X = 32, PT_Y = 8;            // tile of one 256-thread workgroup: 32 x 8 pixels
constexpr int PAD_R = 124, PAD_G = 116, PAD_B = 104;   // saturate_cast<uchar>(123.7, 116.3, 103.5)

// 8-bit RGB -> HSV (12-bit fixed-point division tables) -> V' = trunc(V * a_v) (clipped when a_v > 1) -> RGB (float path)
__device__ __forceinline__ void hsv_scale_v(int& r, int& g, int& b, float a_v, const int* __restrict__ sdiv,
                                            const int* __restrict__ hdiv) {
  const int v = max(max(r, g), b), vmin = min(min(r, g), b), diff = v - vmin;
  const int s = (diff * sdiv[v] + (1 << 11)) >> 12;
  int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * hdiv[diff] + (1 << 11)) >> 12;
  if (h < 0) h += 180;
  float vf = (float)v * a_v;
  if (a_v > 1.f) vf = fminf(vf, 255.f);
  const int V = (int)vf;                                        // astype(uint8) of a value in [0, 255]: truncation
  const float vv = (float)V * (1.f / 255.f);
  float fr, fg, fb;
  if (s == 0) {
    fr = fg = fb = vv;
  } else {
    const float sv = (float)s * (1.f / 255.f);
    float hh = (float)h * (6.f / 180.f);
    int sector = (int)floorf(hh);
    hh = hh - (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
    const float t0 = vv, t1 = vv * (1.f - sv), t2 = vv * (1.f - sv * hh), t3 = vv * (1.f - sv * (1.f - hh));
    // (b, g, r) = tab[sector_data[sector]] with sector_data = {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}
    switch (sector) {
      case 0: fb = t1; fg = t3; fr = t0; break;
      case 1: fb = t1; fg = t0; fr = t2; break;
      case 2: fb = t3; fg = t0; fr = t1; break;
      case 3: fb = t0; fg = t2; fr = t1; break;
      case 4: fb = t0; fg = t1; fr = t3; break;
      default: fb = t2; fg = t1; fr = t0; break;
    }
  }
  r = min(max(__float2int_rn(fr * 255.f), 0), 255);
  g = min(max(__float2int_rn(fg * 255.f), 0), 255);
  b = min(max(__float2int_rn(fb * 255.f), 0), 255);
}

struct Src {
  const uint8_t* p;
  int h, w, flip, hsv;
  float a_v;
  const int *sdiv, *hdiv;
  // pixel (row, col) of the flipped, HSV-adjusted frame; indices are clamped into the frame (the rules never leave it)
  __device__ __forceinline__ void at(int row, int col, int& r, int& g, int& b) const {
    row = min(max(row, 0), h - 1);
    col = min(max(col, 0), w - 1);
    if (flip) col = w - 1 - col;
    const uint8_t* q = p + ((size_t)row * w + col) * 3;
    r = q[0]; g = q[1]; b = q[2];
    if (hsv) hsv_scale_v(r, g, b, a_v, sdiv, hdiv);
  }
};

// INTER_AREA downscale taps of one axis (OpenCV computeResizeAreaTab): [first, last] source indices, the fractional end weights
struct AreaAxis {
  int first, last;
  float wl, wm, wr;        // weight of `first` when it is a partial cell, of the full cells, of `last` when partial
  bool hl, hr;
  __device__ __forceinline__ AreaAxis(int d, int ssize, int dsize) {
    const double scale = 1.0 / ((double)dsize / (double)ssize);
    const double fs1 = (double)d * scale, fs2 = fs1 + scale;
    const double cell = fmin(scale, (double)ssize - fs1);
    int s2 = (int)floor(fs2), s1 = (int)ceil(fs1);
    s2 = min(s2, ssize - 1);
    s1 = min(s1, s2);
    hl = (double)s1 - fs1 > 1e-3;
    hr = fs2 - (double)s2 > 1e-3;
    wl = (float)(((double)s1 - fs1) / cell);
    wm = (float)(1.0 / cell);
    wr = (float)(fmin(fmin(fs2 - (double)s2, 1.0), cell) / cell);
    first = hl ? s1 - 1 : s1;
    last = hr ? s2 : s2 - 1;
  }
  __device__ __forceinline__ float weight(int s) const { return (hl && s == first) ? wl : ((hr && s == last) ? wr : wm); }
};

// INTER_AREA upscale rule of one axis (OpenCV resize, area_mode): source index and 11-bit weights of it and its successor
__device__ __forceinline__ void lin_axis(int d, int ssize, int dsize, int& s0, int& s1, int& a0, int& a1) {
  const double inv = (double)dsize / (double)ssize, scale = 1.0 / inv;
  int sx = (int)floor((double)d * scale);
  float fx = (float)((double)(d + 1) - (double)(sx + 1) * inv);
  fx = fx <= 0.f ? 0.f : fx - floorf(fx);
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= ssize - 1) { fx = 0.f; sx = ssize - 1; }
  s0 = sx; s1 = min(sx + 1, ssize - 1);
  a0 = __float2int_rn((1.f - fx) * 2048.f);
  a1 = __float2int_rn(fx * 2048.f);
}

__global__ __launch_bounds__(256) void prep_letterbox_kernel(const uint8_t* __restrict__ src, const DcnPrepJob* __restrict__ jobs,
                                                             int S, uchar4* __restrict__ lb) {
  __shared__ int sdiv[256], hdiv[256];
  const int tid = threadIdx.x;
  // sdiv[i] = round((255 << 12) / i), hdiv[i] = round((180 << 12) / (6 i)): cvRound, ties to even
  sdiv[tid] = tid ? (int)rint(1044480.0 / (double)tid) : 0;
  hdiv[tid] = tid ? (int)rint(737280.0 / (6.0 * (double)tid)) : 0;
  __syncthreads();
  const int f = blockIdx.y, tiles_x = S / PT_X;
  const int x = (blockIdx.x % tiles_x) * PT_X + (tid & (PT_X - 1)), y = (blockIdx.x / tiles_x) * PT_Y + (tid / PT_X);
  const DcnPrepJob& J = jobs[f];
  const int lx = x - J.left, ly = y - J.top;
  int R = PAD_R, G = PAD_G, B = PAD_B;
  if (lx >= 0 && ly >= 0 && lx < J.rw && ly < J.rh) {
    const Src s{src + J.src_off, J.h, J.w, J.flip, J.hsv, J.a_v, sdiv, hdiv};
    if (J.w >= J.rw && J.h >= J.rh) {                            // downscale (or same size): area-weighted box, fp32
      const AreaAxis ax(lx, J.w, J.rw), ay(ly, J.h, J.rh);
      float tr = 0.f, tg = 0.f, tb = 0.f;
      for (int sy = ay.first; sy <= ay.last; ++sy) {
        float rr = 0.f, rg = 0.f, rb = 0.f;
        for (int sx = ax.first; sx <= ax.last; ++sx) {
          int r, g, b;
          s.at(sy, sx, r, g, b);
          const float wx = ax.weight(sx);
          rr = rr + wx * (float)r; rg = rg + wx * (float)g; rb = rb + wx * (float)b;
        }
        const float wy = ay.weight(sy);
        tr = tr + wy * rr; tg = tg + wy * rg; tb = tb + wy * rb;
      }
      R = min(max(__float2int_rn(tr), 0), 255);
      G = min(max(__float2int_rn(tg), 0), 255);
      B = min(max(__float2int_rn(tb), 0), 255);
    } else {                                                     // upscale: two taps per axis, 11-bit fixed point
      int x0, x1, a0, a1, y0, y1, b0, b1;
      lin_axis(lx, J.w, J.rw, x0, x1, a0, a1);
      lin_axis(ly, J.h, J.rh, y0, y1, b0, b1);
      int p00[3], p01[3], p10[3], p11[3];
      s.at(y0, x0, p00[0], p00[1], p00[2]); s.at(y0, x1, p01[0], p01[1], p01[2]);
      s.at(y1, x0, p10[0], p10[1], p10[2]); s.at(y1, x1, p11[0], p11[1], p11[2]);
      int o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int d0 = a0 * p00[c] + a1 * p01[c], d1 = a0 * p10[c] + a1 * p11[c];
        o[c] = min(max((b0 * d0 + b1 * d1 + (1 << 21)) >> 22, 0), 255);
      }
      R = o[0]; G = o[1]; B = o[2];
    }
  }
  lb[((size_t)f * S + y) * S + x] = make_uchar4((unsigned char)R, (unsigned char)G, (unsigned char)B, 0);
}

__global__ __launch_bounds__(256) void prep_warp_kernel(const uchar4* __restrict__ lb, const DcnPrepJob* __restrict__ jobs, int S,
                                                        float* __restrict__ out, uint8_t* __restrict__ u8) {
  const int tid = threadIdx.x, f = blockIdx.y, tiles_x = S / PT_X;
  const int x = (blockIdx.x % tiles_x) * PT_X + (tid & (PT_X - 1)), y = (blockIdx.x / tiles_x) * PT_Y + (tid / PT_X);
  const DcnPrepJob& J = jobs[f];
  const uchar4* img = lb + (size_t)f * S * S;
  int v[3];
  if (!J.warp) {
    const uchar4 p = img[(size_t)y * S + x];
    v[0] = p.x; v[1] = p.y; v[2] = p.z;
  } else {
    // source coordinate in fp64, rounded to 1/32 pixel (W = 1 for an affine M: the scale factor is 32 / 1)
    double X = J.minv[0] * (double)x + J.minv[1] * (double)y + J.minv[2];
    double Y = J.minv[3] * (double)x + J.minv[4] * (double)y + J.minv[5];
    X = fmin(fmax(X * 32.0, -1073741824.0), 1073741824.0);
    Y = fmin(fmax(Y * 32.0, -1073741824.0), 1073741824.0);
    const int Xi = __double2int_rn(X), Yi = __double2int_rn(Y);
    const int sx = Xi >> 5, sy = Yi >> 5, ax = Xi & 31, ay = Yi & 31;
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    const int pad[3] = {PAD_R, PAD_G, PAD_B};
    int t[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xx = sx + (k & 1), yy = sy + (k >> 1);
      if (xx >= 0 && yy >= 0 && xx < S && yy < S) {
        const uchar4 p = img[(size_t)yy * S + xx];
        t[k][0] = p.x; t[k][1] = p.y; t[k][2] = p.z;
      } else {
        t[k][0] = pad[0]; t[k][1] = pad[1]; t[k][2] = pad[2];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      v[c] = min((t[0][c] * w00 + t[1][c] * w01 + t[2][c] * w10 + t[3][c] * w11 + (1 << 14)) >> 15, 255);
  }
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const size_t plane = (size_t)S * S, o = (size_t)f * 3 * plane + (size_t)y * S + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[o + c * plane] = ((float)v[c] / 255.f - mean[c]) / stdv[c];
  if (u8) {
    uint8_t* q = u8 + (((size_t)f * S + y) * S + x) * 3;
    q[0] = (uint8_t)v[0]; q[1] = (uint8_t)v[1]; q[2] = (uint8_t)v[2];
  }
}

}  // namespace

extern "C" int64_t dcn_clip_prep_ws(int n, int size) { return n > 0 && size > 0 ? (int64_t)n * size * size * 4 : 0; }

extern "C" int dcn_clip_prep(const uint8_t* src, int64_t src_bytes, const DcnPrepJob* jobs, const DcnPrepJob* jobs_host, int n, int size,
                             uint8_t* ws, float* out, uint8_t* u8_out, void* stream) {
  DCN_CHECK_ARG(src && jobs && jobs_host && ws && out, "clip_prep: null argument");
  DCN_CHECK_ARG(n > 0 && n <= 65535 && src_bytes > 0, "clip_prep: bad batch (n=%d, src_bytes=%lld)", n, (long long)src_bytes);
  DCN_CHECK_ARG(size >= 32 && size <= 4096 && size % 32 == 0, "clip_prep: size %d is not a multiple of 32 in [32, 4096]", size);
  DCN_CHECK_ARG(((uintptr_t)ws & 3) == 0, "clip_prep: workspace not 4-byte aligned");
  for (int i = 0; i < n; ++i) {
    const DcnPrepJob& J = jobs_host[i];
    DCN_CHECK_ARG(J.h > 0 && J.w > 0 && J.h <= 16384 && J.w <= 16384, "clip_prep: job %d: bad frame size %dx%d", i, J.h, J.w);
    DCN_CHECK_ARG(J.src_off >= 0 && J.src_off + (int64_t)J.h * J.w * 3 <= src_bytes,
                  "clip_prep: job %d: frame [%lld, +%lld) outside the source buffer (%lld bytes)", i, (long long)J.src_off,
                  (long long)J.h * J.w * 3, (long long)src_bytes);
    DCN_CHECK_ARG(J.rh > 0 && J.rw > 0 && J.top >= 0 && J.left >= 0 && J.top + J.rh <= size && J.left + J.rw <= size,
                  "clip_prep: job %d: letterbox %dx%d at (%d, %d) does not fit %d", i, J.rh, J.rw, J.top, J.left, size);
    DCN_CHECK_ARG((J.flip == 0 || J.flip == 1) && (J.hsv == 0 || J.hsv == 1) && (J.warp == 0 || J.warp == 1),
                  "clip_prep: job %d: flags must be 0 or 1", i);
    DCN_CHECK_ARG(!J.hsv || (isfinite(J.a_v) && J.a_v >= 0.f && J.a_v <= 2.f), "clip_prep: job %d: a_v %g outside [0, 2]", i, (double)J.a_v);
    for (int k = 0; k < 6 && J.warp; ++k) DCN_CHECK_ARG(isfinite(J.minv[k]), "clip_prep: job %d: non-finite warp", i);
  }
  const dim3 grid((size / PT_X) * (size / PT_Y), n);
  hipLaunchKernelGGL(prep_letterbox_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, jobs, size, (uchar4*)ws);
  DCN_CHECK_LAUNCH("clip_prep letterbox");
  hipLaunchKernelGGL(prep_warp_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const uchar4*)ws, jobs, size, out, u8_out);
  DCN_CHECK_LAUNCH("clip_prep warp");
  return DCN_OK;
}
