// gs_bilateral.hip — bilateral filter of the raw depth (the pre-pass of Keller et al. / KinectFusion in front of the
// vertex and normal maps), forward and hand-written backward, batched over n frames.  Off by default everywhere.
//
// Forward (float32, one rounding per operation, -ffp-contract=off).  A pixel is valid when d > 0 (false for 0, negatives
// and NaN).  An invalid centre is copied through (its bits), W = 0.  For a valid centre q the window is visited in
// row-major order, dy = -r..r outer, dx = -r..r inner, the centre in its place; a neighbour p outside the image or
// invalid is skipped, otherwise
//     g = gs_alpha_of((float)dx, (float)dy, 0, two_s, 0)       e = gs_alpha_of(d_p - d_q, 0, 0, two_r, 0)
//     w = g * e        S = S + w * d_p        W = W + w
// and out_q = S / W (IEEE division).  two_s = (float)(2 sigma_space^2), two_r = (float)(2 sigma_range^2), evaluated in
// double by the caller.  radius 0 returns the input bits (w = 1, S = d, W = 1).  tests/bilateral_ref.py restates this
// in NumPy float32 with the oracle's exp; every forward test compares bits.
//
// Kernel shape: the 64 x 8 tile of the frame-maps kernel (one wave per row, two rows per wave) with a halo of `radius`
// on every side, staged in LDS with pixels outside the image as 0 (= invalid: the window test needs no bounds check);
// the row stride of the LDS tile is fixed (80 floats, radius 8), so a wave's 64 lanes read 64 consecutive words of a
// row in every step of the window walk (no bank conflict).  The (2r+1)^2 spatial weights are computed once per block
// (LDS, read as a broadcast).  HBM: 4 B read + 4 B written per pixel (+ 4 B with wsum); the work is (2r+1)^2 specified
// exps per pixel out of LDS.
//
// Backward: a gather per INPUT pixel p in the same fixed window order, no atomics, bitwise reproducible.  With
// c(q, p) = (d_p - out_q)(d_p - d_q) / sigma_range^2 and w_qp = w_pq (equal bits: dx^2, dy^2 and (d_p - d_q)^2 are
// symmetric)
//     depth_bar[p] = sum_{q in window(p), q != p, q valid} out_bar[q] (w_qp / W_q) (1 - c(q, p))
//                  + out_bar[p] (1 + sum_{p' != p} w_pp' c(p, p')) / W_p                              (p valid)
//     depth_bar[p] = out_bar[p]                                                                        (p invalid)
// Which neighbours are valid is a constant of the gradient.  w is the forward's float32 w (recomputed, same bits);
// EVERYTHING ELSE -- the factors c, out_bar / W, the products and both sums -- is float64, rounded to float32 once at
// the store; sigma_range^2 = (double)two_r / 2.  LDS tiles: depth, out (float32) and out_bar / W (float64, 0 at invalid
// pixels), 31 KB per block.
#include "gs_common.h"

constexpr int BL_TW = 64;    // tile width  (one wave per row)
constexpr int BL_TH = 8;     // tile height (each of the 4 waves handles 2 rows)
constexpr int BL_RMAX = 8;   // largest radius
constexpr int BL_LW = BL_TW + 2 * BL_RMAX;
constexpr int BL_LH = BL_TH + 2 * BL_RMAX;
constexpr int BL_NG = (2 * BL_RMAX + 1) * (2 * BL_RMAX + 1);

// the (2r+1)^2 spatial weights of the block, row-major over (dy, dx)
GS_DEV void bl_spatial_weights(float* __restrict__ gw, int radius, float two_s) {
  const int side = 2 * radius + 1;
  for (int i = threadIdx.x; i < side * side; i += 256) {
    const int iy = i / side, ix = i - iy * side;
    gw[i] = gs_alpha_of((float)(ix - radius), (float)(iy - radius), 0.0f, two_s, 0.0f);
  }
}

__global__ void __launch_bounds__(256) gs_bilateral_depth_kernel(
    const float* __restrict__ depth, int64_t stride_frame, int64_t stride_row, int H, int W, int radius, float two_s,
    float two_r, float* __restrict__ out, float* __restrict__ wsum) {
  __shared__ float tile[BL_LH][BL_LW];
  __shared__ float gw[BL_NG];
  const int w_base = blockIdx.x * BL_TW, h_base = blockIdx.y * BL_TH;
  const float* __restrict__ src = depth + (int64_t)blockIdx.z * stride_frame;
  const int lw_n = BL_TW + 2 * radius, lh_n = BL_TH + 2 * radius;
  for (int i = threadIdx.x; i < lh_n * lw_n; i += 256) {
    const int lh = i / lw_n, lw = i - lh * lw_n;
    const int gh = h_base + lh - radius, gx = w_base + lw - radius;
    float v = 0.0f;   // outside the image: invalid
    if (gh >= 0 && gh < H && gx >= 0 && gx < W) v = src[(int64_t)gh * stride_row + gx];
    tile[lh][lw] = v;
  }
  bl_spatial_weights(gw, radius, two_s);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = w_base + lane;
  if (w >= W) return;
  const int side = 2 * radius + 1;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int lh = wave * 2 + r;
    const int h = h_base + lh;
    if (h >= H) continue;
    const float dq = tile[lh + radius][lane + radius];
    float o = dq, Wq = 0.0f;
    if (dq > 0.0f) {
      float S = 0.0f;
      for (int iy = 0; iy < side; ++iy) {
        const float* __restrict__ row = &tile[lh + iy][lane];
        const float* __restrict__ g = &gw[iy * side];
        for (int ix = 0; ix < side; ++ix) {
          const float dp = row[ix];
          if (dp > 0.0f) {
            const float e = gs_alpha_of(dp - dq, 0.0f, 0.0f, two_r, 0.0f);
            const float wt = g[ix] * e;
            const float t = wt * dp;
            S = S + t;
            Wq = Wq + wt;
          }
        }
      }
      o = S / Wq;
    }
    const size_t p = ((size_t)blockIdx.z * H + h) * W + w;
    out[p] = o;
    if (wsum) wsum[p] = Wq;
  }
}

__global__ void __launch_bounds__(256) gs_bilateral_depth_backward_kernel(
    const float* __restrict__ depth, int64_t stride_frame, int64_t stride_row, const float* __restrict__ out,
    const float* __restrict__ wsum, const float* __restrict__ out_bar, int H, int W, int radius, float two_s,
    float two_r, float* __restrict__ depth_bar) {
  __shared__ float td[BL_LH][BL_LW];    // depth
  __shared__ float to[BL_LH][BL_LW];    // filtered depth
  __shared__ double tk[BL_LH][BL_LW];   // out_bar / W, 0 at invalid pixels
  __shared__ float gw[BL_NG];
  const int w_base = blockIdx.x * BL_TW, h_base = blockIdx.y * BL_TH;
  const float* __restrict__ src = depth + (int64_t)blockIdx.z * stride_frame;
  const size_t frame = (size_t)blockIdx.z * H * W;
  const int lw_n = BL_TW + 2 * radius, lh_n = BL_TH + 2 * radius;
  for (int i = threadIdx.x; i < lh_n * lw_n; i += 256) {
    const int lh = i / lw_n, lw = i - lh * lw_n;
    const int gh = h_base + lh - radius, gx = w_base + lw - radius;
    float d = 0.0f, o = 0.0f;
    double k = 0.0;
    if (gh >= 0 && gh < H && gx >= 0 && gx < W) {
      d = src[(int64_t)gh * stride_row + gx];
      if (d > 0.0f) {
        const size_t p = frame + (size_t)gh * W + gx;
        o = out[p];
        k = (double)out_bar[p] / (double)wsum[p];
      }
    }
    td[lh][lw] = d;
    to[lh][lw] = o;
    tk[lh][lw] = k;
  }
  bl_spatial_weights(gw, radius, two_s);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = w_base + lane;
  if (w >= W) return;
  const int side = 2 * radius + 1;
  const double isr2 = 2.0 / (double)two_r;   // 1 / sigma_range^2
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int lh = wave * 2 + r;
    const int h = h_base + lh;
    if (h >= H) continue;
    const size_t p = frame + (size_t)h * W + w;
    const float dp = td[lh + radius][lane + radius];
    if (!(dp > 0.0f)) {   // the forward is the identity here
      depth_bar[p] = out_bar[p];
      continue;
    }
    const double dpd = (double)dp, opd = (double)to[lh + radius][lane + radius];
    double A = 0.0, Bs = 0.0;
    for (int iy = 0; iy < side; ++iy) {
      const float* __restrict__ rd = &td[lh + iy][lane];
      const float* __restrict__ ro = &to[lh + iy][lane];
      const double* __restrict__ rk = &tk[lh + iy][lane];
      const float* __restrict__ g = &gw[iy * side];
      for (int ix = 0; ix < side; ++ix) {
        const float dn = rd[ix];
        if (dn > 0.0f && !(iy == radius && ix == radius)) {
          const float e = gs_alpha_of(dn - dp, 0.0f, 0.0f, two_r, 0.0f);
          const double wd = (double)(g[ix] * e);
          const double diff = (double)dn - dpd;                       // d_n - d_p
          const double c_np = ((dpd - (double)ro[ix]) * (-diff)) * isr2;   // c(q = n, p)
          const double c_pn = (((double)dn - opd) * diff) * isr2;          // c(p, p' = n)
          A = A + (rk[ix] * wd) * (1.0 - c_np);
          Bs = Bs + wd * c_pn;
        }
      }
    }
    const double res = A + tk[lh + radius][lane + radius] * (1.0 + Bs);
    depth_bar[p] = (float)res;
  }
}

// ------------------------------------------------------------------ entry points -------
static bool bl_overlap(const void* a, int64_t a_elems, const void* b, int64_t b_elems) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * (uintptr_t)a_elems;
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + 4 * (uintptr_t)b_elems;
  return a0 < b1 && b0 < a1;
}
static bool bl_sigma_ok(float two_sigma_sq) { return two_sigma_sq > 0.0f && two_sigma_sq <= 3.0e38f; }   // (NaN fails)

#define BL_CHECK_COMMON()                                                                                            \
  GS_REQUIRE(n > 0 && H > 0 && W > 0 && H <= 65535 * BL_TH, "n, H and W must be positive (H at most 524280)");       \
  GS_REQUIRE(radius >= 0 && radius <= BL_RMAX, "radius must be 0 ... 8");                                            \
  GS_REQUIRE(bl_sigma_ok(two_sigma_space_sq) && bl_sigma_ok(two_sigma_range_sq),                                     \
             "sigma_space and sigma_range must be finite and > 0");                                                  \
  GS_REQUIRE(stride_row >= W && (n == 1 || stride_frame >= (int64_t)(H - 1) * stride_row + W), "bad depth strides"); \
  const int64_t P = (int64_t)H * W;                                                                                  \
  const int64_t depth_elems = (int64_t)(n - 1) * stride_frame + (int64_t)(H - 1) * stride_row + W

extern "C" int gs_bilateral_depth_f32(const float* depth, int64_t stride_frame, int64_t stride_row, int n, int H, int W,
                                      int radius, float two_sigma_space_sq, float two_sigma_range_sq, float* out,
                                      float* wsum, void* stream) {
  GS_REQUIRE(depth && out, "depth and out must not be NULL");
  BL_CHECK_COMMON();
  GS_REQUIRE(!bl_overlap(depth, depth_elems, out, n * P), "out must not alias depth (blocks read each other's halo)");
  GS_REQUIRE(!wsum || (!bl_overlap(depth, depth_elems, wsum, n * P) && !bl_overlap(out, n * P, wsum, n * P)),
             "wsum must not alias depth or out");
  const dim3 tiles((unsigned)gs_ceil_div(W, BL_TW), (unsigned)gs_ceil_div(H, BL_TH));
  for (int f0 = 0; f0 < n; f0 += 65535) {   // (gridDim.z limit)
    const int m = n - f0 < 65535 ? n - f0 : 65535;
    hipLaunchKernelGGL(gs_bilateral_depth_kernel, dim3(tiles.x, tiles.y, (unsigned)m), dim3(256), 0, gs_stream(stream),
                       depth + (int64_t)f0 * stride_frame, stride_frame, stride_row, H, W, radius, two_sigma_space_sq,
                       two_sigma_range_sq, out + (int64_t)f0 * P, wsum ? wsum + (int64_t)f0 * P : nullptr);
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}

extern "C" int gs_bilateral_depth_backward_f32(const float* depth, int64_t stride_frame, int64_t stride_row,
                                               const float* out, const float* wsum, const float* out_bar, int n, int H,
                                               int W, int radius, float two_sigma_space_sq, float two_sigma_range_sq,
                                               float* depth_bar, void* stream) {
  GS_REQUIRE(depth && out && wsum && out_bar && depth_bar, "depth, out, wsum, out_bar and depth_bar must not be NULL");
  BL_CHECK_COMMON();
  GS_REQUIRE(!bl_overlap(depth, depth_elems, depth_bar, n * P) && !bl_overlap(out, n * P, depth_bar, n * P) &&
                 !bl_overlap(wsum, n * P, depth_bar, n * P) && !bl_overlap(out_bar, n * P, depth_bar, n * P),
             "depth_bar must not alias an input (blocks read each other's halo)");
  const dim3 tiles((unsigned)gs_ceil_div(W, BL_TW), (unsigned)gs_ceil_div(H, BL_TH));
  for (int f0 = 0; f0 < n; f0 += 65535) {
    const int m = n - f0 < 65535 ? n - f0 : 65535;
    hipLaunchKernelGGL(gs_bilateral_depth_backward_kernel, dim3(tiles.x, tiles.y, (unsigned)m), dim3(256), 0,
                       gs_stream(stream), depth + (int64_t)f0 * stride_frame, stride_frame, stride_row,
                       out + (int64_t)f0 * P, wsum + (int64_t)f0 * P, out_bar + (int64_t)f0 * P, H, W, radius,
                       two_sigma_space_sq, two_sigma_range_sq, depth_bar + (int64_t)f0 * P);
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}
