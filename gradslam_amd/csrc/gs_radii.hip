// gs_radii.hip — the radius of a depth sample as a surfel: Keller et al.'s r = (1 / sqrt 2) z / f over the cosine of the
// viewing angle, with ElasticFusion's cap on oblique surfaces (at most twice the fronto-parallel radius).  The image it
// yields is what a SurfelRadii layer fuses into the map (gs_fuse_features_batch) and what the model view with radii
// (gs_render_map_radii_dc_f32) turns back into a splat size in pixels.
//
// Arithmetic (float32, -ffp-contract=off, one rounding per operation; tests/radii_ref.py restates it):
//   fbar  = 0.5f * (K[0][0] + K[1][1])
//   r0    = (0.70710678f * z) / fbar
//   c     = fabsf(n_z)                                  n: the frame's LOCAL normal at the pixel
//   rho   = fminf(r0 / c, 2.0f * r0)                    (c == 0: 2.0f * r0)
//   valid = z > 0 and n finite and not all zero;        rho = +0.0f where not valid
#include "gs_common.h"

__global__ void __launch_bounds__(256) gs_surfel_radius_kernel(const float* __restrict__ depth, int64_t depth_stride,
                                                               const float* __restrict__ normal, int64_t normal_stride,
                                                               const float* __restrict__ K16, int64_t P, int64_t total,
                                                               float* __restrict__ radius, uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // pixel of the (n, H, W) output stack
  if (i >= total) return;
  const int64_t img = i / P, p = i - img * P;
  const float* K = K16 + 16 * img;
  const float* nrm = normal + img * normal_stride + 3 * p;
  const float z = depth[img * depth_stride + p];
  const float n0 = nrm[0], n1 = nrm[1], n2 = nrm[2];
  const bool finite = fabsf(n0) < INFINITY && fabsf(n1) < INFINITY && fabsf(n2) < INFINITY;   // (false for a NaN)
  const bool ok = z > 0.0f && finite && !(n0 == 0.0f && n1 == 0.0f && n2 == 0.0f);
  const float fbar = 0.5f * (K[0] + K[5]);
  const float r0 = (0.70710678f * z) / fbar;
  const float c = fabsf(n2), cap = 2.0f * r0;
  const float rho = c == 0.0f ? cap : fminf(r0 / c, cap);
  radius[i] = ok ? rho : 0.0f;
  if (valid) valid[i] = ok ? 1 : 0;
}

extern "C" int gs_surfel_radius_f32(const float* depth, int64_t depth_stride, const float* normal, int64_t normal_stride,
                                    const float* K16, int64_t n, int H, int W, float* radius, uint8_t* valid,
                                    void* stream) {
  GS_REQUIRE(n >= 0 && H > 0 && W > 0, "bad arguments");
  GS_REQUIRE(depth_stride >= 0 && normal_stride >= 0, "negative stride");
  if (n == 0) return GS_OK;
  GS_REQUIRE(depth && normal && K16 && radius, "NULL pointer");
  const int64_t P = (int64_t)H * W;
  GS_REQUIRE(n <= ((1ll << 31) - 1) * 256 / P, "stack too large for one launch");
  hipLaunchKernelGGL(gs_surfel_radius_kernel, dim3((unsigned)gs_ceil_div(n * P, 256)), dim3(256), 0, gs_stream(stream),
                     depth, depth_stride, normal, normal_stride, K16, P, n * P, radius, valid);
  GS_LAUNCH_CHECK();
  return GS_OK;
}
