// gs_carve.hip — free-space carving: which surfels of a map do later depth frames see through?
//
// The map update only merges and appends, and gs_prune.hip only drops rows of low confidence: a surfel of something that
// has moved away keeps its confidence, and the surface behind it is appended behind it (the new measurements fail the
// distance gate against it).  Keller et al.'s point-based fusion removes such points as free-space violations.  This
// pass finds them; the removal is the stable compaction of gs_prune.hip (its keep mask).
//
// The rule, for row r < n = min(*n_dev, n_bound) with point p, and view l with pose T_l, intrinsics K and depth D_l:
//   cam = gs_camera(T_l, K);  in = gs_project_point_hw_q(cam, p, H, W, u_hi, v_hi, h, w, q);  z = q[2]
//   (the association's and the render's projection, unchanged: the pixel the map update and the model view give the row)
//   r violates l  iff  in  &&  D_l[h, w] > 0  &&  for every pixel (hh, ww) of the (2 window + 1)^2 square around (h, w),
//   clipped to the image, with D_l[hh, ww] > 0:  (D_l[hh, ww] - z) > margin       (float32: one subtraction, one compare)
// "> 0" is false for 0, negative depths and NaN: pixels without a measurement abstain, and a centre pixel without one is
// no evidence.  Equality at the margin does not violate.  So the row must lie in front of the nearest measured depth of
// its window: a surfel next to a depth edge is not carved because rounding put it on the background side.
//   violations[r] = number of views of the call r violates;  keep[r] = violations[r] < min_views
// Rows in [n, n_bound) get violations = 0 and keep = 0 without being read.  Every element of both outputs is written by
// exactly one thread: no atomics, no clearing, no read-back; integer outputs, a pure function of the inputs.
//
// One thread per map row, the sequence index in the grid (as gs_render.hip / gs_prune.hip).  A thread walks all L views
// inside the one launch with its count in a register; the cameras are built once per block into LDS, GS_CV_GROUP views
// at a time.  The window is read only once the centre pixel has depth and itself violates (the rule is a conjunction, so
// the result is the same): for a row on the surface the depth frame shows -- almost all rows -- a view costs one 4-byte
// gather.
//
// Bytes per row and view: 12 B of the point once per launch, 4 B gathered per view in which the row is in the frame
// (rows that are neighbours in the map are mostly neighbours in the image, so a wave's gathers share cache lines),
// (2 window + 1)^2 - 1 more only for rows whose centre pixel violates; 5 B written per row.
#include "gs_assoc_dev.h"

#include <math.h>

constexpr int GS_CV_GROUP = 16;      // cameras in LDS at a time (96 B each)
constexpr int GS_CV_MAX_WINDOW = 3;

struct CvSeq {
  const float* points;
  GsCount n;
  const float* depth;      // view 0
  int64_t stride_view;     // in floats
  const float* poses16;    // (L, 16)
  const float* K16;
  int32_t* violations;     // (n.host) or NULL
  uint8_t* keep;           // (n.host) or NULL
};
struct CvBatch {
  CvSeq s[GS_MAX_BATCH];
  int B, L, H, W, window, min_views;
  float margin, u_hi, v_hi;
};

__global__ void __launch_bounds__(256) gs_free_space_kernel(const CvBatch cb) {
  __shared__ GsCamera cams[GS_CV_GROUP];
  const CvSeq& q = cb.s[blockIdx.x % cb.B];
  const int64_t base = (int64_t)(blockIdx.x / cb.B) * 256;
  if (base >= q.n.host) return;   // (the whole block: a shorter map of the batch)
  const int64_t r = base + threadIdx.x;
  const int64_t n = gs_count(q.n);
  const bool live = r < n;
  int count = 0;
  if (base < n) {   // (block-uniform: the barriers below are reached by every thread of the block or by none)
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
    if (live) {
      p0 = q.points[3 * r];
      p1 = q.points[3 * r + 1];
      p2 = q.points[3 * r + 2];
    }
    const int win = cb.window;
    for (int v0 = 0; v0 < cb.L; v0 += GS_CV_GROUP) {
      const int V = cb.L - v0 < GS_CV_GROUP ? cb.L - v0 : GS_CV_GROUP;
      if (v0 > 0) __syncthreads();   // the cameras of the group before are no longer read
      if ((int)threadIdx.x < V) cams[threadIdx.x] = gs_camera(q.poses16 + 16 * (int64_t)(v0 + threadIdx.x), q.K16);
      __syncthreads();
      if (!live) continue;
      for (int v = 0; v < V; ++v) {
        int h, w;
        float cq[3];
        if (!gs_project_point_hw_q(cams[v], p0, p1, p2, cb.H, cb.W, cb.u_hi, cb.v_hi, h, w, cq)) continue;
        const float z = cq[2];
        const float* D = q.depth + (int64_t)(v0 + v) * q.stride_view;
        const float d = D[(int64_t)h * cb.W + w];
        if (!(d > 0.0f)) continue;
        if (!((d - z) > cb.margin)) continue;
        bool viol = true;
        if (win > 0) {
          // the (2 window + 1)^2 square around (h, w), clipped to the image (h, w are inside it)
          const int h0 = h - win < 0 ? 0 : h - win, h1 = h + win > cb.H - 1 ? cb.H - 1 : h + win;
          const int w0 = w - win < 0 ? 0 : w - win, w1 = w + win > cb.W - 1 ? cb.W - 1 : w + win;
          for (int hh = h0; hh <= h1 && viol; ++hh)
            for (int ww = w0; ww <= w1; ++ww) {
              if (hh == h && ww == w) continue;   // (the centre has been tested)
              const float dd = D[(int64_t)hh * cb.W + ww];
              if (dd > 0.0f && !((dd - z) > cb.margin)) {
                viol = false;
                break;
              }
            }
        }
        count += viol ? 1 : 0;
      }
    }
  }
  if (r >= q.n.host) return;
  if (q.violations) q.violations[r] = count;   // (count is 0 for rows at or beyond the device count)
  if (q.keep) q.keep[r] = (live && count < cb.min_views) ? 1 : 0;
}

extern "C" int gs_free_space_dc_f32(const gs_carve_seq* seqs_host, int B, int L, int H, int W, float margin, int window,
                                    int min_views, void* stream) {
  GS_REQUIRE(seqs_host && B > 0 && L > 0 && H > 0 && W > 0, "bad arguments (NULL descriptors or B, L, H, W <= 0)");
  GS_REQUIRE((int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  GS_REQUIRE(margin >= 0.0f && margin < INFINITY, "margin must be finite and >= 0");
  GS_REQUIRE(window >= 0 && window <= GS_CV_MAX_WINDOW, "window must be 0, 1, 2 or 3");
  GS_REQUIRE(min_views >= 1, "min_views must be >= 1");
  for (int b = 0; b < B; ++b) {
    const gs_carve_seq& u = seqs_host[b];
    GS_REQUIRE(u.map.n_bound >= 0, "negative n_bound");
    GS_REQUIRE(u.map.n_bound < (1ll << 32), "maps of 2^32 rows or more are not supported (blocks of 8 sequences must fit one grid)");
    GS_REQUIRE(u.depth && u.poses16 && u.K16, "NULL pointer (depth, poses16, K16)");
    GS_REQUIRE(u.depth_stride_view >= 0, "negative depth_stride_view");
    // (an empty map may come without buffers: nothing of it is read or written)
    GS_REQUIRE(u.violations || u.keep || u.map.n_bound == 0, "NULL pointer (violations and keep: at least one output is needed)");
    GS_REQUIRE(u.map.points || u.map.n_bound == 0, "NULL pointer (points)");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    CvBatch cb = {};
    cb.B = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    cb.L = L; cb.H = H; cb.W = W;
    cb.window = window; cb.min_views = min_views; cb.margin = margin;
    cb.u_hi = (float)((double)W - 0.999); cb.v_hi = (float)((double)H - 0.999);
    int64_t n_max = 0;
    for (int b = 0; b < cb.B; ++b) {
      const gs_carve_seq& u = seqs_host[c0 + b];
      CvSeq& s = cb.s[b];
      s.points = u.map.points;
      s.n = GsCount{u.map.n_bound, u.map.n_dev};
      s.depth = u.depth;
      s.stride_view = u.depth_stride_view;
      s.poses16 = u.poses16;
      s.K16 = u.K16;
      s.violations = u.violations;
      s.keep = u.keep;
      n_max = u.map.n_bound > n_max ? u.map.n_bound : n_max;
    }
    if (n_max == 0) continue;
    const unsigned blocks = (unsigned)cb.B * (unsigned)gs_ceil_div(n_max, 256);   // < 8 * 2^24
    hipLaunchKernelGGL(gs_free_space_kernel, dim3(blocks), dim3(256), 0, st, cb);
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}
