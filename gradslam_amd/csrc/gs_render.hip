// gs_render.hip — the model view: a surfel map seen from a pose as depth / colour / normal / confidence / index
// images (forward only).  A z-buffered point render in two passes:
//
//   key pass      one thread per map row: project the row under every view of the launch (the projection of the
//                 association, gs_project_point_hw_q) and let it compete for its pixel(s) with a 64-bit atomicMin on
//                 key = (bits(z) << 32) | row.  z > 0, so the unsigned order of the bits is the order of the floats,
//                 and the row index in the low word settles equal depths towards the lowest row: the minimum of a set
//                 does not depend on the order of arrival, so the images are a pure function of the inputs.
//   resolve pass  one thread per pixel: decode the key, gather the winner's attributes, write the five images.
//
// The key image (8 B per pixel and view) lives in the caller's scratch and is set to "empty" (all ones: no row can
// produce it, bits(z) <= bits(+inf)) by a memset in front of the key pass: the scratch then carries no state from call
// to call (a resolve pass that left it cleared for the next call would save 8 B per pixel of a pass that moves 56, and
// would make every call depend on who used the scratch before).
//
// Arithmetic (-ffp-contract=off, every FMA spelled out; tests/render_ref.py restates it with the oracle):
//   q      = camera-frame point of gs_project_point_hw_q: q_j = fma(p2, Ri[3j+2], fma(p1, Ri[3j+1], p0 * Ri[3j])) + ti[j]
//   z      = q[2]
//   nc     = camera-frame normal, no translation: nc_j = fma(n2, Ri[3j+2], fma(n1, Ri[3j+1], n0 * Ri[3j]))
//   back-face test (cull_backfaces): d = (nc0 * q0 + nc1 * q1) + nc2 * q2, one rounding per operation, left to right;
//            the row is skipped when d >= 0 (it faces away from the camera or is seen edge-on)
//   min_confidence: the row is skipped when ccount < min_confidence
#include "gs_assoc_dev.h"

// Build-time switch for measurements (tools/render_profile.py): 0 = every candidate issues its atomic.
#ifndef GS_RENDER_PRECHECK
#define GS_RENDER_PRECHECK 1
#endif

constexpr int GS_RV_MAX_VIEWS = 4;   // views of one map served by one launch (one camera each in LDS); more views = more launches
constexpr int GS_RV_MAX_RADIUS = 3;
constexpr uint64_t GS_RV_EMPTY = ~0ull;

struct RvSeq {
  const float* points;
  const float* normals;
  const float* colors;
  const float* ccounts;
  GsCount n;
  const float* poses16;   // first view of the launch
  const float* K16;
  uint64_t* keys;         // (views of the launch, H * W)
  float* depth;           // outputs: first view of the launch; any may be NULL
  float* color;
  float* normal;
  float* conf;
  int64_t* index;
};
struct RvBatch {
  RvSeq s[GS_MAX_BATCH];
  int B, V, H, W, radius, cull, use_conf;
  int64_t P;
  float u_hi, v_hi, min_conf;
};

__global__ void __launch_bounds__(256) gs_render_key_kernel(const RvBatch rb) {
  __shared__ GsCamera cams[GS_RV_MAX_VIEWS];
  const RvSeq& q = rb.s[blockIdx.x % rb.B];
  if ((int)threadIdx.x < rb.V) cams[threadIdx.x] = gs_camera(q.poses16 + 16 * threadIdx.x, q.K16);
  __syncthreads();
  const int64_t n = (int64_t)(blockIdx.x / rb.B) * 256 + threadIdx.x;
  if (n >= gs_count(q.n)) return;
  if (rb.use_conf && q.ccounts[n] < rb.min_conf) return;
  const float p0 = q.points[3 * n], p1 = q.points[3 * n + 1], p2 = q.points[3 * n + 2];
  float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
  if (rb.cull) {
    n0 = q.normals[3 * n];
    n1 = q.normals[3 * n + 1];
    n2 = q.normals[3 * n + 2];
  }
  const int r = rb.radius;
  for (int v = 0; v < rb.V; ++v) {
    const GsCamera& c = cams[v];
    int h, w;
    float cq[3];
    if (!gs_project_point_hw_q(c, p0, p1, p2, rb.H, rb.W, rb.u_hi, rb.v_hi, h, w, cq)) continue;
    if (rb.cull) {
      const float nc0 = gs_dot3_fma(n0, n1, n2, c.Ri[0], c.Ri[1], c.Ri[2]);
      const float nc1 = gs_dot3_fma(n0, n1, n2, c.Ri[3], c.Ri[4], c.Ri[5]);
      const float nc2 = gs_dot3_fma(n0, n1, n2, c.Ri[6], c.Ri[7], c.Ri[8]);
      if (gs_dot3_plain(nc0, nc1, nc2, cq[0], cq[1], cq[2]) >= 0.0f) continue;
    }
    const unsigned long long key = ((unsigned long long)__float_as_uint(cq[2]) << 32) | (unsigned long long)(uint32_t)n;
    unsigned long long* kv = reinterpret_cast<unsigned long long*>(q.keys) + (int64_t)v * rb.P;
    // the (2r+1)^2 square around (h, w), clipped to the image (h, w are inside it)
    const int h0 = h - r < 0 ? 0 : h - r, h1 = h + r > rb.H - 1 ? rb.H - 1 : h + r;
    const int w0 = w - r < 0 ? 0 : w - r, w1 = w + r > rb.W - 1 ? rb.W - 1 : w + r;
    for (int hh = h0; hh <= h1; ++hh)
      for (int ww = w0; ww <= w1; ++ww) {
        unsigned long long* a = kv + ((int64_t)hh * rb.W + ww);
#if GS_RENDER_PRECHECK
        // Plain load first: a pixel's key only ever decreases during the pass, so a stale value (an older line in this
        // CU's cache) is never below the current one -- it can let a redundant atomic through, never skip one that
        // would have lowered the key.  Most rows of a dense map lose to a surfel in front of them and stop here.
        if (*a <= key) continue;
#endif
        atomicMin(a, key);
      }
  }
}

__global__ void __launch_bounds__(256) gs_render_resolve_kernel(const RvBatch rb) {
  const RvSeq& q = rb.s[blockIdx.x % rb.B];
  const int64_t i = (int64_t)(blockIdx.x / rb.B) * 256 + threadIdx.x;   // pixel of the (V, H, W) stack of the launch
  if (i >= (int64_t)rb.V * rb.P) return;
  const uint64_t key = q.keys[i];
  const bool hit = key != GS_RV_EMPTY;
  const int64_t row = (int64_t)(uint32_t)key;
  if (q.depth) q.depth[i] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
  if (q.index) q.index[i] = hit ? row : (int64_t)-1;
  if (q.conf) q.conf[i] = hit ? q.ccounts[row] : 0.0f;
  if (q.color) {
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (hit) {
      c0 = q.colors[3 * row];
      c1 = q.colors[3 * row + 1];
      c2 = q.colors[3 * row + 2];
    }
    q.color[3 * i] = c0;
    q.color[3 * i + 1] = c1;
    q.color[3 * i + 2] = c2;
  }
  if (q.normal) {
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if (hit) {
      // the winner's normal in the camera frame: rows of Ri = R^T of the view's pose (as GsCamera::Ri)
      const float* T = q.poses16 + 16 * (i / rb.P);
      const float n0 = q.normals[3 * row], n1 = q.normals[3 * row + 1], n2 = q.normals[3 * row + 2];
      o0 = gs_dot3_fma(n0, n1, n2, T[0], T[4], T[8]);
      o1 = gs_dot3_fma(n0, n1, n2, T[1], T[5], T[9]);
      o2 = gs_dot3_fma(n0, n1, n2, T[2], T[6], T[10]);
    }
    q.normal[3 * i] = o0;
    q.normal[3 * i + 1] = o1;
    q.normal[3 * i + 2] = o2;
  }
}

static size_t render_scratch_per_seq(int views, int H, int W) {
  const int v = views < GS_RV_MAX_VIEWS ? views : GS_RV_MAX_VIEWS;
  return gs_align((size_t)v * (size_t)H * (size_t)W * sizeof(uint64_t));
}

extern "C" int64_t gs_render_scratch_bytes(int views, int H, int W) {
  if (views <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  return (int64_t)render_scratch_per_seq(views, H, W);
}

extern "C" int gs_render_map_dc_f32(const gs_render_seq* seqs_host, int B, int L, int H, int W, int radius,
                                    float min_confidence, int cull_backfaces, void* stream) {
  GS_REQUIRE(seqs_host && B > 0 && L > 0 && H > 0 && W > 0, "bad arguments");
  GS_REQUIRE((int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  GS_REQUIRE(radius >= 0 && radius <= GS_RV_MAX_RADIUS, "radius must be 0, 1, 2 or 3");
  GS_REQUIRE(!(min_confidence != min_confidence), "min_confidence is NaN");
  const bool use_conf = min_confidence > 0.0f;
  for (int b = 0; b < B; ++b) {
    const gs_render_seq& u = seqs_host[b];
    GS_REQUIRE(u.map.n_bound >= 0, "bad map size");
    GS_REQUIRE(u.map.n_bound < (1ll << 32), "maps of 2^32 rows or more are not supported (32-bit row index in the key)");
    GS_REQUIRE(u.poses16 && u.K16 && u.scratch, "NULL pointer");
    if (u.map.n_bound > 0) {
      GS_REQUIRE(u.map.points, "NULL pointer (points)");
      GS_REQUIRE(u.map.normals || !(u.normal || cull_backfaces), "NULL pointer (normals: needed by the normal image and by cull_backfaces)");
      GS_REQUIRE(u.map.colors || !u.color, "NULL pointer (colors: needed by the colour image)");
      GS_REQUIRE(u.map.ccounts || !(u.confidence || use_conf), "NULL pointer (ccounts: needed by the confidence image and by min_confidence)");
    }
  }
  hipStream_t st = gs_stream(stream);
  const int64_t P = (int64_t)H * W;
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    for (int v0 = 0; v0 < L; v0 += GS_RV_MAX_VIEWS) {
      RvBatch rb;
      rb.B = nb;
      rb.V = L - v0 < GS_RV_MAX_VIEWS ? L - v0 : GS_RV_MAX_VIEWS;
      rb.H = H; rb.W = W; rb.P = P;
      rb.radius = radius; rb.cull = cull_backfaces ? 1 : 0; rb.use_conf = use_conf ? 1 : 0;
      rb.u_hi = (float)((double)W - 0.999); rb.v_hi = (float)((double)H - 0.999);
      rb.min_conf = min_confidence;
      int64_t n_max = 0;
      const int64_t off = (int64_t)v0 * P;   // first pixel of the launch in the (L, H, W) stacks
      for (int b = 0; b < nb; ++b) {
        const gs_render_seq& u = seqs_host[c0 + b];
        RvSeq& s = rb.s[b];
        s.points = u.map.points; s.normals = u.map.normals; s.colors = u.map.colors; s.ccounts = u.map.ccounts;
        s.n = GsCount{u.map.n_bound, u.map.n_dev};
        s.poses16 = u.poses16 + 16 * (int64_t)v0;
        s.K16 = u.K16;
        s.keys = static_cast<uint64_t*>(u.scratch);
        s.depth = u.depth ? u.depth + off : nullptr;
        s.color = u.color ? u.color + 3 * off : nullptr;
        s.normal = u.normal ? u.normal + 3 * off : nullptr;
        s.conf = u.confidence ? u.confidence + off : nullptr;
        s.index = u.index ? u.index + off : nullptr;
        n_max = u.map.n_bound > n_max ? u.map.n_bound : n_max;
        GS_HIP(hipMemsetAsync(u.scratch, 0xff, (size_t)rb.V * (size_t)P * sizeof(uint64_t), st));
      }
      if (n_max > 0) {
        const unsigned blocks = (unsigned)nb * (unsigned)gs_ceil_div(n_max, 256);   // < 8 * 2^24
        hipLaunchKernelGGL(gs_render_key_kernel, dim3(blocks), dim3(256), 0, st, rb);
      }
      const unsigned pblocks = (unsigned)nb * (unsigned)gs_ceil_div((int64_t)rb.V * P, 256);
      hipLaunchKernelGGL(gs_render_resolve_kernel, dim3(pblocks), dim3(256), 0, st, rb);
      GS_LAUNCH_CHECK();
    }
  }
  return GS_OK;
}
