// gs_render.hip — the model view: a surfel map seen from a pose as depth / colour / normal / confidence / index
// images, and its reverse mode (at the end of the file).  The forward is a z-buffered point render in two passes:
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
//
// With per-surfel radii (gs_render_map_radii_dc_f32, gs_render_map_radii_backward_dc_f32) the half-width of the square
// a row competes for is its own, from its radius rho (metres; a fused map attribute) and its depth in the view:
//   fbar = 0.5f * (K[0][0] + K[1][1])
//   x    = (rho * fbar) / q2                  float32, two operations
//   r    = rho > 0 and 0 < x < inf ? min(max_radius, (int)floorf(x)) : 0        (max_radius 0 .. 8)
// Everything else is the pass above: the same key, the same atomicMin, the same resolve pass.  With every r equal to
// k <= 3 the key image, hence every output, is that of radius = k.
#include "gs_assoc_dev.h"

// Build-time switch for measurements (tools/render_profile.py): 0 = every candidate issues its atomic.
#ifndef GS_RENDER_PRECHECK
#define GS_RENDER_PRECHECK 1
#endif

constexpr int GS_RV_MAX_VIEWS = 4;   // views of one map served by one launch (one camera each in LDS); more views = more launches
constexpr int GS_RV_MAX_RADIUS = 3;
constexpr int GS_RV_MAX_SPLAT = 8;   // cap of a per-surfel radius in pixels (the radii entries)
constexpr uint64_t GS_RV_EMPTY = ~0ull;

struct RvSeq {
  const float* points;
  const float* normals;
  const float* colors;
  const float* ccounts;
  const float* radii;     // (rows) metres, the radii entries only
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
  int B, V, H, W, radius, cull, use_conf;   // radius: the radii entries' max_radius
  int64_t P;
  float u_hi, v_hi, min_conf;
};

// the half-width in pixels of the square of a row of radius rho (metres) at camera-frame depth q2 > 0 in view c
GS_DEV int rv_splat_radius(const GsCamera& c, float rho, float q2, int max_radius) {
  const float fbar = 0.5f * (c.K[0] + c.K[5]);
  const float x = (rho * fbar) / q2;
  if (!(rho > 0.0f && x > 0.0f && x < INFINITY)) return 0;
  return x >= (float)max_radius ? max_radius : (int)x;   // x > 0: the cast is floorf
}

// one candidate pixel of a row: lower its key to the row's
GS_DEV void rv_compete(unsigned long long* a, unsigned long long key) {
#if GS_RENDER_PRECHECK
  // Plain load first: a pixel's key only ever decreases during the pass, so a stale value (an older line in this
  // CU's cache) is never below the current one -- it can let a redundant atomic through, never skip one that
  // would have lowered the key.  Most rows of a dense map lose to a surfel in front of them and stop here.
  if (*a <= key) return;
#endif
  atomicMin(a, key);
}

template <bool RADII>
GS_DEV void rv_key_body(const RvBatch& rb) {
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
  float rho = 0.0f;
  if (RADII) rho = q.radii[n];
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
    const int r = RADII ? rv_splat_radius(c, rho, cq[2], rb.radius) : rb.radius;
    const unsigned long long key = ((unsigned long long)__float_as_uint(cq[2]) << 32) | (unsigned long long)(uint32_t)n;
    unsigned long long* kv = reinterpret_cast<unsigned long long*>(q.keys) + (int64_t)v * rb.P;
    if (RADII) {
      // r differs from lane to lane.  The loops run over the offsets of the widest square among the wave's lanes that
      // are still here -- bounds and counters the whole wave shares, in scalar registers -- and a lane sits out the
      // offsets beyond its own r or outside the image: the trips a wave makes are those of its widest lane either way.
      int rw = 0;
      for (int k = 1; k <= rb.radius; ++k)
        if (__ballot(r >= k) != 0ull) rw = k;
      for (int dh = -rw; dh <= rw; ++dh)
        for (int dw = -rw; dw <= rw; ++dw) {
          const int reach = (dh < 0 ? -dh : dh) > (dw < 0 ? -dw : dw) ? (dh < 0 ? -dh : dh) : (dw < 0 ? -dw : dw);
          const int hh = h + dh, ww = w + dw;
          if (reach > r || hh < 0 || hh >= rb.H || ww < 0 || ww >= rb.W) continue;
          rv_compete(kv + ((int64_t)hh * rb.W + ww), key);
        }
      continue;
    }
    // the (2r+1)^2 square around (h, w), clipped to the image (h, w are inside it)
    const int h0 = h - r < 0 ? 0 : h - r, h1 = h + r > rb.H - 1 ? rb.H - 1 : h + r;
    const int w0 = w - r < 0 ? 0 : w - r, w1 = w + r > rb.W - 1 ? rb.W - 1 : w + r;
    for (int hh = h0; hh <= h1; ++hh)
      for (int ww = w0; ww <= w1; ++ww) rv_compete(kv + ((int64_t)hh * rb.W + ww), key);
  }
}

__global__ void __launch_bounds__(256) gs_render_key_kernel(const RvBatch rb) { rv_key_body<false>(rb); }
// (named gs_rview_*: see the note on names in front of the reverse mode)
__global__ void __launch_bounds__(256) gs_rview_radii_key_kernel(const RvBatch rb) { rv_key_body<true>(rb); }

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

// what is wrong with the arguments of a forward entry, or NULL (radii_host: NULL for the plain entry)
static const char* rv_check(const gs_render_seq* seqs_host, const float* const* radii_host, bool with_radii, int B, int L,
                            int H, int W, int radius, float min_confidence, int cull_backfaces) {
  if (!(seqs_host && B > 0 && L > 0 && H > 0 && W > 0)) return "bad arguments";
  if (!((int64_t)H * W < (1ll << 31))) return "image too large for int32 pixel ids";
  if (with_radii) {
    if (!radii_host) return "NULL pointer (radii)";
    if (!(radius >= 0 && radius <= GS_RV_MAX_SPLAT)) return "max_radius must be 0 ... 8";
  } else if (!(radius >= 0 && radius <= GS_RV_MAX_RADIUS)) {
    return "radius must be 0, 1, 2 or 3";
  }
  if (min_confidence != min_confidence) return "min_confidence is NaN";
  const bool use_conf = min_confidence > 0.0f;
  for (int b = 0; b < B; ++b) {
    const gs_render_seq& u = seqs_host[b];
    if (!(u.map.n_bound >= 0)) return "bad map size";
    if (!(u.map.n_bound < (1ll << 32))) return "maps of 2^32 rows or more are not supported (32-bit row index in the key)";
    if (!(u.poses16 && u.K16 && u.scratch)) return "NULL pointer";
    if (u.map.n_bound > 0) {
      if (!u.map.points) return "NULL pointer (points)";
      if (!(u.map.normals || !(u.normal || cull_backfaces)))
        return "NULL pointer (normals: needed by the normal image and by cull_backfaces)";
      if (!(u.map.colors || !u.color)) return "NULL pointer (colors: needed by the colour image)";
      if (!(u.map.ccounts || !(u.confidence || use_conf)))
        return "NULL pointer (ccounts: needed by the confidence image and by min_confidence)";
      if (with_radii && !radii_host[b]) return "NULL pointer (radii of a sequence)";
    }
  }
  return nullptr;
}

// the launches of a forward entry over checked arguments; radii_host NULL: the plain key pass, `radius` for every row
static int gs_render_map_launch(const gs_render_seq* seqs_host, const float* const* radii_host, int B, int L, int H, int W,
                                int radius, float min_confidence, int cull_backfaces, void* stream) {
  const bool use_conf = min_confidence > 0.0f;
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
        s.radii = radii_host ? radii_host[c0 + b] : nullptr;
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
        if (radii_host)
          hipLaunchKernelGGL(gs_rview_radii_key_kernel, dim3(blocks), dim3(256), 0, st, rb);
        else
          hipLaunchKernelGGL(gs_render_key_kernel, dim3(blocks), dim3(256), 0, st, rb);
      }
      const unsigned pblocks = (unsigned)nb * (unsigned)gs_ceil_div((int64_t)rb.V * P, 256);
      hipLaunchKernelGGL(gs_render_resolve_kernel, dim3(pblocks), dim3(256), 0, st, rb);
      GS_LAUNCH_CHECK();
    }
  }
  return GS_OK;
}

extern "C" int gs_render_map_dc_f32(const gs_render_seq* seqs_host, int B, int L, int H, int W, int radius,
                                    float min_confidence, int cull_backfaces, void* stream) {
  const char* bad = rv_check(seqs_host, nullptr, false, B, L, H, W, radius, min_confidence, cull_backfaces);
  GS_REQUIRE(!bad, bad);
  return gs_render_map_launch(seqs_host, nullptr, B, L, H, W, radius, min_confidence, cull_backfaces, stream);
}

// The model view with per-surfel radii: radii_host[b] is a device array of map.n_bound floats (metres) for sequence b.
extern "C" int gs_render_map_radii_dc_f32(const gs_render_seq* seqs_host, const float* const* radii_host, int B, int L,
                                          int H, int W, int max_radius, float min_confidence, int cull_backfaces,
                                          void* stream) {
  const char* bad = rv_check(seqs_host, radii_host, true, B, L, H, W, max_radius, min_confidence, cull_backfaces);
  GS_REQUIRE(!bad, bad);
  return gs_render_map_launch(seqs_host, radii_host, B, L, H, W, max_radius, min_confidence, cull_backfaces, stream);
}

// ---------------------------------------------------------------- reverse mode of the model view ----
// The winner of a pixel (the index image of the forward) and the two filters are constants; gradients flow through the
// values the resolve pass writes for the winner (T = [R t; 0 1] camera-to-world, row n wins pixel i of view v, upstream
// adjoints zb / cb(3) / ob(3) / fb):
//   depth   z   = sum_k R[k][2] (p_k - t_k):  points_bar[n][k] += R[k][2] zb,  T_bar[k][2] += (p_k - t_k) zb,
//                                             T_bar[k][3] -= R[k][2] zb
//   normal  o_j = sum_k n_k R[k][j]:          normals_bar[n][k] += sum_j R[k][j] ob_j,  T_bar[k][j] += n_k ob_j
//   colour, confidence: copies:               colors_bar[n] += cb,  ccounts_bar[n] += fb
// A row-centric gather, no float atomics: one thread per map row re-projects its row under every view of the launch
// (gs_project_point_hw_q: the forward's arithmetic, hence the forward's (h, w)), scans the clipped (2 radius + 1)^2 square
// of the saved index image for pixels it won (raster order) and adds up their adjoints in float64; every row of the four
// row outputs is written exactly once per launch (zeros for rows that win nothing or lie beyond the count: no memset).
// A row that the forward filtered out is in no pixel of the index image and needs no test here.  Upstream images are
// read only at pixels some row won: whatever they hold at empty pixels (index -1) never enters.
// Pose adjoint: each thread holds its row's 12 contributions to T_bar of a view (3x3 part, then the translation column),
// a block reduction (float64, fixed order) writes one partial row per block and view to the caller's scratch, and a
// second launch adds the partial rows up in a fixed order.  Views beyond GS_RV_MAX_VIEWS are served by further launches
// on the same stream that add to the row outputs of the launches before them (read back as the float32 values they
// were rounded to: one more rounding per group of 4 views): a fixed order as well, so every output
// is a pure function of the inputs (bitwise reproducible; T_bar of a view does not depend on the other views).
// (The kernels are named gs_rview_*: "gs_render_" stays the prefix of the two forward passes, whose register budget
// tests/test_render_cpu.py pins by that prefix.)
constexpr int GS_RB_NV = 12;

struct RbSeq {
  const float* points;
  const float* normals;
  const float* radii;     // (rows) metres, the radii entry only
  GsCount n;
  int64_t rows;           // rows of the four row outputs (= the host-side bound of the map)
  int nblk;               // blocks of 256 rows
  const float* poses16;   // first view of the launch
  const float* K16;
  const int64_t* index;   // (views of the launch, H * W) ...
  const float* zb;        // ... upstream adjoints, any may be NULL
  const float* cb;
  const float* ob;
  const float* fb;
  float* points_bar;      // (rows, 3), any may be NULL
  float* normals_bar;
  float* colors_bar;
  float* ccounts_bar;     // (rows)
  double* partials;       // (views of the launch, nblk, 12); NULL: no pose adjoint
  float* poses_bar;       // first view of the launch
};
struct RbBatch {
  RbSeq s[GS_MAX_BATCH];
  int B, V, H, W, radius, accumulate;   // radius: the radii entry's max_radius
  int64_t P;
  float u_hi, v_hi;
};

template <bool RADII>
GS_DEV void rv_backward_rows_body(const RbBatch& rb) {
  __shared__ GsCamera cams[GS_RV_MAX_VIEWS];
  __shared__ float trans[GS_RV_MAX_VIEWS][3];
  __shared__ double red[GS_RV_MAX_VIEWS][256 / GS_WAVE][GS_RB_NV];
  const RbSeq& q = rb.s[blockIdx.x % rb.B];
  const int blk = blockIdx.x / rb.B;
  if (blk >= q.nblk) return;   // (the whole block: a shorter map of the batch)
  if ((int)threadIdx.x < rb.V) {
    const float* T = q.poses16 + 16 * threadIdx.x;
    cams[threadIdx.x] = gs_camera(T, q.K16);
    trans[threadIdx.x][0] = T[3];
    trans[threadIdx.x][1] = T[7];
    trans[threadIdx.x][2] = T[11];
  }
  __syncthreads();
  const int lane = threadIdx.x & (GS_WAVE - 1), wave = threadIdx.x / GS_WAVE;
  const int64_t n = (int64_t)blk * 256 + threadIdx.x;
  const bool live = n < gs_count(q.n);
  const bool want_n = q.ob != nullptr && q.normals != nullptr;
  float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
  if (live) {
    p0 = q.points[3 * n];
    p1 = q.points[3 * n + 1];
    p2 = q.points[3 * n + 2];
    if (want_n) {
      n0 = q.normals[3 * n];
      n1 = q.normals[3 * n + 1];
      n2 = q.normals[3 * n + 2];
    }
  }
  float rho = 0.0f;
  if (RADII && live) rho = q.radii[n];
  double aP[3] = {0.0, 0.0, 0.0}, aN[3] = {0.0, 0.0, 0.0}, aC[3] = {0.0, 0.0, 0.0}, aF = 0.0;
  for (int v = 0; v < rb.V; ++v) {
    const GsCamera& c = cams[v];
    double Z = 0.0, O[3] = {0.0, 0.0, 0.0};
    bool won = false;
    int h, w;
    float cq[3];
    if (live && gs_project_point_hw_q(c, p0, p1, p2, rb.H, rb.W, rb.u_hi, rb.v_hi, h, w, cq)) {
      const int64_t base = (int64_t)v * rb.P;
      const int r = RADII ? rv_splat_radius(c, rho, cq[2], rb.radius) : rb.radius;   // (the forward's r)
      const int h0 = h - r < 0 ? 0 : h - r, h1 = h + r > rb.H - 1 ? rb.H - 1 : h + r;
      const int w0 = w - r < 0 ? 0 : w - r, w1 = w + r > rb.W - 1 ? rb.W - 1 : w + r;
      for (int hh = h0; hh <= h1; ++hh)
        for (int ww = w0; ww <= w1; ++ww) {
          const int64_t i = base + ((int64_t)hh * rb.W + ww);
          if (q.index[i] != n) continue;
          won = true;
          if (q.zb) Z += (double)q.zb[i];
          if (want_n) {
            O[0] += (double)q.ob[3 * i];
            O[1] += (double)q.ob[3 * i + 1];
            O[2] += (double)q.ob[3 * i + 2];
          }
          if (q.cb) {
            aC[0] += (double)q.cb[3 * i];
            aC[1] += (double)q.cb[3 * i + 1];
            aC[2] += (double)q.cb[3 * i + 2];
          }
          if (q.fb) aF += (double)q.fb[i];
        }
    }
    // R[k][j] = Ri[3 j + k]
    if (won) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        aP[k] += (double)c.Ri[6 + k] * Z;
        aN[k] += ((double)c.Ri[k] * O[0] + (double)c.Ri[3 + k] * O[1]) + (double)c.Ri[6 + k] * O[2];
      }
    }
    if (q.partials) {
      double t[GS_RB_NV];
#pragma unroll
      for (int i = 0; i < GS_RB_NV; ++i) t[i] = 0.0;
      if (won) {
        const double pn[3] = {(double)n0, (double)n1, (double)n2};
        const double pt[3] = {(double)p0 - (double)trans[v][0], (double)p1 - (double)trans[v][1],
                              (double)p2 - (double)trans[v][2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          t[3 * k] = pn[k] * O[0];
          t[3 * k + 1] = pn[k] * O[1];
          t[3 * k + 2] = pn[k] * O[2] + pt[k] * Z;
          t[9 + k] = -((double)c.Ri[6 + k] * Z);
        }
      }
      // a wave none of whose rows won a pixel of this view contributes exact zeros: skip its shuffles
      const bool any = __ballot(won) != 0ull;
#pragma unroll
      for (int i = 0; i < GS_RB_NV; ++i) {
        const double sum = any ? gs_wave_sum_f64(t[i]) : 0.0;
        if (lane == 0) red[v][wave][i] = sum;
      }
    }
  }
  if (q.partials) {
    __syncthreads();
    if ((int)threadIdx.x < GS_RB_NV * rb.V) {
      const int v = threadIdx.x / GS_RB_NV, i = threadIdx.x % GS_RB_NV;
      double t = 0.0;
      for (int wv = 0; wv < 256 / GS_WAVE; ++wv) t += red[v][wv][i];
      q.partials[((int64_t)v * q.nblk + blk) * GS_RB_NV + i] = t;
    }
  }
  if (n >= q.rows) return;
  if (rb.accumulate) {   // a later launch of the same call: add to what the views before left
    if (q.points_bar)
      for (int k = 0; k < 3; ++k) aP[k] += (double)q.points_bar[3 * n + k];
    if (q.normals_bar)
      for (int k = 0; k < 3; ++k) aN[k] += (double)q.normals_bar[3 * n + k];
    if (q.colors_bar)
      for (int k = 0; k < 3; ++k) aC[k] += (double)q.colors_bar[3 * n + k];
    if (q.ccounts_bar) aF += (double)q.ccounts_bar[n];
  }
  if (q.points_bar)
    for (int k = 0; k < 3; ++k) q.points_bar[3 * n + k] = (float)aP[k];
  if (q.normals_bar)
    for (int k = 0; k < 3; ++k) q.normals_bar[3 * n + k] = (float)aN[k];
  if (q.colors_bar)
    for (int k = 0; k < 3; ++k) q.colors_bar[3 * n + k] = (float)aC[k];
  if (q.ccounts_bar) q.ccounts_bar[n] = (float)aF;
}

__global__ void __launch_bounds__(256) gs_rview_backward_rows_kernel(const RbBatch rb) { rv_backward_rows_body<false>(rb); }
__global__ void __launch_bounds__(256) gs_rview_radii_backward_rows_kernel(const RbBatch rb) {
  rv_backward_rows_body<true>(rb);
}

// One wave per (sequence, view) adds the partial rows up (rows strided over the lanes, then across the lanes: a fixed
// order) and writes the 4x4 pose adjoint, bottom row zero.
__global__ void __launch_bounds__(GS_WAVE) gs_rview_backward_pose_kernel(const RbBatch rb) {
  const RbSeq& q = rb.s[blockIdx.y];
  if (!q.partials || !q.poses_bar) return;
  const int v = blockIdx.x, lane = threadIdx.x;
  const double* part = q.partials + (int64_t)v * q.nblk * GS_RB_NV;
  float* out = q.poses_bar + 16 * v;
  for (int i = 0; i < GS_RB_NV; ++i) {
    double s = 0.0;
    for (int b = lane; b < q.nblk; b += GS_WAVE) s += part[(int64_t)b * GS_RB_NV + i];
    s = gs_wave_sum_f64(s);
    if (lane == 0) out[i < 9 ? 4 * (i / 3) + i % 3 : 4 * (i - 9) + 3] = (float)s;
  }
  if (lane < 4) out[12 + lane] = 0.0f;
}

static size_t render_backward_scratch_per_seq(int views, int64_t n_bound) {
  const int v = views < GS_RV_MAX_VIEWS ? views : GS_RV_MAX_VIEWS;
  return gs_align((size_t)v * (size_t)gs_ceil_div(n_bound, 256) * GS_RB_NV * sizeof(double)) + 256;
}

extern "C" int64_t gs_render_backward_scratch_bytes(int views, int H, int W, int64_t n_bound) {
  if (views <= 0 || H <= 0 || W <= 0 || n_bound < 0 || n_bound >= (1ll << 32)) return 0;
  return (int64_t)render_backward_scratch_per_seq(views, n_bound);
}

static const char* rb_check(const gs_render_backward_seq* seqs_host, const float* const* radii_host, bool with_radii,
                            int B, int L, int H, int W, int radius) {
  if (!(seqs_host && B > 0 && L > 0 && H > 0 && W > 0)) return "bad arguments";
  if (!((int64_t)H * W < (1ll << 31))) return "image too large for int32 pixel ids";
  if (with_radii) {
    if (!radii_host) return "NULL pointer (radii)";
    if (!(radius >= 0 && radius <= GS_RV_MAX_SPLAT)) return "max_radius must be 0 ... 8";
  } else if (!(radius >= 0 && radius <= GS_RV_MAX_RADIUS)) {
    return "radius must be 0, 1, 2 or 3";
  }
  for (int b = 0; b < B; ++b) {
    const gs_render_backward_seq& u = seqs_host[b];
    if (!(u.map.n_bound >= 0)) return "bad map size";
    if (!(u.map.n_bound < (1ll << 32))) return "maps of 2^32 rows or more are not supported (32-bit row index in the key)";
    if (!(u.poses16 && u.K16 && u.index)) return "NULL pointer";
    if (!(!u.poses_bar || u.scratch)) return "NULL pointer (scratch: needed by poses_bar)";
    if (u.map.n_bound > 0) {
      if (!u.map.points) return "NULL pointer (points)";
      if (!(u.map.normals || !u.normal_bar)) return "NULL pointer (normals: needed by the terms of normal_bar)";
      if (with_radii && !radii_host[b]) return "NULL pointer (radii of a sequence)";
    }
  }
  return nullptr;
}

static int gs_render_map_backward_launch(const gs_render_backward_seq* seqs_host, const float* const* radii_host, int B,
                                         int L, int H, int W, int radius, void* stream) {
  hipStream_t st = gs_stream(stream);
  const int64_t P = (int64_t)H * W;
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    for (int v0 = 0; v0 < L; v0 += GS_RV_MAX_VIEWS) {
      RbBatch rb;
      rb.B = nb;
      rb.V = L - v0 < GS_RV_MAX_VIEWS ? L - v0 : GS_RV_MAX_VIEWS;
      rb.H = H; rb.W = W; rb.P = P;
      rb.radius = radius;
      rb.accumulate = v0 > 0 ? 1 : 0;
      rb.u_hi = (float)((double)W - 0.999); rb.v_hi = (float)((double)H - 0.999);
      int64_t n_max = 0;
      bool any_pose = false;
      const int64_t off = (int64_t)v0 * P;   // first pixel of the launch in the (L, H, W) stacks
      for (int b = 0; b < nb; ++b) {
        const gs_render_backward_seq& u = seqs_host[c0 + b];
        RbSeq& s = rb.s[b];
        s.points = u.map.points; s.normals = u.map.normals;
        s.radii = radii_host ? radii_host[c0 + b] : nullptr;
        s.n = GsCount{u.map.n_bound, u.map.n_dev};
        s.rows = u.map.n_bound;
        s.nblk = (int)gs_ceil_div(u.map.n_bound, 256);   // < 2^24
        s.poses16 = u.poses16 + 16 * (int64_t)v0;
        s.K16 = u.K16;
        s.index = u.index + off;
        s.zb = u.depth_bar ? u.depth_bar + off : nullptr;
        s.cb = u.color_bar ? u.color_bar + 3 * off : nullptr;
        s.ob = u.normal_bar ? u.normal_bar + 3 * off : nullptr;
        s.fb = u.confidence_bar ? u.confidence_bar + off : nullptr;
        s.points_bar = u.points_bar; s.normals_bar = u.normals_bar;
        s.colors_bar = u.colors_bar; s.ccounts_bar = u.ccounts_bar;
        s.partials = u.poses_bar ? static_cast<double*>(u.scratch) : nullptr;
        s.poses_bar = u.poses_bar ? u.poses_bar + 16 * (int64_t)v0 : nullptr;
        any_pose = any_pose || u.poses_bar;
        n_max = u.map.n_bound > n_max ? u.map.n_bound : n_max;
      }
      if (n_max > 0) {
        const unsigned blocks = (unsigned)nb * (unsigned)gs_ceil_div(n_max, 256);   // < 8 * 2^24
        if (radii_host)
          hipLaunchKernelGGL(gs_rview_radii_backward_rows_kernel, dim3(blocks), dim3(256), 0, st, rb);
        else
          hipLaunchKernelGGL(gs_rview_backward_rows_kernel, dim3(blocks), dim3(256), 0, st, rb);
      }
      if (any_pose) hipLaunchKernelGGL(gs_rview_backward_pose_kernel, dim3(rb.V, nb), dim3(GS_WAVE), 0, st, rb);
      GS_LAUNCH_CHECK();
    }
  }
  return GS_OK;
}

extern "C" int gs_render_map_backward_dc_f32(const gs_render_backward_seq* seqs_host, int B, int L, int H, int W,
                                             int radius, void* stream) {
  const char* bad = rb_check(seqs_host, nullptr, false, B, L, H, W, radius);
  GS_REQUIRE(!bad, bad);
  return gs_render_map_backward_launch(seqs_host, nullptr, B, L, H, W, radius, stream);
}

// Reverse mode of gs_render_map_radii_dc_f32: the radii are a constant of the gradient (they only say which pixels a
// row could have won); radii_host and max_radius must be those of the forward call.
extern "C" int gs_render_map_radii_backward_dc_f32(const gs_render_backward_seq* seqs_host, const float* const* radii_host,
                                                   int B, int L, int H, int W, int max_radius, void* stream) {
  const char* bad = rb_check(seqs_host, radii_host, true, B, L, H, W, max_radius);
  GS_REQUIRE(!bad, bad);
  return gs_render_map_backward_launch(seqs_host, radii_host, B, L, H, W, max_radius, stream);
}
