// gs_picp_outliers.hip — the projective ICP's outlier mask: from the residuals of a converged solve to the image of the
// pixels that belong to something that moved (Keller et al., section "dynamics"; the KinectFusion descendants): the
// outliers of the solve, isolated ones dropped, the rest grown over similar neighbours.  Per sequence, at a float32 pose
// T, over EVERY pixel of the live frame (stride 1 whatever the solve's stride: the mask is a full image, the map update
// can use it); tests/outlier_mask_ref.py restates it operation by operation:
//
//   1  association   code, b of each pixel: pi_associate + gn_row_pn at T, the linearise kernel's own device functions
//                    (the bits of gs_projective_icp_rows_f32 at stride 1; with weights a masked pixel has code 6)
//   2  scale         med = the lower median of |b| over the code-0 pixels (gs_picp_scale.hip's residual pass and radix
//                    selection);  hi_t = max((float)hi * 1.4826f * med, floor), lo_t alike with lo: one float32 product
//                    for the constant, one with med, a product that is not above the floor gives the floor; +0.0
//                    without a code-0 pixel.  A threshold of 0 makes no pixel strong or eligible by its residual
//   3  classes       strong   = (code == 0 && |b| > hi_t && hi_t > 0) || code == 4 || code == 5
//                    eligible = strong || (code == 0 && |b| > lo_t && lo_t > 0)
//                    strict float32 comparisons; codes 1, 2, 3 and 6 have class 0.  Byte: bit 0 strong, bit 1 eligible
//   4  support       seed(p) = strong(p) and at least min_support of the 3 x 3 window around p are strong (p counts,
//                    pixels outside the image do not)
//   5  growth        M_0 = seed;  M_{i+1}(p) = M_i(p) || (eligible(p) && some 4-neighbour q inside the image has M_i(q)
//                    && fabsf(depth(p) - depth(q)) <= grow_depth); exactly `grow` steps; the mask is M_grow, 0 / 1
//
// The class pass (gs_picp_outlier_classes_batch_f32; 8 sequences per launch, any B in groups) is three launches and, in
// front of a call's first use of the counters, one that clears them: the residual pass of gs_picp_scale.hip (keys, first
// digit), one block per sequence that selects the median (ps_select_median, shared) and forms both thresholds, and one
// thread per pixel that associates again and writes the class byte.  Nothing is read back, the map count is read on the
// device, a stale index entry is rejected as ever; no float atomics.
// The region pass (gs_region_mask_u8; one launch for all images) works on 32 x 32 tiles with a halo of grow + 1 pixels
// in LDS: a pixel's result depends only on the seeds within Manhattan distance grow, a seed on the 3 x 3 around it.  The
// support count and all grow steps run inside the block, on ping-pong byte images with a barrier per step: M_i is right
// within grow - i pixels of the tile, so M_grow is right on the tile, without any communication between blocks.  Integer
// outputs, bitwise reproducible.
#include "gs_picp_scale_dev.h"

constexpr int GS_OUT_STRONG = 1, GS_OUT_ELIGIBLE = 2;

// ------------------------------------------------------------------ the class pass
struct PoSeq {
  PiInputs in;
  const float* T;       // the pose the classes are taken at
  float* th_dev;        // (2) hi_t, lo_t: written by the threshold kernel, read by the class kernel
  float* th_out;        // the caller's copy (2), or NULL
  uint8_t* classes;     // (H, W)
};
struct PoBatch {
  PoSeq s[GS_MAX_BATCH];
  PiGeom g;
};
struct PoRule {
  float c_hi, c_lo, floor;
};

// one threshold of the rule from the median's key: +0.0 without a used pixel
GS_DEV float po_threshold(const uint32_t n, const uint32_t med, const float c, const float floor) {
  if (n == 0u) return 0.0f;
  const float t = c * __uint_as_float(med);
  return t > floor ? t : floor;
}

// one block per sequence: the median of the key table the residual pass left, then both thresholds
__global__ void __launch_bounds__(GS_PS_THREADS) gs_picp_outlier_thresholds_kernel(const PiScaleBatch sb, const PoBatch ob,
                                                                                   const PoRule rule) {
  const PoSeq& q = ob.s[blockIdx.x];
  uint32_t n;
  const uint32_t med = ps_select_median(sb.s[blockIdx.x].r[PS_GEO], sb.g.nslots, n);
  if (threadIdx.x == 0) {
    const float hi_t = po_threshold(n, med, rule.c_hi, rule.floor), lo_t = po_threshold(n, med, rule.c_lo, rule.floor);
    q.th_dev[0] = hi_t;
    q.th_dev[1] = lo_t;
    if (q.th_out) {
      q.th_out[0] = hi_t;
      q.th_out[1] = lo_t;
    }
  }
}

// one thread per pixel (256 per block = one chunk of the stride-1 lattice, batched like the linearise kernel)
template <bool WEIGHTED>
GS_DEV void po_classes(const PoBatch& ob) {
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  const PoSeq& q = ob.s[blockIdx.x % ob.g.B];
  const PiSlot t = pi_prologue(q.in, ob.g, q.T, cam, Ts);
  const int64_t n_map = gs_count(q.in.n);
  if (!t.in_lattice) return;
  const float hi_t = q.th_dev[0], lo_t = q.th_dev[1];
  int64_t row;
  float s[3], wp;
  float4 d, m;
  const int code = pi_associate<WEIGHTED>(Ts, cam, q.in, ob.g, n_map, t.p, row, s, d, m, wp);
  bool strong = code == 4 || code == 5, eligible = strong;
  if (code == 0) {
    float a[6], b;
    gn_row_pn(s[0], s[1], s[2], d, m, a, b);
    const float r = fabsf(b);
    strong = r > hi_t && hi_t > 0.0f;
    eligible = strong || (r > lo_t && lo_t > 0.0f);
  }
  q.classes[t.k] = (uint8_t)((strong ? GS_OUT_STRONG : 0) | (eligible ? GS_OUT_ELIGIBLE : 0));
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_outlier_classes_kernel(const PoBatch ob) { po_classes<false>(ob); }
__global__ void __launch_bounds__(GS_PI_CHUNK) gs_weighted_picp_outlier_classes_kernel(const PoBatch ob) {
  po_classes<true>(ob);
}

extern "C" int64_t gs_picp_outlier_classes_scratch_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  // keys (H W) | the first digit's counters (2048) | the two thresholds
  return (int64_t)picp_scaled_bytes(0, (int64_t)H * W);
}

extern "C" int gs_picp_outlier_classes_batch_f32(const gs_picp_seq* seqs_host, const float* const* weights_host,
                                                 uint8_t* const* classes_host, float* const* thresholds_host, int B, int H,
                                                 int W, float dist_th, float dot_th, float hi, float lo, float floor,
                                                 void* stream) {
  const char* who = __func__;
  PICP_REQUIRE(who, seqs_host && classes_host && B > 0 && H > 0 && W > 0, "bad arguments");
  PICP_REQUIRE(who, (int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  PICP_REQUIRE(who, !(dist_th != dist_th) && !(dot_th != dot_th), "a threshold is NaN");
  PICP_REQUIRE(who, lo > 0.0f && lo < __builtin_inff(), "lo must be finite and positive");
  PICP_REQUIRE(who, hi >= lo && hi < __builtin_inff(), "hi must be finite and at least lo");
  PICP_REQUIRE(who, floor >= 0.0f && floor < __builtin_inff(), "floor must be finite and not negative");
  for (int b = 0; b < B; ++b) {
    PICP_CHECK_SEQ(who, seqs_host[b]);
    PICP_REQUIRE(who, classes_host[b], "NULL pointer (classes)");
    PICP_REQUIRE(who, ((uintptr_t)seqs_host[b].scratch & 15) == 0, "scratch must be 16-byte aligned");
  }
  hipStream_t st = gs_stream(stream);
  const bool weighted = weights_host != nullptr;
  const PiScale sc = picp_scale_geo(1.0f, 0.0f, nullptr, nullptr);   // (which residual: the constants are the rule's)
  const PoRule rule{picp_scale_c(hi), picp_scale_c(lo), floor};
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    PiScaleBatch sb;
    PoBatch ob;
    picp_fill(ob.g, nb, H, W, 1, dist_th, dot_th, 1.0f);
    sb.g = ob.g;
    for (int b = 0; b < nb; ++b) {
      const gs_picp_seq& u = seqs_host[c0 + b];
      PoSeq& q = ob.s[b];
      picp_fill_inputs(q.in, u);
      if (weighted) q.in.weight = weights_host[c0 + b];
      q.T = u.init_pose16;
      q.classes = classes_host[c0 + b];
      q.th_out = thresholds_host ? thresholds_host[c0 + b] : nullptr;
      char* p = static_cast<char*>(u.scratch);
      PiScaleSeq& z = sb.s[b];
      z.in = q.in;
      z.T_in = q.T;
      z.color = nullptr;
      z.model = nullptr;
      z.r[PS_GEO].keys = reinterpret_cast<uint32_t*>(p);
      z.r[PS_GEO].hist = reinterpret_cast<uint32_t*>(p + picp_keys_bytes(ob.g.nslots));
      z.r[PS_GEO].delta_dev = nullptr;
      z.r[PS_GEO].delta_out = nullptr;
      z.r[PS_COLOR] = PiScaleRes{nullptr, nullptr, nullptr, nullptr};
      q.th_dev = reinterpret_cast<float*>(p + picp_keys_bytes(ob.g.nslots) + picp_hist_bytes());
    }
    picp_scale_keys_launch(sb, picp_scale_pick(sc), true, weighted, st);
    hipLaunchKernelGGL(gs_picp_outlier_thresholds_kernel, dim3((unsigned)nb), dim3(GS_PS_THREADS), 0, st, sb, ob, rule);
    const dim3 chunks((unsigned)nb * (unsigned)ob.g.nchunks);   // < 8 * 2^23
    if (weighted)
      hipLaunchKernelGGL(gs_weighted_picp_outlier_classes_kernel, chunks, dim3(GS_PI_CHUNK), 0, st, ob);
    else
      hipLaunchKernelGGL(gs_picp_outlier_classes_kernel, chunks, dim3(GS_PI_CHUNK), 0, st, ob);
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}

// ------------------------------------------------------------------ the region pass
constexpr int GS_RM_TILE = 32;                                      // output pixels per side of a block's tile
constexpr int GS_RM_MAX_GROW = 16;
constexpr int GS_RM_SIDE = GS_RM_TILE + 2 * (GS_RM_MAX_GROW + 1);   // the widest region: 66
constexpr int GS_RM_CELLS = GS_RM_SIDE * GS_RM_SIDE;                // 4 356 cells: 17 KB of depth, 3 x 4.3 KB of bytes
constexpr int GS_RM_THREADS = 256;
constexpr int GS_RM_MAX_IMAGES = 65535;                             // images per launch (gridDim.y)

// Block (x, y): tile x of image y.  The region is the tile with a halo of grow + 1 cells, side = 32 + 2 (grow + 1); cells
// outside the image have class 0 and are never set.  The outermost ring only lends its classes to the seeds of the ring
// inside it and stays 0 in both mask images.
__global__ void __launch_bounds__(GS_RM_THREADS) gs_region_mask_kernel(const uint8_t* __restrict__ classes,
                                                                       const float* __restrict__ depth,
                                                                       uint8_t* __restrict__ mask, const int H, const int W,
                                                                       const int tiles_x, const int min_support,
                                                                       const int grow, const float grow_depth) {
  __shared__ float dep[GS_RM_CELLS];
  __shared__ uint8_t cls[GS_RM_CELLS];
  __shared__ uint8_t buf[2][GS_RM_CELLS];
  const int tid = threadIdx.x;
  const int halo = grow + 1, side = GS_RM_TILE + 2 * halo, cells = side * side;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int y0 = ty * GS_RM_TILE - halo, x0 = tx * GS_RM_TILE - halo;
  const int64_t image = (int64_t)blockIdx.y * H * W;
  for (int c = tid; c < cells; c += GS_RM_THREADS) {
    const int ry = c / side, rx = c - ry * side;
    const int y = y0 + ry, x = x0 + rx;
    const bool inside = y >= 0 && y < H && x >= 0 && x < W;
    const int64_t p = image + (int64_t)y * W + x;
    cls[c] = inside ? classes[p] : (uint8_t)0;
    dep[c] = inside && grow > 0 ? depth[p] : 0.0f;
    buf[0][c] = 0;
    buf[1][c] = 0;
  }
  __syncthreads();
  // the seeds, for every cell but the outermost ring
  for (int c = tid; c < cells; c += GS_RM_THREADS) {
    const int ry = c / side, rx = c - ry * side;
    if (ry < 1 || ry >= side - 1 || rx < 1 || rx >= side - 1 || !(cls[c] & GS_OUT_STRONG)) continue;
    int n = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) n += cls[c + dy * side + dx] & GS_OUT_STRONG;
    if (n >= min_support) buf[0][c] = 1;
  }
  __syncthreads();
  int cur = 0;
  for (int step = 0; step < grow; ++step) {
    const uint8_t* M = buf[cur];
    uint8_t* Mn = buf[cur ^ 1];
    for (int c = tid; c < cells; c += GS_RM_THREADS) {
      const int ry = c / side, rx = c - ry * side;
      if (ry < 1 || ry >= side - 1 || rx < 1 || rx >= side - 1) continue;
      uint8_t v = M[c];
      if (!v && (cls[c] & GS_OUT_ELIGIBLE)) {
        const float z = dep[c];
        // (a neighbour outside the image is never set)
        if ((M[c - side] && fabsf(z - dep[c - side]) <= grow_depth) || (M[c + side] && fabsf(z - dep[c + side]) <= grow_depth) ||
            (M[c - 1] && fabsf(z - dep[c - 1]) <= grow_depth) || (M[c + 1] && fabsf(z - dep[c + 1]) <= grow_depth))
          v = 1;
      }
      Mn[c] = v;
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int i = tid; i < GS_RM_TILE * GS_RM_TILE; i += GS_RM_THREADS) {
    const int ly = i / GS_RM_TILE, lx = i - ly * GS_RM_TILE;
    const int y = ty * GS_RM_TILE + ly, x = tx * GS_RM_TILE + lx;
    if (y < H && x < W) mask[image + (int64_t)y * W + x] = buf[cur][(ly + halo) * side + lx + halo];
  }
}

extern "C" int gs_region_mask_u8(const uint8_t* classes, const float* depth, uint8_t* mask, int64_t B, int H, int W,
                                 int min_support, int grow, float grow_depth, void* stream) {
  GS_REQUIRE(classes && depth && mask, "NULL pointer");
  GS_REQUIRE(B > 0 && H > 0 && W > 0, "bad arguments");
  GS_REQUIRE((int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  GS_REQUIRE(min_support >= 1 && min_support <= 9, "min_support must be within 1 .. 9");
  GS_REQUIRE(grow >= 0 && grow <= GS_RM_MAX_GROW, "grow must be within 0 .. 16");
  GS_REQUIRE(grow_depth >= 0.0f && grow_depth < __builtin_inff(), "grow_depth must be finite and not negative");
  hipStream_t st = gs_stream(stream);
  const int tiles_x = (int)gs_ceil_div(W, GS_RM_TILE), tiles_y = (int)gs_ceil_div(H, GS_RM_TILE);   // < 2^21 tiles
  const int64_t HW = (int64_t)H * W;
  for (int64_t b0 = 0; b0 < B; b0 += GS_RM_MAX_IMAGES) {
    const int64_t nb = B - b0 < GS_RM_MAX_IMAGES ? B - b0 : GS_RM_MAX_IMAGES;
    hipLaunchKernelGGL(gs_region_mask_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)nb), dim3(GS_RM_THREADS), 0,
                       st, classes + b0 * HW, depth + b0 * HW, mask + b0 * HW, H, W, tiles_x, min_support, grow,
                       grow_depth);
  }
  GS_LAUNCH_CHECK();
  return GS_OK;
}
