// gs_picp_color.hip — the projective ICP (gs_picp.hip) with a photometric term (Steinbruecker / Kerl; the hybrid odometry
// of Kintinuous, ElasticFusion and Open3D): a slot of the live frame's lattice contributes its point-to-plane row and, where
// the model view has an intensity gradient, a colour row against the rendered colour of the map.  The association, the
// reject codes, the reduction order, the solve and the update are those of gs_picp.hip: gs_picp_dev.h holds ONE
// definition of each -- the block prologue (pi_prologue), pi_associate, the chunk reduction (pi_chunk_reduce, PI_PAIRS),
// the finish body (pi_finish with pi_column_sums) and the host drivers (picp_solve, picp_rows), which this file
// instantiates with its traits (PiJoint).  What this file adds is
//
//   model intensity  one thread per pixel of the model view (a 32 x 8 tile with a one-pixel halo in LDS), batched over B:
//                    (I, gx, gy, ok) of the rendered colour, once per localisation
//   linearise        gs_picp_linearize_kernel's slot, plus the colour row: one 16-byte gather of the model pixel and the
//                    three colour loads of the live pixel
//   finish           pi_finish<true>: the plain finish, which also adds up the colour-row counts
//
// Two launches per iteration for up to 8 sequences, nothing read back, the map count read on the device.
//
// Arithmetic (-ffp-contract=off; float32, one rounding per operation, NO FMA anywhere in what this file adds: every product
// and sum below is plain, every division the correctly rounded float32 '/'; tests/picp_color_ref.py restates it).
// luma(R, G, B) = (0.299f * R + 0.587f * G) + 0.114f * B.
// Model intensity at pixel (h, w), I = luma(color[h, w]):
//   ok = 1.0f iff 0 < h < H - 1, 0 < w < W - 1 and index >= 0 at (h, w), (h, w - 1), (h, w + 1), (h - 1, w), (h + 1, w)
//   gx = 0.5f * (I[h, w + 1] - I[h, w - 1]),  gy = 0.5f * (I[h + 1, w] - I[h - 1, w])   when ok, else gx = gy = +0.0f
//   out[h, w] = (I, gx, gy, ok): I is the luma of whatever the render left at the pixel (0 in a hole); a hole of the view
//   never leaks a gradient.
// Colour row of a slot with code 0 (s, d, m of pi_associate), (q, h2, w2) = gs_project_point_hw_q(cam, s):
//   (u, v) = the projector's continuous pixel: r_j = ((K[j,0] q0 + K[j,1] q1) + K[j,2] q2) + K[j,3] * 1, z = r_2 (1 if 0),
//            u = r_0 / z, v = r_1 / z               (the operations of gs_project_point_hw_q, restated by pic_project_uv)
//   (I, gx, gy, ok) = model[h2, w2]; the slot has a colour row iff ok == 1.0f
//   Il = luma(color[pixel of the slot])
//   r  = Il - ((I + gx * (u - (float)w2)) + gy * (v - (float)h2))
//   ax = gx * K[0,0], ay = gy * K[1,1]
//   Jq = (ax / q2, ay / q2, (-(ax * q0 + ay * q1)) / (q2 * q2))
//   Js_j = (R_m[j,0] Jq0 + R_m[j,1] Jq1) + R_m[j,2] Jq2                    (gs_dot3_plain, R_m = the model pose's rotation)
//   c  = s x Js with the operations of gn_row_pn: (Js2 s1 - Js1 s2, Js0 s2 - Js2 s0, Js1 s0 - Js0 s1)
//   a_c = (w Js0, w Js1, w Js2, w c0, w c1, w c2),  b_c = w r,  w = color_weight (metres per intensity unit)
// A slot without a colour row has a_c = b_c = +0.0f.
// The 28 terms of a slot are (double)x_g (double)y_g + (double)x_c (double)y_c: two exact products of float32 factors,
// their sum rounded once; a rejected slot contributes +0.0.  The reduction, the solve, the update and the "no geometric
// inlier keeps the pose bits" rule are gs_picp.hip's; the colour rows are counted alongside as an integer.
// The robust entries (gs_projective_icp_color_robust_batch_f32 / _rows_f32) launch the ROBUST instance of the joint body:
// w as in gs_picp.hip for b, wc = |r| > cdelta ? cdelta / |r| : 1 for the colour residual r BEFORE the weight w is applied
// (a threshold of 0: that weight is 1), terms (double)w * (x_g y_g) + (double)wc * (x_c y_c), each product exact and
// rounded once by its weight.  With both thresholds 0 they launch the plain kernel.
// The colour row itself (pic_color_row) lives in gs_picp_color_dev.h: the residual pass of the median rule
// (gs_picp_scale.hip) forms r with it too.  The joint scaled entries (gs_projective_icp_color_joint_scaled_*) estimate
// cdelta per sequence and iteration from the lower median of |r| over the slots with a colour row; the ROBUST instance
// then reads it from the sequence's device float (PicSeq::cdelta_dev) instead of the launch's constant.
#include "gs_picp_color_dev.h"

struct PicSeq {
  PiSeq g;
  const float* color;       // live frame (H, W, 3)
  const float4* model;      // model intensity (H, W)
  const float* cdelta_dev;  // the sequence's colour Huber threshold of this iteration (gs_picp_scale.hip), or NULL:
                            // PiRobust::cdelta
  int32_t* ccounts;         // (nchunks) colour rows per chunk
  int32_t* cflag_out;       // table-level outputs, any may be NULL: (nslots)
  float* ac_out;            // (nslots, 6)
  float* bc_out;            // (nslots)
  int64_t* ccount_out;      // finish: (1), or NULL
};
struct PicBatch {
  PicSeq s[GS_MAX_BATCH];
  PiGeom g;
  float weight;
};

// ------------------------------------------------------------------ model intensity
constexpr int PIC_TX = 32, PIC_TY = 8;   // 256 threads: a row of the tile is 32 pixels = 384 contiguous bytes of colour

__global__ void __launch_bounds__(PIC_TX * PIC_TY) gs_picp_color_intensity_kernel(const float* __restrict__ color,
                                                                                  const int64_t* __restrict__ index,
                                                                                  float4* __restrict__ out, const int H,
                                                                                  const int W) {
  __shared__ float lum[PIC_TY + 2][PIC_TX + 2];
  __shared__ uint8_t hit[PIC_TY + 2][PIC_TX + 2];
  const int64_t img = (int64_t)blockIdx.z * H * W;
  const int w0 = blockIdx.x * PIC_TX - 1, h0 = blockIdx.y * PIC_TY - 1;
  for (int e = threadIdx.x; e < (PIC_TY + 2) * (PIC_TX + 2); e += PIC_TX * PIC_TY) {
    const int ly = e / (PIC_TX + 2), lx = e - ly * (PIC_TX + 2);
    const int h = h0 + ly, w = w0 + lx;
    float I = 0.0f;
    uint8_t ok = 0;
    if (h >= 0 && h < H && w >= 0 && w < W) {
      const int64_t p = img + (int64_t)h * W + w;
      I = pic_luma(color[3 * p], color[3 * p + 1], color[3 * p + 2]);
      ok = index[p] >= 0;
    }
    lum[ly][lx] = I;
    hit[ly][lx] = ok;
  }
  __syncthreads();
  const int lx = threadIdx.x % PIC_TX + 1, ly = threadIdx.x / PIC_TX + 1;
  const int h = h0 + ly, w = w0 + lx;
  if (h >= H || w >= W) return;
  // (a neighbour outside the image has hit = 0)
  const bool ok = hit[ly][lx] && hit[ly][lx - 1] && hit[ly][lx + 1] && hit[ly - 1][lx] && hit[ly + 1][lx];
  float gx = 0.0f, gy = 0.0f;
  if (ok) {
    gx = 0.5f * (lum[ly][lx + 1] - lum[ly][lx - 1]);
    gy = 0.5f * (lum[ly + 1][lx] - lum[ly - 1][lx]);
  }
  out[img + (int64_t)h * W + w] = make_float4(lum[ly][lx], gx, gy, ok ? 1.0f : 0.0f);
}

extern "C" int gs_model_intensity_f32(const float* color, const int64_t* index, int B, int H, int W, float* out,
                                      void* stream) {
  GS_REQUIRE(color && index && out, "NULL pointer");
  GS_REQUIRE(B > 0 && H > 0 && W > 0, "bad sizes");
  GS_REQUIRE((int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  GS_REQUIRE(((uintptr_t)out & 15) == 0, "out must be 16-byte aligned");
  GS_REQUIRE(out != color, "out must not be an input");
  hipStream_t st = gs_stream(stream);
  const dim3 tiles((unsigned)gs_ceil_div(W, PIC_TX), (unsigned)gs_ceil_div(H, PIC_TY), 1);
  GS_REQUIRE(tiles.y <= 65535u, "image too tall");
  for (int b0 = 0; b0 < B; b0 += 65535) {   // (the z extent of a grid)
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    const int64_t off = (int64_t)b0 * H * W;
    hipLaunchKernelGGL(gs_picp_color_intensity_kernel, dim3(tiles.x, tiles.y, (unsigned)nb), dim3(PIC_TX * PIC_TY), 0, st,
                       color + 3 * off, index + off, reinterpret_cast<float4*>(out) + off, H, W);
  }
  GS_LAUNCH_CHECK();
  return GS_OK;
}

// ------------------------------------------------------------------ the joint linearisation
// The joint linearise kernel's body: prologue, association, the rows z = (a0 .. a5, b) and zc = (ac0 .. ac5, bc), the
// table outputs, the chunk reduction.  ROBUST: the geometric product of every term carries the Huber weight w of the
// slot's residual b, the colour product the weight wc of its colour residual r (pi_huber_weight, gs_picp_dev.h).
// WEIGHTED (with ROBUST; the weighted entries, see gs_picp.hip): both weights carry the slot's pixel weight, wp * w and
// wp * wc, one float32 product each; a masked slot has code 6 and no colour row.
template <bool ROBUST, bool WEIGHTED = false>
GS_DEV void pic_linearize(const PicBatch& pb, const PiRobust& rb) {
  static_assert(ROBUST || !WEIGHTED, "the weighted instance carries its weight through the robust terms");
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  __shared__ int cnt[GS_PI_CHUNK / GS_WAVE], ccnt[GS_PI_CHUNK / GS_WAVE];
  const PicSeq& qc = pb.s[blockIdx.x % pb.g.B];
  const PiSeq& q = qc.g;
  const PiSlot t = pi_prologue(q.in, pb.g, q.T_in, cam, Ts);
  const int64_t n_map = gs_count(q.in.n);
  int code = 1;
  bool colored = false;
  int64_t row = -1;
  float z[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, zc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float w = 1.0f, wc = 1.0f;
  const float delta = ROBUST ? pi_huber_delta(q.delta_dev, rb) : 0.0f;
  const float cdelta = ROBUST ? (qc.cdelta_dev ? *qc.cdelta_dev : rb.cdelta) : 0.0f;
  if (t.in_lattice) {
    float s[3];
    float4 d, m;
    float wp;
    code = pi_associate<WEIGHTED>(Ts, cam, q.in, pb.g, n_map, t.p, row, s, d, m, wp);
    if (code == 0) {
      gn_row_pn(s[0], s[1], s[2], d, m, z, z[6]);
      if (ROBUST) w = pi_huber_weight(pi_huber_clipped(z[6], delta), z[6], delta);
      if (WEIGHTED) w = wp * w;
      float r = 0.0f;
      colored = pic_color_row(cam, pb.g, qc.color, qc.model, t.p, s, pb.weight, zc, r);
      if (ROBUST && colored) wc = pi_huber_weight(pi_huber_clipped(r, cdelta), r, cdelta);
      if (WEIGHTED && colored) wc = wp * wc;
    }
    pi_table_out(q, t.k, code, row, z);
    if (qc.cflag_out) qc.cflag_out[t.k] = colored ? 1 : 0;
    if (qc.ac_out) {
#pragma unroll
      for (int c = 0; c < 6; ++c) qc.ac_out[6 * (int64_t)t.k + c] = zc[c];
    }
    if (qc.bc_out) qc.bc_out[t.k] = zc[6];
    if (ROBUST) {
      if (rb.weight_out) rb.weight_out[t.k] = code == 0 ? w : 0.0f;
      if (rb.cweight_out) rb.cweight_out[t.k] = colored ? wc : 0.0f;
    }
  }
  const bool used = code == 0;   // (z, zc are zero otherwise: every term below is then +0.0)
  const unsigned long long mask = __ballot(used);
  const unsigned long long cmask = __ballot(colored);
  if (t.lane == 0) {
    cnt[t.wave] = __popcll(mask);
    ccnt[t.wave] = __popcll(cmask);
  }
  // (a colour row needs a used slot: a wave without a used slot adds up +0.0 only)
  double* partial_row = q.partials + (int64_t)t.chunk * LIN_NV;
  if constexpr (ROBUST)
    pi_chunk_reduce<LIN_NV>(
        [&](const int i) {
          const int x = PI_PAIRS.x[i], y = PI_PAIRS.y[i];
          return pi_term(w, z[x], z[y]) + pi_term(wc, zc[x], zc[y]);
        },
        mask != 0ull, partial_row);
  else
    pi_chunk_reduce<LIN_NV>(
        [&](const int i) {
          const int x = PI_PAIRS.x[i], y = PI_PAIRS.y[i];
          return (double)z[x] * (double)z[y] + (double)zc[x] * (double)zc[y];
        },
        mask != 0ull, partial_row);
  if (threadIdx.x == GS_WAVE) q.counts[t.chunk] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
  if (threadIdx.x == GS_WAVE + 1) qc.ccounts[t.chunk] = (ccnt[0] + ccnt[1]) + (ccnt[2] + ccnt[3]);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_color_linearize_kernel(const PicBatch pb) {
  pic_linearize<false>(pb, PiRobust{0.0f, 0.0f, nullptr, nullptr});
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_robust_picp_color_linearize_kernel(const PicBatch pb, const PiRobust rb) {
  pic_linearize<true>(pb, rb);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_weighted_picp_color_linearize_kernel(const PicBatch pb,
                                                                                       const PiRobust rb) {
  pic_linearize<true, true>(pb, rb);
}

__global__ void __launch_bounds__(GS_PI_FIN) gs_picp_color_finish_kernel(const PicBatch pb) {
  const PicSeq& qc = pb.s[blockIdx.x];
  pi_finish<true>(qc.g, pb.g.nchunks, pb.g.damp, qc.ccounts, qc.ccount_out);
}

// ------------------------------------------------------------------ entry points
// scratch of a sequence: the plain solve's (partials, counts), then the colour-row counts
extern "C" int64_t gs_projective_icp_color_scratch_bytes(int H, int W, int stride) {
  if (H <= 0 || W <= 0 || stride <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  const int64_t nchunks = gs_ceil_div(picp_slots(H, W, stride), GS_PI_CHUNK);
  return (int64_t)(picp_partials_bytes(nchunks) + 2 * picp_counts_bytes(nchunks));
}

extern "C" int64_t gs_projective_icp_color_scaled_scratch_bytes(int H, int W, int stride) {
  const int64_t base = gs_projective_icp_color_scratch_bytes(H, W, stride);
  return base > 0 ? (int64_t)picp_scaled_bytes((size_t)base, picp_slots(H, W, stride)) : 0;
}

// the traits of the colour solve for the drivers of gs_picp_dev.h
struct PiJoint {
  using Seq = gs_picp_color_seq;
  using Batch = PicBatch;
  static constexpr int TRACE = GS_PIC_TRACE;
  static constexpr auto linearize = gs_picp_color_linearize_kernel;
  static constexpr auto robust_linearize = gs_robust_picp_color_linearize_kernel;
  static constexpr auto weighted_linearize = gs_weighted_picp_color_linearize_kernel;
  static constexpr auto finish = gs_picp_color_finish_kernel;
  static const gs_picp_seq& base(const Seq& u) { return u.base; }
  static PiSeq& seq(Batch& pb, int b) { return pb.s[b].g; }
  static int check(const char* who, const Seq& u) {
    PICP_CHECK_SEQ(who, u.base);
    PICP_REQUIRE(who, u.color && u.model_intensity, "NULL pointer (color / model_intensity)");
    PICP_REQUIRE(who, ((uintptr_t)u.model_intensity & 15) == 0, "model_intensity must be 16-byte aligned");
    return GS_OK;
  }
  static void fill(Batch& pb, int b, const Seq& u, float color_weight) {
    PicSeq& s = pb.s[b];
    const int nchunks = pb.g.nchunks;
    pb.weight = color_weight;
    picp_fill_seq(s.g, u.base, nchunks);
    s.color = u.color;
    s.model = reinterpret_cast<const float4*>(u.model_intensity);
    s.cdelta_dev = nullptr;
    s.ccounts = reinterpret_cast<int32_t*>(static_cast<char*>(u.base.scratch) + picp_partials_bytes(nchunks) +
                                           picp_counts_bytes(nchunks));
    s.cflag_out = nullptr; s.ac_out = nullptr; s.bc_out = nullptr; s.ccount_out = nullptr;
  }
  static size_t scratch_bytes(int64_t nchunks) { return picp_partials_bytes(nchunks) + 2 * picp_counts_bytes(nchunks); }
  static void color_outputs(Batch& pb, const PiRowsOut& o) {
    PicSeq& s = pb.s[0];
    s.ac_out = o.ac6; s.bc_out = o.bc; s.cflag_out = o.colored; s.ccount_out = o.color_count;
  }
  // the colour side of the median rule: the residual pass reads the sequence's colour inputs, and with a colour
  // threshold asked for the sequence reads it from the rule's device float
  static void color_scale(Batch& pb, int b, PiScaleSeq& z, bool col) {
    PicSeq& s = pb.s[b];
    z.color = s.color;
    z.model = s.model;
    if (col) s.cdelta_dev = z.r[PS_COLOR].delta_dev;
  }
};

extern "C" int gs_projective_icp_color_batch_f32(const gs_picp_color_seq* seqs_host, int B, int H, int W,
                                                 const gs_picp_params* params_host, float color_weight, void* stream) {
  return picp_solve<PiJoint>(__func__, seqs_host, nullptr, B, H, W, params_host, color_weight, 0.0f, 0.0f, nullptr, stream);
}

extern "C" int gs_projective_icp_color_robust_batch_f32(const gs_picp_color_seq* seqs_host, int B, int H, int W,
                                                        const gs_picp_params* params_host, float color_weight,
                                                        float huber_delta, float color_huber_delta, void* stream) {
  return picp_solve<PiJoint>(__func__, seqs_host, nullptr, B, H, W, params_host, color_weight, huber_delta,
                             color_huber_delta, nullptr, stream);
}

// the joint solve with the geometric threshold from the median of |b| (gs_picp_scale.hip); the colour threshold stays
// the caller's constant
extern "C" int gs_projective_icp_color_scaled_batch_f32(const gs_picp_color_seq* seqs_host, float* const* deltas_host,
                                                        int B, int H, int W, const gs_picp_params* params_host,
                                                        float color_weight, float huber_k, float huber_floor,
                                                        float color_huber_delta, void* stream) {
  PICP_CHECK_SCALE(__func__, huber_k, huber_floor);
  const PiScale sc = picp_scale_geo(huber_k, huber_floor, deltas_host, nullptr);
  return picp_solve<PiJoint>(__func__, seqs_host, nullptr, B, H, W, params_host, color_weight, 0.0f, color_huber_delta,
                             &sc, stream);
}

// The joint solve with either threshold, or both, from its residuals' median (gs_picp_scale.hip): huber_k > 0: the
// geometric one from |b| over the used slots, huber_floor its floor; color_huber_k > 0: the colour one from |r| (the
// colour residual before color_weight is applied) over the slots with a colour row, color_huber_floor its floor.  A
// constant of 0 leaves that threshold the constant its floor names (0: off).  The same two extra launches per iteration
// whichever are asked for.  The scratch is gs_projective_icp_color_joint_scaled_scratch_bytes.
static int pic_check_joint_scale(const char* who, float huber_k, float huber_floor, float color_huber_k,
                                 float color_huber_floor) {
  PICP_REQUIRE(who, huber_k >= 0.0f && huber_k < __builtin_inff(), "huber_k must be finite and not negative");
  PICP_REQUIRE(who, huber_floor >= 0.0f && huber_floor < __builtin_inff(), "huber_floor must be finite and not negative");
  PICP_REQUIRE(who, color_huber_k >= 0.0f && color_huber_k < __builtin_inff(),
               "color_huber_k must be finite and not negative");
  PICP_REQUIRE(who, color_huber_floor >= 0.0f && color_huber_floor < __builtin_inff(),
               "color_huber_floor must be finite and not negative");
  return GS_OK;
}

extern "C" int64_t gs_projective_icp_color_joint_scaled_scratch_bytes(int H, int W, int stride) {
  const int64_t base = gs_projective_icp_color_scratch_bytes(H, W, stride);
  return base > 0 ? (int64_t)picp_joint_scaled_bytes((size_t)base, picp_slots(H, W, stride)) : 0;
}

extern "C" int gs_projective_icp_color_joint_scaled_batch_f32(const gs_picp_color_seq* seqs_host,
                                                              float* const* deltas_host, float* const* cdeltas_host,
                                                              int B, int H, int W, const gs_picp_params* params_host,
                                                              float color_weight, float huber_k, float huber_floor,
                                                              float color_huber_k, float color_huber_floor,
                                                              void* stream) {
  if (const int err = pic_check_joint_scale(__func__, huber_k, huber_floor, color_huber_k, color_huber_floor)) return err;
  const PiScale sc = picp_scale_joint(huber_k, huber_floor, color_huber_k, color_huber_floor, deltas_host, cdeltas_host,
                                      nullptr, nullptr);
  return picp_solve<PiJoint>(__func__, seqs_host, nullptr, B, H, W, params_host, color_weight, huber_floor,
                             color_huber_floor, sc.on[PS_GEO] || sc.on[PS_COLOR] ? &sc : nullptr, stream);
}

extern "C" int gs_projective_icp_color_rows_f32(const gs_picp_color_seq* seq_host, int H, int W, int stride,
                                                float dist_th, float dot_th, float color_weight, int32_t* code,
                                                int64_t* row, float* a6, float* b, float* ac6, float* bc,
                                                int32_t* colored, double* sums28, int64_t* count, int64_t* color_count,
                                                void* stream) {
  return picp_rows<PiJoint>(__func__, seq_host, H, W, stride, dist_th, dot_th, color_weight,
                            PiRobust{0.0f, 0.0f, nullptr, nullptr},
                            PiRowsOut{code, row, a6, b, ac6, bc, colored, sums28, count, color_count}, nullptr, stream);
}

extern "C" int gs_projective_icp_color_robust_rows_f32(const gs_picp_color_seq* seq_host, int H, int W, int stride,
                                                       float dist_th, float dot_th, float color_weight,
                                                       float huber_delta, float color_huber_delta, int32_t* code,
                                                       int64_t* row, float* a6, float* b, float* ac6, float* bc,
                                                       int32_t* colored, float* weight, float* color_weight_out,
                                                       double* sums28, int64_t* count, int64_t* color_count,
                                                       void* stream) {
  return picp_rows<PiJoint>(__func__, seq_host, H, W, stride, dist_th, dot_th, color_weight,
                            PiRobust{huber_delta, color_huber_delta, weight, color_weight_out},
                            PiRowsOut{code, row, a6, b, ac6, bc, colored, sums28, count, color_count}, nullptr, stream);
}

// one joint linearisation with the thresholds derived at init_pose16 as in gs_projective_icp_color_joint_scaled_batch_f32;
// delta_out / cdelta_out (one float each, may be NULL): the thresholds the weights were taken with
extern "C" int gs_projective_icp_color_joint_scaled_rows_f32(const gs_picp_color_seq* seq_host, int H, int W, int stride,
                                                             float dist_th, float dot_th, float color_weight,
                                                             float huber_k, float huber_floor, float color_huber_k,
                                                             float color_huber_floor, int32_t* code, int64_t* row,
                                                             float* a6, float* b, float* ac6, float* bc,
                                                             int32_t* colored, float* weight, float* color_weight_out,
                                                             double* sums28, int64_t* count, int64_t* color_count,
                                                             float* delta_out, float* cdelta_out, void* stream) {
  if (const int err = pic_check_joint_scale(__func__, huber_k, huber_floor, color_huber_k, color_huber_floor)) return err;
  const PiScale sc = picp_scale_joint(huber_k, huber_floor, color_huber_k, color_huber_floor, nullptr, nullptr, delta_out,
                                      cdelta_out);
  return picp_rows<PiJoint>(__func__, seq_host, H, W, stride, dist_th, dot_th, color_weight,
                            PiRobust{huber_floor, color_huber_floor, weight, color_weight_out},
                            PiRowsOut{code, row, a6, b, ac6, bc, colored, sums28, count, color_count},
                            sc.on[PS_GEO] || sc.on[PS_COLOR] ? &sc : nullptr, stream);
}

// The weighted joint entries (pixel weights: the rule is in gs_picp.hip's header): thresholds as in the joint scaled
// entries with huber_delta / color_huber_delta for the floors -- a constant of 0 leaves that threshold the constant its
// floor names --, the scratch gs_projective_icp_color_joint_scaled_scratch_bytes when a rule is on, else the colour one.
static int pic_check_weighted(const char* who, float huber_delta, float huber_k, float color_huber_delta,
                              float color_huber_k) {
  PICP_CHECK_DELTA(who, huber_delta, "huber_delta");
  PICP_CHECK_DELTA(who, color_huber_delta, "color_huber_delta");
  PICP_REQUIRE(who, huber_k >= 0.0f && huber_k < __builtin_inff(), "huber_k must be finite and not negative");
  PICP_REQUIRE(who, color_huber_k >= 0.0f && color_huber_k < __builtin_inff(),
               "color_huber_k must be finite and not negative");
  return GS_OK;
}

extern "C" int gs_projective_icp_color_weighted_batch_f32(const gs_picp_color_seq* seqs_host,
                                                          const float* const* weights_host, float* const* deltas_host,
                                                          float* const* cdeltas_host, int B, int H, int W,
                                                          const gs_picp_params* params_host, float color_weight,
                                                          float huber_delta, float huber_k, float color_huber_delta,
                                                          float color_huber_k, void* stream) {
  if (const int err = pic_check_weighted(__func__, huber_delta, huber_k, color_huber_delta, color_huber_k)) return err;
  const PiScale sc = picp_scale_joint(huber_k, huber_delta, color_huber_k, color_huber_delta, deltas_host, cdeltas_host,
                                      nullptr, nullptr);
  return picp_solve<PiJoint>(__func__, seqs_host, nullptr, B, H, W, params_host, color_weight, huber_delta,
                             color_huber_delta, sc.on[PS_GEO] || sc.on[PS_COLOR] ? &sc : nullptr, stream, weights_host,
                             true);
}

extern "C" int gs_projective_icp_color_weighted_rows_f32(const gs_picp_color_seq* seq_host, const float* weights, int H,
                                                         int W, int stride, float dist_th, float dot_th,
                                                         float color_weight, float huber_delta, float huber_k,
                                                         float color_huber_delta, float color_huber_k, int32_t* code,
                                                         int64_t* row, float* a6, float* b, float* ac6, float* bc,
                                                         int32_t* colored, float* weight, float* color_weight_out,
                                                         double* sums28, int64_t* count, int64_t* color_count,
                                                         float* delta_out, float* cdelta_out, void* stream) {
  if (const int err = pic_check_weighted(__func__, huber_delta, huber_k, color_huber_delta, color_huber_k)) return err;
  const PiScale sc = picp_scale_joint(huber_k, huber_delta, color_huber_k, color_huber_delta, nullptr, nullptr, delta_out,
                                      cdelta_out);
  return picp_rows<PiJoint>(__func__, seq_host, H, W, stride, dist_th, dot_th, color_weight,
                            PiRobust{huber_delta, color_huber_delta, weight, color_weight_out},
                            PiRowsOut{code, row, a6, b, ac6, bc, colored, sums28, count, color_count},
                            sc.on[PS_GEO] || sc.on[PS_COLOR] ? &sc : nullptr, stream, weights, true);
}
