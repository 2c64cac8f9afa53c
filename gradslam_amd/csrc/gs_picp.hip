// gs_picp.hip — frame-to-model tracking by projective data association (Keller et al. / KinectFusion): every live pixel
// of the [::stride, ::stride] lattice is carried by the current pose estimate into the model view (gs_render.hip's index
// image at the model pose), its correspondence is the surfel that won that pixel, and a point-to-plane Gauss-Newton step
// with constant damping follows.  No grid, no lists, no search: an iteration is two launches,
//
//   linearise  one thread per lattice slot (256 per block = one chunk): the slot's row (a[6], b) or a reject code, the 28
//              float64 terms of the normal equations, one partial row per chunk in the caller's scratch
//   finish     one block per sequence: the partial rows added up, the 6x6 solve, se3_exp, T <- Tr T, the trace row
//
// and the launch boundary is the dependency between them (the cheapest one here).  All numiters
// iterations are enqueued back to back; nothing is read back, the map's device count is read on the device.
//
// Arithmetic (-ffp-contract=off; tests/picp_ref.py restates it with the oracle), slot k = i * Wl + j, Wl = ceil(W / stride),
// pixel (h, w) = (i stride, j stride):
//   1  depth[h, w] > 0                                              else code 1 (NaN fails too)
//   s  = gs_rigid_fma(T, v)          g_j = gs_dot3_fma(T[4j], T[4j+1], T[4j+2], n)      (live vertex / normal under T)
//   2  gs_project_point_hw(gs_camera(model_pose, K), s) = (h', w')  else code 2
//   3  row = index[h', w'],  0 <= row < min(device count, bound)    else code 3 (a stale index is never dereferenced)
//   4  the gate of gs_is_similar_v: gs_norm3(s - p[row]) < dist_th  else code 4, gs_dot3_plain(g, n[row]) > dot_th else 5
//   (a, b) = gn_row_pn(s, p[row], n[row]);  terms: 21 a_i a_j (i <= j), 6 a_i b, b b as (double)x * (double)y (exact);
//   a rejected slot contributes +0.0 to every term.
// Reduction (its order is part of the contract: no float atomics, bitwise reproducible): inside a chunk of 256 slots a
// pairwise adjacent tree of 8 levels -- an xor butterfly over 1, 2, 4, 8, 16, 32 in each wave (lane l adds the value of
// lane l ^ d: both lanes of a pair form the same sum, a + b == b + a), then (w0 + w1) + (w2 + w3) over the four waves;
// slots beyond the lattice are +0.0.  The chunk partials are added in ascending chunk order starting from the first.
// The inlier count is an integer sum.
// The taped entry (gs_projective_icp_tape_batch_f32) is the same two kernels: the finish kernel also writes the pose it
// read, the 28 sums, the step and the inlier count of every iteration to the caller's tape (PiTapeRow), which is all the
// backward pass (gs_picp_bwd.hip) needs besides the inputs.  The pose bits are those of the untaped call.
// The robust entries (gs_projective_icp_robust_batch_f32 / _rows_f32, huber_delta > 0) launch the ROBUST instance of the
// linearise body: w = |b| > delta ? delta / |b| : 1 in float32 (pi_huber_weight), every term (double)w * ((double)x *
// (double)y); the finish kernel, the reduction and the counts are the plain ones, S[27] is the weighted sum of squares.
// With delta = 0 they launch the plain kernel.
#include "gs_picp_dev.h"

// The linearise kernel's body.  ROBUST: every term of a used slot carries the Huber weight of its residual b
// (pi_huber_weight, gs_picp_dev.h), which also goes to weight_out (nslots, 0 for a slot that is not used) when asked for;
// the plain instance is the kernel as it was.
template <bool ROBUST>
GS_DEV void pi_linearize(const PiBatch& pb, const float delta, float* __restrict__ weight_out) {
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  __shared__ double red[GS_PI_CHUNK / GS_WAVE][LIN_NV];
  __shared__ int cnt[GS_PI_CHUNK / GS_WAVE];
  const PiSeq& q = pb.s[blockIdx.x % pb.g.B];
  const int chunk = blockIdx.x / pb.g.B;
  if (threadIdx.x == 0) cam = gs_camera(q.model_pose16, q.K16);
  if (threadIdx.x >= GS_WAVE && threadIdx.x < GS_WAVE + 12) Ts[threadIdx.x - GS_WAVE] = q.T_in[threadIdx.x - GS_WAVE];
  __syncthreads();
  const int lane = threadIdx.x & (GS_WAVE - 1), wave = threadIdx.x / GS_WAVE;
  const int k = chunk * GS_PI_CHUNK + (int)threadIdx.x;
  const bool in_lattice = k < pb.g.nslots;
  const int64_t n_map = gs_count(q.n);
  int code = 1;
  int64_t row = -1;
  float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, b = 0.0f, w = 1.0f;
  if (in_lattice) {
    const int i = k / pb.g.Wl, j = k - i * pb.g.Wl;
    const int64_t p = (int64_t)(i * pb.g.stride) * pb.g.W + j * pb.g.stride;
    float s[3];
    float4 d, m;
    code = pi_associate(Ts, cam, q.vertex, q.normal, q.depth, q.index, q.points, q.normals, n_map, p, pb.g.H, pb.g.W,
                        pb.g.u_hi, pb.g.v_hi, pb.g.dist_th, pb.g.dot_th, row, s, d, m);
    if (code == 0) gn_row_pn(s[0], s[1], s[2], d, m, a, b);
    if (q.code_out) q.code_out[k] = code;
    if (q.row_out) q.row_out[k] = row;
    if (q.a_out) {
#pragma unroll
      for (int c = 0; c < 6; ++c) q.a_out[6 * (int64_t)k + c] = a[c];
    }
    if (q.b_out) q.b_out[k] = b;
    if (ROBUST) {
      if (code == 0) w = pi_huber_weight(pi_huber_clipped(b, delta), b, delta);
      if (weight_out) weight_out[k] = code == 0 ? w : 0.0f;
    }
  }
  const bool used = code == 0;   // (a, b are zero otherwise: every term below is then +0.0)
  const unsigned long long mask = __ballot(used);
  if (lane == 0) cnt[wave] = __popcll(mask);
  // a wave without a used slot adds up +0.0 only: its sums are +0.0, no shuffle needed
  const bool any = mask != 0ull;
  int t = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = r; c < 6; ++c) {
      const double x = pi_wave_tree(ROBUST ? pi_term(w, a[r], a[c]) : (double)a[r] * (double)a[c], any);
      if (lane == 0) red[wave][t] = x;
      ++t;
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double x = pi_wave_tree(ROBUST ? pi_term(w, a[r], b) : (double)a[r] * (double)b, any);
    if (lane == 0) red[wave][21 + r] = x;
  }
  {
    const double x = pi_wave_tree(ROBUST ? pi_term(w, b, b) : (double)b * (double)b, any);
    if (lane == 0) red[wave][27] = x;
  }
  __syncthreads();
  if (threadIdx.x < LIN_NV)
    q.partials[(int64_t)chunk * LIN_NV + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  if (threadIdx.x == GS_WAVE) q.counts[chunk] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_linearize_kernel(const PiBatch pb) {
  pi_linearize<false>(pb, 0.0f, nullptr);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_robust_picp_linearize_kernel(const PiBatch pb, const float delta,
                                                                               float* __restrict__ weight_out) {
  pi_linearize<true>(pb, delta, weight_out);
}

__global__ void __launch_bounds__(GS_PI_FIN) gs_picp_finish_kernel(const PiBatch pb) {
  pi_finish<false>(pb.s[blockIdx.x], pb.g.nchunks, pb.g.damp, nullptr, nullptr);   // (the body: gs_picp_dev.h)
}

extern "C" int64_t gs_projective_icp_scratch_bytes(int H, int W, int stride) {
  if (H <= 0 || W <= 0 || stride <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  const int64_t nchunks = gs_ceil_div(picp_slots(H, W, stride), GS_PI_CHUNK);
  return (int64_t)(picp_partials_bytes(nchunks) + picp_counts_bytes(nchunks));
}

extern "C" int64_t gs_projective_icp_tape_bytes(int numiters) {
  return numiters >= 1 ? (int64_t)numiters * (int64_t)sizeof(PiTapeRow) : 0;
}

// the solve behind the batch entries; tapes_host: per sequence the device buffer of numiters tape rows, or NULL
// (untaped); delta: the Huber threshold of the robust entry (0: the plain kernel)
static int picp_solve(const char* who, const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                      const gs_picp_params* params_host, float delta, void* stream) {
  PICP_REQUIRE(who, seqs_host && params_host && B > 0 && H > 0 && W > 0, "bad arguments");
  PICP_REQUIRE(who, (int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  const gs_picp_params& prm = *params_host;
  PICP_CHECK_PARAMS(who, prm);
  PICP_CHECK_DELTA(who, delta, "huber_delta");
  for (int b = 0; b < B; ++b) {
    PICP_CHECK_SEQ(who, seqs_host[b]);
    PICP_REQUIRE(who, seqs_host[b].out_pose16, "NULL pointer (out_pose16)");
    PICP_REQUIRE(who, !tapes_host || (tapes_host[b] && ((uintptr_t)tapes_host[b] & 7) == 0), "NULL or misaligned tape");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    PiBatch pb;
    pb.g.B = nb;
    picp_fill(pb.g, H, W, prm.stride, prm.dist_th, prm.dot_th, prm.damp);
    for (int b = 0; b < nb; ++b) {
      picp_fill_seq(pb.s[b], seqs_host[c0 + b], pb.g.nchunks);
      pb.s[b].T_out = seqs_host[c0 + b].out_pose16;
    }
    const unsigned blocks = (unsigned)nb * (unsigned)pb.g.nchunks;   // < 8 * 2^23
    for (int it = 0; it < prm.numiters; ++it) {
      for (int b = 0; b < nb; ++b) {
        const gs_picp_seq& u = seqs_host[c0 + b];
        pb.s[b].T_in = it == 0 ? u.init_pose16 : u.out_pose16;
        pb.s[b].trace_row = u.trace ? u.trace + (int64_t)GS_PI_TRACE * it : nullptr;
        pb.s[b].tape_row = tapes_host ? static_cast<PiTapeRow*>(tapes_host[c0 + b]) + it : nullptr;
      }
      if (delta > 0.0f)
        hipLaunchKernelGGL(gs_robust_picp_linearize_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, delta,
                           static_cast<float*>(nullptr));
      else
        hipLaunchKernelGGL(gs_picp_linearize_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb);
      hipLaunchKernelGGL(gs_picp_finish_kernel, dim3(nb), dim3(GS_PI_FIN), 0, st, pb);
    }
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}

extern "C" int gs_projective_icp_batch_f32(const gs_picp_seq* seqs_host, int B, int H, int W,
                                           const gs_picp_params* params_host, void* stream) {
  return picp_solve(__func__, seqs_host, nullptr, B, H, W, params_host, 0.0f, stream);
}

extern "C" int gs_projective_icp_tape_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                                                const gs_picp_params* params_host, void* stream) {
  GS_REQUIRE(tapes_host, "NULL pointer (tapes)");
  return picp_solve(__func__, seqs_host, tapes_host, B, H, W, params_host, 0.0f, stream);
}

extern "C" int gs_projective_icp_robust_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H,
                                                  int W, const gs_picp_params* params_host, float huber_delta,
                                                  void* stream) {
  return picp_solve(__func__, seqs_host, tapes_host, B, H, W, params_host, huber_delta, stream);
}

// the linearisation behind both table-level entries; weight: the robust entry's output, or NULL
static int picp_rows(const char* who, const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th, float dot_th,
                     float delta, int32_t* code, int64_t* row, float* a6, float* b, float* weight, double* sums28,
                     int64_t* count, void* stream) {
  PICP_REQUIRE(who, seq_host && H > 0 && W > 0, "bad arguments");
  PICP_REQUIRE(who, (int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  PICP_REQUIRE(who, stride >= 1, "stride must be at least 1");
  PICP_REQUIRE(who, !(dist_th != dist_th) && !(dot_th != dot_th), "a threshold is NaN");
  PICP_CHECK_DELTA(who, delta, "huber_delta");
  PICP_CHECK_SEQ(who, *seq_host);
  hipStream_t st = gs_stream(stream);
  PiBatch pb;
  pb.g.B = 1;
  picp_fill(pb.g, H, W, stride, dist_th, dot_th, 1.0f);
  picp_fill_seq(pb.s[0], *seq_host, pb.g.nchunks);
  pb.s[0].code_out = code; pb.s[0].row_out = row; pb.s[0].a_out = a6; pb.s[0].b_out = b;
  pb.s[0].sums_out = sums28; pb.s[0].count_out = count;
  if (delta > 0.0f || weight)   // (delta == 0 with a weight table: the robust kernel writes 1 for every used slot)
    hipLaunchKernelGGL(gs_robust_picp_linearize_kernel, dim3((unsigned)pb.g.nchunks), dim3(GS_PI_CHUNK), 0, st, pb, delta,
                       weight);
  else
    hipLaunchKernelGGL(gs_picp_linearize_kernel, dim3((unsigned)pb.g.nchunks), dim3(GS_PI_CHUNK), 0, st, pb);
  if (sums28 || count) hipLaunchKernelGGL(gs_picp_finish_kernel, dim3(1), dim3(GS_PI_FIN), 0, st, pb);
  GS_LAUNCH_CHECK();
  return GS_OK;
}

extern "C" int gs_projective_icp_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                          float dot_th, int32_t* code, int64_t* row, float* a6, float* b,
                                          double* sums28, int64_t* count, void* stream) {
  return picp_rows(__func__, seq_host, H, W, stride, dist_th, dot_th, 0.0f, code, row, a6, b, nullptr, sums28, count,
                   stream);
}

extern "C" int gs_projective_icp_robust_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                                 float dot_th, float huber_delta, int32_t* code, int64_t* row, float* a6,
                                                 float* b, float* weight, double* sums28, int64_t* count, void* stream) {
  return picp_rows(__func__, seq_host, H, W, stride, dist_th, dot_th, huber_delta, code, row, a6, b, weight, sums28,
                   count, stream);
}
