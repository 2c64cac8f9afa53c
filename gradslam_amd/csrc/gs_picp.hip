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
// The scaled entries (gs_projective_icp_scaled_batch_f32 / _rows_f32, huber_k > 0) put the two launches of
// gs_picp_scale.hip in front of the robust linearisation: the kernel then reads its sequence's threshold of this iteration,
// max(huber_k * 1.4826 * lower median |b|, huber_floor), from a device float (PiSeq::delta_dev; NULL: the constant above),
// and the finish kernel tapes it in PiTapeRow::pad[0].
// The weighted entries (gs_projective_icp_weighted_batch_f32 / _rows_f32): one optional float32 image of PIXEL WEIGHTS
// per sequence, read at the pixel of each lattice slot.  The rule, per slot with pixel p and wp = weight[p]:
//   1  depth[p] > 0, else code 1, as above
//   6  wp > 0 && wp < +inf in float32, else code 6 ("masked"): zero, negative, NaN and +inf all mask; nothing is
//      validated on the host, nothing is read back.  A masked slot is not associated, not counted as an inlier, not part
//      of any median; it contributes +0.0 to every term and has no colour row
//   2 .. 5 as above
//   a used slot's total weight is wt = wp * h, ONE float32 product, h the Huber weight of its raw residual b
//   (pi_huber_weight; 1.0f without a threshold; the clip flag is taken from the unweighted float32 b), and every one of
//   its 28 terms is pi_term(wt, x, y); in the joint solve the colour products carry wp * wc in the same way.
//   The inlier count stays the integer number of used slots, S[27] is the weighted sum of squares; with huber_k the
//   median is that of the unweighted |b| of the used slots (masked slots excluded).  The reduction shape, the finish
//   kernel, the solve, the update and "no inlier keeps the pose bits" are untouched.
// They launch the WEIGHTED instance of the linearise body (and of the residual pass), one 4-byte load per slot more than
// the robust one.  Two consequences, bit for bit: weights of all 1.0f give the unweighted entries' bits ((double)1.0f *
// (x y) is the exact product), and weight 0 on a set of pixels gives the bits of depth 0 on those pixels (the code
// tables differ in 6 against 1).  A sequence whose weights pointer is NULL has no weights.
// What this file holds: the body of the linearise kernel with its two term expressions, the traits of the plain solve and
// the entries.  The block prologue (pi_prologue), the association (pi_associate), the chunk reduction (pi_chunk_reduce,
// PI_PAIRS), the column sum of the partials (pi_column_sums), the finish body (pi_finish) and the host drivers
// (picp_solve, picp_rows) are gs_picp_dev.h's, shared with gs_picp_color.hip and gs_picp_bwd.hip.
#include "gs_picp_dev.h"

// The linearise kernel's body: prologue, association, the row z = (a0 .. a5, b), the table outputs, the chunk reduction.
// ROBUST: every term of a used slot carries the Huber weight of its residual b (pi_huber_weight), which also goes to
// rb.weight_out (nslots, 0 for a slot that is not used) when asked for; the colour half of rb is ignored.
// WEIGHTED (with ROBUST): the weight of a used slot is wp * w, wp the slot's pixel weight (pi_associate<true>); a
// masked slot has code 6.
template <bool ROBUST, bool WEIGHTED = false>
GS_DEV void pi_linearize(const PiBatch& pb, const PiRobust& rb) {
  static_assert(ROBUST || !WEIGHTED, "the weighted instance carries its weight through the robust terms");
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  __shared__ int cnt[GS_PI_CHUNK / GS_WAVE];
  const PiSeq& q = pb.s[blockIdx.x % pb.g.B];
  const PiSlot t = pi_prologue(q.in, pb.g, q.T_in, cam, Ts);
  const int64_t n_map = gs_count(q.in.n);
  int code = 1;
  int64_t row = -1;
  float z[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, w = 1.0f;
  const float delta = ROBUST ? pi_huber_delta(q.delta_dev, rb) : 0.0f;
  if (t.in_lattice) {
    float s[3];
    float4 d, m;
    float wp;
    code = pi_associate<WEIGHTED>(Ts, cam, q.in, pb.g, n_map, t.p, row, s, d, m, wp);
    if (code == 0) gn_row_pn(s[0], s[1], s[2], d, m, z, z[6]);
    pi_table_out(q, t.k, code, row, z);
    if (ROBUST) {
      if (code == 0) w = pi_huber_weight(pi_huber_clipped(z[6], delta), z[6], delta);
      if (WEIGHTED && code == 0) w = wp * w;
      if (rb.weight_out) rb.weight_out[t.k] = code == 0 ? w : 0.0f;
    }
  }
  const bool used = code == 0;   // (z is zero otherwise: every term below is then +0.0)
  const unsigned long long mask = __ballot(used);
  if (t.lane == 0) cnt[t.wave] = __popcll(mask);
  double* partial_row = q.partials + (int64_t)t.chunk * LIN_NV;
  if constexpr (ROBUST)
    pi_chunk_reduce<LIN_NV>([&](const int i) { return pi_term(w, z[PI_PAIRS.x[i]], z[PI_PAIRS.y[i]]); }, mask != 0ull,
                            partial_row);
  else
    pi_chunk_reduce<LIN_NV>([&](const int i) { return (double)z[PI_PAIRS.x[i]] * (double)z[PI_PAIRS.y[i]]; }, mask != 0ull,
                            partial_row);
  if (threadIdx.x == GS_WAVE) q.counts[t.chunk] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_linearize_kernel(const PiBatch pb) {
  pi_linearize<false>(pb, PiRobust{0.0f, 0.0f, nullptr, nullptr});
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_robust_picp_linearize_kernel(const PiBatch pb, const PiRobust rb) {
  pi_linearize<true>(pb, rb);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_weighted_picp_linearize_kernel(const PiBatch pb, const PiRobust rb) {
  pi_linearize<true, true>(pb, rb);
}

__global__ void __launch_bounds__(GS_PI_FIN) gs_picp_finish_kernel(const PiBatch pb) {
  pi_finish<false>(pb.s[blockIdx.x], pb.g.nchunks, pb.g.damp, nullptr, nullptr);
}

extern "C" int64_t gs_projective_icp_scratch_bytes(int H, int W, int stride) {
  if (H <= 0 || W <= 0 || stride <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  const int64_t nchunks = gs_ceil_div(picp_slots(H, W, stride), GS_PI_CHUNK);
  return (int64_t)(picp_partials_bytes(nchunks) + picp_counts_bytes(nchunks));
}

extern "C" int64_t gs_projective_icp_scaled_scratch_bytes(int H, int W, int stride) {
  const int64_t base = gs_projective_icp_scratch_bytes(H, W, stride);
  return base > 0 ? (int64_t)picp_scaled_bytes((size_t)base, picp_slots(H, W, stride)) : 0;
}

extern "C" int64_t gs_projective_icp_tape_bytes(int numiters) {
  return numiters >= 1 ? (int64_t)numiters * (int64_t)sizeof(PiTapeRow) : 0;
}

// the traits of the plain solve for the drivers of gs_picp_dev.h
struct PiPlain {
  using Seq = gs_picp_seq;
  using Batch = PiBatch;
  static constexpr int TRACE = GS_PI_TRACE;
  static constexpr auto linearize = gs_picp_linearize_kernel;
  static constexpr auto robust_linearize = gs_robust_picp_linearize_kernel;
  static constexpr auto weighted_linearize = gs_weighted_picp_linearize_kernel;
  static constexpr auto finish = gs_picp_finish_kernel;
  static const gs_picp_seq& base(const Seq& u) { return u; }
  static PiSeq& seq(Batch& pb, int b) { return pb.s[b]; }
  static int check(const char* who, const Seq& u) {
    PICP_CHECK_SEQ(who, u);
    return GS_OK;
  }
  static void fill(Batch& pb, int b, const Seq& u, float) { picp_fill_seq(pb.s[b], u, pb.g.nchunks); }
  static size_t scratch_bytes(int64_t nchunks) { return picp_partials_bytes(nchunks) + picp_counts_bytes(nchunks); }
  static void color_outputs(Batch&, const PiRowsOut&) {}
  static void color_scale(Batch&, int, PiScaleSeq& z, bool) { z.color = nullptr; z.model = nullptr; }
};

extern "C" int gs_projective_icp_batch_f32(const gs_picp_seq* seqs_host, int B, int H, int W,
                                           const gs_picp_params* params_host, void* stream) {
  return picp_solve<PiPlain>(__func__, seqs_host, nullptr, B, H, W, params_host, 0.0f, 0.0f, 0.0f, nullptr, stream);
}

extern "C" int gs_projective_icp_tape_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                                                const gs_picp_params* params_host, void* stream) {
  GS_REQUIRE(tapes_host, "NULL pointer (tapes)");
  return picp_solve<PiPlain>(__func__, seqs_host, tapes_host, B, H, W, params_host, 0.0f, 0.0f, 0.0f, nullptr, stream);
}

extern "C" int gs_projective_icp_robust_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H,
                                                  int W, const gs_picp_params* params_host, float huber_delta,
                                                  void* stream) {
  return picp_solve<PiPlain>(__func__, seqs_host, tapes_host, B, H, W, params_host, 0.0f, huber_delta, 0.0f, nullptr, stream);
}

extern "C" int gs_projective_icp_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                          float dot_th, int32_t* code, int64_t* row, float* a6, float* b,
                                          double* sums28, int64_t* count, void* stream) {
  return picp_rows<PiPlain>(__func__, seq_host, H, W, stride, dist_th, dot_th, 0.0f, PiRobust{0.0f, 0.0f, nullptr, nullptr},
                            PiRowsOut{code, row, a6, b, nullptr, nullptr, nullptr, sums28, count, nullptr}, nullptr, stream);
}

extern "C" int gs_projective_icp_robust_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                                 float dot_th, float huber_delta, int32_t* code, int64_t* row, float* a6,
                                                 float* b, float* weight, double* sums28, int64_t* count, void* stream) {
  return picp_rows<PiPlain>(__func__, seq_host, H, W, stride, dist_th, dot_th, 0.0f,
                            PiRobust{huber_delta, 0.0f, weight, nullptr},
                            PiRowsOut{code, row, a6, b, nullptr, nullptr, nullptr, sums28, count, nullptr}, nullptr, stream);
}

// The scaled entries: the Huber threshold of every sequence and iteration from the lower median of |b| over its used
// slots (gs_picp_scale.hip: two launches in front of the robust linearisation), delta = max(c * median, huber_floor).
extern "C" int gs_projective_icp_scaled_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host,
                                                  float* const* deltas_host, int B, int H, int W,
                                                  const gs_picp_params* params_host, float huber_k, float huber_floor,
                                                  void* stream) {
  PICP_CHECK_SCALE(__func__, huber_k, huber_floor);
  const PiScale sc = picp_scale_geo(huber_k, huber_floor, deltas_host, nullptr);
  return picp_solve<PiPlain>(__func__, seqs_host, tapes_host, B, H, W, params_host, 0.0f, 0.0f, 0.0f, &sc, stream);
}

extern "C" int gs_projective_icp_scaled_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                                 float dot_th, float huber_k, float huber_floor, int32_t* code,
                                                 int64_t* row, float* a6, float* b, float* weight, double* sums28,
                                                 int64_t* count, float* delta_out, void* stream) {
  PICP_CHECK_SCALE(__func__, huber_k, huber_floor);
  const PiScale sc = picp_scale_geo(huber_k, huber_floor, nullptr, delta_out);
  return picp_rows<PiPlain>(__func__, seq_host, H, W, stride, dist_th, dot_th, 0.0f,
                            PiRobust{0.0f, 0.0f, weight, nullptr},
                            PiRowsOut{code, row, a6, b, nullptr, nullptr, nullptr, sums28, count, nullptr}, &sc, stream);
}

// The weighted entries: pixel weights next to any of the thresholds above.  huber_k > 0: the median rule, huber_delta its
// floor (the scratch is then the scaled entries'); else huber_delta is the constant threshold (0: none).  tapes_host /
// deltas_host as in the scaled entry (either may be NULL; deltas_host is read with huber_k > 0 only).
static int pi_check_weighted(const char* who, float huber_delta, float huber_k) {
  PICP_CHECK_DELTA(who, huber_delta, "huber_delta");
  PICP_REQUIRE(who, huber_k >= 0.0f && huber_k < __builtin_inff(), "huber_k must be finite and not negative");
  return GS_OK;
}

extern "C" int gs_projective_icp_weighted_batch_f32(const gs_picp_seq* seqs_host, const float* const* weights_host,
                                                    void* const* tapes_host, float* const* deltas_host, int B, int H,
                                                    int W, const gs_picp_params* params_host, float huber_delta,
                                                    float huber_k, void* stream) {
  if (const int err = pi_check_weighted(__func__, huber_delta, huber_k)) return err;
  const PiScale sc = picp_scale_geo(huber_k, huber_delta, deltas_host, nullptr);
  return picp_solve<PiPlain>(__func__, seqs_host, tapes_host, B, H, W, params_host, 0.0f, sc.on[PS_GEO] ? 0.0f : huber_delta,
                             0.0f, sc.on[PS_GEO] ? &sc : nullptr, stream, weights_host, true);
}

extern "C" int gs_projective_icp_weighted_rows_f32(const gs_picp_seq* seq_host, const float* weights, int H, int W,
                                                   int stride, float dist_th, float dot_th, float huber_delta,
                                                   float huber_k, int32_t* code, int64_t* row, float* a6, float* b,
                                                   float* weight, double* sums28, int64_t* count, float* delta_out,
                                                   void* stream) {
  if (const int err = pi_check_weighted(__func__, huber_delta, huber_k)) return err;
  const PiScale sc = picp_scale_geo(huber_k, huber_delta, nullptr, delta_out);
  return picp_rows<PiPlain>(__func__, seq_host, H, W, stride, dist_th, dot_th, 0.0f,
                            PiRobust{sc.on[PS_GEO] ? 0.0f : huber_delta, 0.0f, weight, nullptr},
                            PiRowsOut{code, row, a6, b, nullptr, nullptr, nullptr, sums28, count, nullptr},
                            sc.on[PS_GEO] ? &sc : nullptr, stream, weights, true);
}
