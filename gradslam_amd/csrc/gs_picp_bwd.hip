// gs_picp_bwd.hip — backward pass of the projective-association ICP (gs_picp.hip): reverse-mode differentiation of its
// numiters Gauss-Newton iterations given the forward tape (gs_projective_icp_tape_batch_f32), from dL/dT to the live
// vertex map, the map points, the map normals and the initial pose.
//
// What is differentiated, for iteration k with pose T_k = [R | t] (the taped float32 bits), per used slot with live
// vertex v, map row `row`, p = points[row], m = normals[row]:
//   s = R v + t,  a = [m ; s x m],  b = m . (p - s),  A = sum a a^T,  g = sum a b,  xi = (A + damp I)^-1 g,
//   T_{k+1} = exp(xi) T_k.
// Constants of the differentiation, as in the render and fuse backward: which slots are used and their rows (the reject
// codes, both gates, the projection into the model view, the index image), the device count, K, model_pose, depth and the
// live normal (it only feeds the gate).  The float32 roundings of the forward are treated as the identity.  The
// association is NOT taped: the point stage recomputes it with the forward's own device function (pi_associate,
// gs_picp_dev.h) at the taped float32 pose, so it is the forward's association exactly, and a stale index entry is
// still never dereferenced.
//
// One step backwards, given Tb = dL/dT_{k+1}:
//   scalar stage (one block per sequence)   Tb += the 12 sums of the point stage of iteration k + 1 (chunk partials in
//       ascending order); without inliers Tb passes through; else xib = adjoint of exp at xi applied to Tb T_k^T,
//       u = (A + damp I)^-1 xib, Tb <- exp(xi)^T Tb
//   point stage (one thread per lattice slot, 256 per block = one chunk)   c = xi . a, e = u . a,
//       ab = (b - c) u - e xi, w = ab[3:6], sb = m x w - e m;  points_bar[row] += e m;
//       normals_bar[row] += ab[0:3] + w x s + e (p - s);  vertex_bar[slot] += R^T sb;  12 sums of sb [v^T 1]
// and after iteration 0 a last scalar stage adds the sums of its point stage: init_pose_bar = Tb (top three rows, a zero
// bottom row).  Where no point stage contributed nothing is added: with no inlier in any iteration init_pose_bar is the
// upstream adjoint's top three rows bit for bit, a -0.0 included.  2 numiters + 1 launches per 8 sequences, enqueued back
// to back, nothing read back.
//
// All arithmetic is float64, rounded to float32 once at the end.  The 12 sums use the forward's reduction shape (an xor
// tree per wave, (w0 + w1) + (w2 + w3), chunk partials in ascending order; no float atomics) and vertex_bar is
// accumulated per slot by the slot's own thread across the serialised iterations (a slot is its own pixel): vertex_bar
// and init_pose_bar are BITWISE REPRODUCIBLE.  Several slots can land on the same surfel, so points_bar and normals_bar
// are by default float64 atomic adds into float64 (n_bound, 3) buffers, rounded once: reproducible up to the order of the
// float64 additions.  The ORDERED mode (gs_projective_icp_ordered_backward_batch_f32; the Python layer takes it under
// GRADSLAM_HIP_DETERMINISTIC_BACKWARD or deterministic=True) makes them bitwise reproducible as well; see "ordered mode"
// below.
// Every output may be NULL: its work and its buffer are skipped; with both map outputs NULL nothing of map size is
// touched.
// gs_projective_icp_robust_backward_batch_f32 (a tape of the forward with Huber weights, the same huber_delta) launches
// the ROBUST instance of the point stage (see pb_point); everything else, the scalar stage included, is shared.
// gs_projective_icp_scaled_backward_batch_f32 (a tape of the forward with the threshold from the residuals' median) launches
// the same instance, which then reads every iteration's threshold from its tape row.
// From gs_picp_dev.h, ONE definition with the forward: the inputs and the geometry of a launch (PiInputs, PiGeom), the
// point stage's block prologue (pi_prologue), pi_associate, the chunk reduction (pi_chunk_reduce, here with 12 terms) and
// the scalar stage's column sum of the chunk partials (pi_column_sums, here starting from 0.0).
//
// Ordered mode.  The RECORD instances of the point stage do not add a slot's two 3-vectors atomically: they record them,
// contrib[k][0:6] (float64: the contribution to points_bar[row], then the one to normals_bar[row]) and key[k] = the
// slot's row, or 0x7fffffff for a slot that contributes nothing.  A settle step follows each point stage: ONE stable
// radix sort of the (sequence << 32 | key, slot) pairs of all sequences of the launch group (hipcub, 35 key bits), then
// one thread per run of equal keys adds the run up and adds the sum to the row's float64 accumulator.  Two more launches
// and a sort per iteration for up to 8 sequences; the record and the sort buffers are per-iteration scratch, reused.
// The order contract (tests/picp_ordered_ref.py restates it, tests/test_hip_picp_ordered_backward.py pins the bits):
//   * acc[row] starts at +0.0; a row that nobody touches ends as +0.0;
//   * the iterations are processed in launch order, numiters - 1 down to 0;
//   * in an iteration a row's run sum starts at 0.0 and adds the contributions of its slots in ascending slot id, then
//     acc[row] = acc[row] + run_sum;
//   * an iteration without inliers (state->active == 0) records no contribution: the point stage writes the key "none"
//     for every slot of the lattice in every launch, so nothing of the iteration before is seen again;
//   * slot ids at or beyond nslots in the tail of the last chunk write nothing; a stale index entry is rejected by
//     pi_associate as ever and never recorded;
//   * the accumulators are rounded to float32 once at the end;
//   * vertex_bar, init_pose_bar, the scalar stage and the 12 sums are those of the atomic mode, bit for bit (the slot's
//     arithmetic is ONE definition, pb_point).
// With no map output asked for in a launch group the group runs the atomic mode's launches: nothing is recorded or sorted.
//
// Pixel weights (gs_projective_icp_weighted_backward_batch_f32, a tape of the weighted forward; the rule is in
// gs_picp.hip's header).  With wp the slot's pixel weight and h the Huber weight of its residual (1 without a threshold)
// the system is A = sum wp h a a^T, g = sum wp h a b.  The WEIGHTED instances of the point stage take, with the scalar
// stage's u and xi unchanged, e = u . a and c = xi . a as above:
//   pixel_weights_bar[p] += h e (b - c);   ab is multiplied by wp h;   the residual's adjoint is e wp (h + h' (b - c))
// (h' as in the ROBUST instance, 0 without a threshold).  Which slots are masked (code 6 of pi_associate<true>) is a
// constant of the pass like the association and the clip flags.  A slot is its own pixel and the iterations are
// serialised, so pixel_weights_bar accumulates like vertex_bar: float64 per slot (wacc), no atomics, rounded once:
// BITWISE REPRODUCIBLE in the atomic and in the ordered mode, and the same bits in both (ONE definition, pb_point; the
// ordered mode's records are the weighted contributions).  Pixels off the lattice, masked slots and slots never used get
// +0.0.  Not asked for (NULL): no work, no store, and the sequence's scratch is that of the unweighted entry.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "gs_picp_dev.h"
#include "gs_se3_f64.h"

constexpr int PB_NV = 12;          // 3x3 outer-product sum + 3-vector sum

struct PbState {       // per sequence, between the launches
  double Tb[12];       // dL/dT of the iteration boundary being crossed, without the sums of the point stage after it
  double u[6];         // scalar stage -> point stage
  double xi[6];
  int32_t active;      // 0: the iteration had no inlier (nothing flows through its step)
  int32_t pad;
};

struct PbSeq {
  PiInputs in;
  const PiTapeRow* tape;
  const float* pose_bar16;
  float* vertex_bar;        // (H, W, 3) or NULL
  float* init_pose_bar16;   // (16) or NULL
  PbState* state;
  double* partials;         // (nchunks, 12)
  double* vacc;             // (nslots, 3) or NULL (no vertex_bar)
  double* pbar;             // (n_bound, 3) or NULL
  double* mbar;             // (n_bound, 3) or NULL
  float* weights_bar;       // (H, W) or NULL (the weighted entry)
  double* wacc;             // (nslots) or NULL (no weights_bar)
};
struct PbBatch {
  PbSeq s[GS_MAX_BATCH];
  PiGeom g;
};
// ordered mode: what the RECORD instances of the point stage write, per launch group (slot k of sequence b is pair
// b nslots + k of the sort)
constexpr int32_t PB_NO_KEY = 0x7fffffff;
struct PbRecord {
  double* contrib[GS_MAX_BATCH];   // (nslots, 6): a used slot's contributions to points_bar[row] and normals_bar[row]
  int32_t* key[GS_MAX_BATCH];      // (nslots): the slot's row, or PB_NO_KEY
  uint64_t* sort_key;              // (B nslots): sequence << 32 | key
};
// ... and what the settle step needs of the group
struct PbSettle {
  const double* contrib[GS_MAX_BATCH];
  double* pbar[GS_MAX_BATCH];
  double* mbar[GS_MAX_BATCH];
  int64_t nslots;
};

// Scalar stage in front of the point stage of iteration `it` (it == -1: the last one, which only hands out
// init_pose_bar).  have_sums: a point stage ran before (false for the first launch, whose Tb is the upstream adjoint).
__global__ void __launch_bounds__(GS_PI_FIN) gs_picp_bwd_scalar_kernel(const PbBatch pb, const int it, const int have_sums) {
  __shared__ double G[PB_NV];
  const PbSeq& q = pb.s[blockIdx.x];
  const int tid = threadIdx.x;
  // The sums are added only where a point stage contributed: behind an iteration without inliers (and in front of the
  // first one) Tb keeps its bits -- x + 0.0 would turn a -0.0 of the upstream adjoint into +0.0.  (state->active is the
  // flag of the point stage that ran last; this launch rewrites it only after every thread has passed the barrier below.)
  const bool add_sums = have_sums && q.state->active != 0;
  if (add_sums) {   // (block-uniform) column i in ascending chunk order, the chain starting from 0.0
    const double s = pi_column_sums<PB_NV, false>(q.partials, pb.g.nchunks);
    if (tid < PB_NV) G[tid] = s;
  } else if (tid < PB_NV) {
    G[tid] = 0.0;
  }
  __syncthreads();
  if (tid != 0) return;
  double Tb[16];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j)
      Tb[4 * i + j] = have_sums ? q.state->Tb[4 * i + j] : (double)q.pose_bar16[4 * i + j];
    if (add_sums) {
      for (int j = 0; j < 3; ++j) Tb[4 * i + j] += G[3 * i + j];
      Tb[4 * i + 3] += G[9 + i];
    }
  }
  for (int j = 0; j < 4; ++j) Tb[12 + j] = 0.0;
  if (it < 0) {
    if (q.init_pose_bar16) {
      for (int i = 0; i < 12; ++i) q.init_pose_bar16[i] = (float)Tb[i];
      for (int j = 0; j < 4; ++j) q.init_pose_bar16[12 + j] = 0.0f;
    }
    return;
  }
  const PiTapeRow& tr = q.tape[it];
  PbState& st = *q.state;
  if (tr.count <= 0) {   // no inlier: T_{k+1} = T_k, the adjoint passes through
    for (int i = 0; i < 12; ++i) st.Tb[i] = Tb[i];
    for (int i = 0; i < 6; ++i) { st.u[i] = 0.0; st.xi[i] = 0.0; }
    st.active = 0;
    return;
  }
  double xi[6], Tk[16], E[16], Eb[16], xb[6], u[6], Hm[36];
  for (int i = 0; i < 6; ++i) xi[i] = (double)tr.xi[i];
  for (int i = 0; i < 16; ++i) Tk[i] = (double)tr.T[i];
  // Eb = Tb T_k^T (the bottom row of Tb is zero), xib = the adjoint of exp at xi
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = 0.0;
      for (int m = 0; m < 4; ++m) acc += Tb[4 * i + m] * Tk[4 * j + m];
      Eb[4 * i + j] = acc;
    }
  d_se3_exp_adjoint(xi, Eb, xb);
  // u = (A + damp I)^-1 xib: the forward's system (the float32 roundings of S and of the damped diagonal included)
  int t = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      const float v = (float)tr.S[t];
      ++t;
      Hm[6 * r + c] = Hm[6 * c + r] = (double)(r == c ? v + pb.g.damp : v);
    }
  d_solve6(Hm, xb, u);
  // Tb <- exp(xi)^T Tb
  d_se3_exp(xi, E);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = 0.0;
      for (int m = 0; m < 3; ++m) acc += E[4 * m + i] * Tb[4 * m + j];
      st.Tb[4 * i + j] = acc;
    }
  for (int i = 0; i < 6; ++i) { st.u[i] = u[i]; st.xi[i] = xi[i]; }
  st.active = 1;
}

// Point stage of iteration `it`.  first: the first point stage of the call (vacc is written, not added to);
// last: iteration 0 (vertex_bar is rounded and stored).
// ROBUST (the forward ran with Huber weights, delta > 0): the taped S is the weighted system, so the scalar stage is
// unchanged; here the weight w(b) = delta / |b| of a clipped slot is differentiated, the clip flag is frozen like the
// association and recomputed as the forward computed it (pi_huber_clipped on the float32 b of gn_row_pn at the taped
// pose).  With w' = dw/db (-w / b clipped, 0 otherwise): ab = w ((b - c) u - e xi), and the residual's adjoint
// bb = e (w + w' (b - c)) takes the place of e in sb, points_bar and normals_bar.
// taped (the scaled backward): the threshold is not the launch's but the one the forward derived for this iteration and
// taped (PiTapeRow::pad[0], the median rule of gs_picp_scale.hip), a constant of the pass like the clip flags.
// RECORD (the ordered mode, rec != NULL): the two map contributions are not added atomically but stored in the slot's
// record (zeros for a map output that is not asked for), and EVERY slot of the lattice writes its key, used or not,
// active iteration or not.
// WEIGHTED (with ROBUST; the weighted entry): the slot's pixel weight wp enters as the header says, and the slot's
// contribution to pixel_weights_bar is accumulated in wacc like vacc.
template <bool ROBUST, bool RECORD, bool WEIGHTED = false>
GS_DEV void pb_point(const PbBatch& pb, const PbRecord* rec, const int it, const int first, const int last,
                     const float delta_launch, const bool taped) {
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  __shared__ double ux[12];   // u(6), xi(6)
  __shared__ int active;
  const int seq = blockIdx.x % pb.g.B;
  const PbSeq& q = pb.s[seq];
  // (what this stage needs besides the camera and the pose, in front of the prologue's barrier)
  if (threadIdx.x == 0) active = q.state->active;
  if (threadIdx.x >= 2 * GS_WAVE && threadIdx.x < 2 * GS_WAVE + 12) {
    const int i = threadIdx.x - 2 * GS_WAVE;
    ux[i] = i < 6 ? q.state->u[i] : q.state->xi[i - 6];
  }
  const PiSlot t = pi_prologue(q.in, pb.g, q.tape[it].T, cam, Ts);
  const float delta = (ROBUST && taped) ? q.tape[it].pad[0] : delta_launch;
  const int64_t p = t.p;
  const int k = t.k;
  bool used = false;
  int32_t key = PB_NO_KEY;   // (RECORD)
  double sb[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
  double wbar = 0.0;   // (WEIGHTED) this iteration's contribution to the slot's pixel_weights_bar
  static_assert(ROBUST || !WEIGHTED, "the weighted instance differentiates its weight next to the Huber weight");
  if (t.in_lattice) {
    if (active) {   // (block-uniform; an iteration without inliers has no used slot)
      const int64_t n_map = gs_count(q.in.n);
      int64_t row;
      float sf[3];
      float4 df, mf;
      float wp;
      used = pi_associate<WEIGHTED>(Ts, cam, q.in, pb.g, n_map, p, row, sf, df, mf, wp) == 0;
      if (used) {
        double s[3], a[6];
        const double d[3] = {(double)df.x, (double)df.y, (double)df.z}, m[3] = {(double)mf.x, (double)mf.y, (double)mf.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (double)q.in.vertex[3 * p + c];
#pragma unroll
        for (int c = 0; c < 3; ++c)
          s[c] = (double)Ts[4 * c] * v[0] + (double)Ts[4 * c + 1] * v[1] + (double)Ts[4 * c + 2] * v[2] + (double)Ts[4 * c + 3];
        a[0] = m[0]; a[1] = m[1]; a[2] = m[2];
        a[3] = s[1] * m[2] - s[2] * m[1];
        a[4] = s[2] * m[0] - s[0] * m[2];
        a[5] = s[0] * m[1] - s[1] * m[0];
        const double r[3] = {d[0] - s[0], d[1] - s[1], d[2] - s[2]};
        const double b = m[0] * r[0] + m[1] * r[1] + m[2] * r[2];
        double cc = 0.0, e = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          cc += ux[6 + c] * a[c];
          e += ux[c] * a[c];
        }
        double ab[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) ab[c] = (b - cc) * ux[c] - e * ux[6 + c];
        if (ROBUST) {   // (e becomes the residual's adjoint bb)
          float af[6], bf;
          gn_row_pn(sf[0], sf[1], sf[2], df, mf, af, bf);
          const bool clipped = pi_huber_clipped(bf, delta);
          const double hw = pi_huber_weight(clipped, b, (double)delta);
          const double hd = clipped ? -hw / b : 0.0;
          if (WEIGHTED) {
            wbar = hw * e * (b - cc);
            const double wt = (double)wp * hw;
#pragma unroll
            for (int c = 0; c < 6; ++c) ab[c] = wt * ab[c];
            e = e * ((double)wp * (hw + hd * (b - cc)));
          } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) ab[c] = hw * ab[c];
            e = e * (hw + hd * (b - cc));
          }
        }
        const double* w = ab + 3;
        sb[0] = (m[1] * w[2] - m[2] * w[1]) - e * m[0];
        sb[1] = (m[2] * w[0] - m[0] * w[2]) - e * m[1];
        sb[2] = (m[0] * w[1] - m[1] * w[0]) - e * m[2];
        double* cr = nullptr;
        if constexpr (RECORD) {
          if (q.pbar || q.mbar) {
            cr = rec->contrib[seq] + 6 * (int64_t)k;
            key = (int32_t)row;   // (row < n_bound < PB_NO_KEY: the entry checks it)
          }
        }
        if (q.pbar) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double x = e * m[c];
            if constexpr (RECORD) cr[c] = x;
            else atomicAdd(&q.pbar[3 * row + c], x);
          }
        } else if (RECORD && cr) {
#pragma unroll
          for (int c = 0; c < 3; ++c) cr[c] = 0.0;
        }
        if (q.mbar) {
          const double wxs[3] = {w[1] * s[2] - w[2] * s[1], w[2] * s[0] - w[0] * s[2], w[0] * s[1] - w[1] * s[0]};
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double x = ab[c] + wxs[c] + e * r[c];
            if constexpr (RECORD) cr[3 + c] = x;
            else atomicAdd(&q.mbar[3 * row + c], x);
          }
        } else if (RECORD && cr) {
#pragma unroll
          for (int c = 0; c < 3; ++c) cr[3 + c] = 0.0;
        }
      }
    }
    if constexpr (RECORD) {   // every slot of the lattice, whatever the iteration: nothing of the launch before stays
      rec->key[seq][k] = key;
      rec->sort_key[(int64_t)seq * pb.g.nslots + k] = ((uint64_t)seq << 32) | (uint32_t)key;
    }
    if (q.vacc) {   // a slot is its own pixel and the iterations are serialised: no atomics
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double acc = first ? 0.0 : q.vacc[3 * (int64_t)k + c];
        if (used) acc += (double)Ts[c] * sb[0] + (double)Ts[4 + c] * sb[1] + (double)Ts[8 + c] * sb[2];
        if (last) q.vertex_bar[3 * p + c] = (float)acc;
        else q.vacc[3 * (int64_t)k + c] = acc;
      }
    }
    if (WEIGHTED && q.wacc) {   // as vacc: the slot's own thread, float64 across the serialised iterations
      double acc = first ? 0.0 : q.wacc[k];
      if (used) acc += wbar;
      if (last) q.weights_bar[p] = (float)acc;
      else q.wacc[k] = acc;
    }
  }
  // the 12 sums of sb [v^T 1] in the forward's reduction shape: terms 0 .. 8 the outer product, 9 .. 11 sb
  pi_chunk_reduce<PB_NV>([&](const int i) { return i < 9 ? sb[i / 3] * v[i % 3] : sb[i - 9]; }, __ballot(used) != 0ull,
                         q.partials + (int64_t)t.chunk * PB_NV);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_bwd_point_kernel(const PbBatch pb, const int it, const int first,
                                                                        const int last) {
  pb_point<false, false>(pb, nullptr, it, first, last, 0.0f, false);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_robust_picp_bwd_point_kernel(const PbBatch pb, const int it,
                                                                               const int first, const int last,
                                                                               const float delta, const int taped) {
  pb_point<true, false>(pb, nullptr, it, first, last, delta, taped != 0);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_weighted_picp_bwd_point_kernel(const PbBatch pb, const int it,
                                                                                 const int first, const int last,
                                                                                 const float delta, const int taped) {
  pb_point<true, false, true>(pb, nullptr, it, first, last, delta, taped != 0);
}

// ------------------------------------------------------------------ ordered mode: the RECORD point stages, the settle step
__global__ void __launch_bounds__(GS_PI_CHUNK) gs_ordered_picp_bwd_point_kernel(const PbBatch pb, const PbRecord rec,
                                                                                const int it, const int first,
                                                                                const int last) {
  pb_point<false, true>(pb, &rec, it, first, last, 0.0f, false);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_ordered_robust_picp_bwd_point_kernel(const PbBatch pb, const PbRecord rec,
                                                                                       const int it, const int first,
                                                                                       const int last, const float delta,
                                                                                       const int taped) {
  pb_point<true, true>(pb, &rec, it, first, last, delta, taped != 0);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_ordered_weighted_picp_bwd_point_kernel(const PbBatch pb, const PbRecord rec,
                                                                                         const int it, const int first,
                                                                                         const int last, const float delta,
                                                                                         const int taped) {
  pb_point<true, true, true>(pb, &rec, it, first, last, delta, taped != 0);
}

// the values of the sort: 0, 1, 2, ... (pair b nslots + k is slot k of sequence b); written once per launch group
__global__ void __launch_bounds__(256) gs_ordered_picp_bwd_iota_kernel(uint32_t* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

// The pairs of a point stage sorted by (sequence, row), equal keys in ascending slot order (the sort is stable and its
// input is in slot order).  The thread at the head of a run adds the run's contributions, one after the other from 0.0,
// and then adds the sum to the row's accumulators: a fixed order, and no other thread of any launch touches the row
// meanwhile (the launches of the backward are ordered).  The shape of bw_segment_add_kernel (gs_icp_bwd.hip).
__global__ void __launch_bounds__(256) gs_ordered_picp_bwd_settle_kernel(const PbSettle z, const uint64_t* __restrict__ key,
                                                                         const uint32_t* __restrict__ src, int64_t n) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint64_t j = key[p];
  const int64_t row = (int64_t)(uint32_t)j;
  if (row == PB_NO_KEY || (p > 0 && key[p - 1] == j)) return;   // a slot without a row, or not the head of its run
  const int b = (int)(j >> 32);
  const double* contrib = z.contrib[b];
  const int64_t slot0 = (int64_t)b * z.nslots;   // (the sequence's first pair)
  double t[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
  for (int64_t q = p; q < n && key[q] == j; ++q) {
    const double* c = contrib + 6 * ((int64_t)src[q] - slot0);
    for (int a = 0; a < 3; ++a) { t[a] += c[a]; m[a] += c[3 + a]; }
  }
  if (z.pbar[b])
    for (int a = 0; a < 3; ++a) z.pbar[b][3 * row + a] = z.pbar[b][3 * row + a] + t[a];
  if (z.mbar[b])
    for (int a = 0; a < 3; ++a) z.mbar[b][3 * row + a] = z.mbar[b][3 * row + a] + m[a];
}

__global__ void __launch_bounds__(256) gs_picp_bwd_cast_kernel(const double* __restrict__ in, int64_t n,
                                                               float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

// scratch of one sequence: state | partials (nchunks, 12) | vacc (nslots, 3) | pbar (n_map, 3) | mbar (n_map, 3)
static size_t pb_partials_bytes(int64_t nchunks) { return gs_align((size_t)nchunks * PB_NV * sizeof(double)); }
static size_t pb_rows_bytes(int64_t rows) { return gs_align((size_t)(rows > 0 ? rows : 0) * 3 * sizeof(double)); }

extern "C" int64_t gs_projective_icp_backward_scratch_bytes(int H, int W, int stride, int64_t n_map) {
  if (H <= 0 || W <= 0 || stride <= 0 || n_map < 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  const int64_t nslots = picp_slots(H, W, stride), nchunks = gs_ceil_div(nslots, GS_PI_CHUNK);
  return (int64_t)(gs_align(sizeof(PbState)) + pb_partials_bytes(nchunks) + pb_rows_bytes(nslots) +
                   2 * pb_rows_bytes(n_map));
}

// ordered mode: the record of a sequence lies behind its atomic-mode scratch, contrib (nslots, 6) | key (nslots); the
// sort buffers of a launch group of g sequences, n = g nslots pairs, are one scratch of the call that its groups take
// in turn: sort_key (n) | sorted keys (n) | values (n) | sorted values (n) | hipcub's temporary storage
static size_t pb_contrib_bytes(int64_t nslots) { return gs_align((size_t)nslots * 6 * sizeof(double)); }
static size_t pb_key_bytes(int64_t nslots) { return gs_align((size_t)nslots * sizeof(int32_t)); }
static size_t pb_sort_temp_bytes(int64_t n) { return gs_align(64 * (size_t)n + (1u << 20)); }
static int64_t pb_group(int B) { return B < GS_MAX_BATCH ? B : GS_MAX_BATCH; }

extern "C" int64_t gs_projective_icp_ordered_backward_scratch_bytes(int H, int W, int stride, int64_t n_map) {
  const int64_t base = gs_projective_icp_backward_scratch_bytes(H, W, stride, n_map);
  if (base == 0) return 0;
  const int64_t nslots = picp_slots(H, W, stride);
  return base + (int64_t)(pb_contrib_bytes(nslots) + pb_key_bytes(nslots));
}

extern "C" int64_t gs_projective_icp_ordered_backward_sort_scratch_bytes(int B, int H, int W, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || stride <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  const int64_t n = pb_group(B) * picp_slots(H, W, stride);
  if (n >= (1ll << 31)) return 0;   // (hipcub counts the pairs in an int)
  return (int64_t)(2 * gs_align((size_t)n * sizeof(uint64_t)) + 2 * gs_align((size_t)n * sizeof(uint32_t)) +
                   pb_sort_temp_bytes(n));
}

// what the ordered entry adds to a call of pb_backward
struct PbOrderedCall {
  const gs_picp_ordered_backward_seq* seqs;
  void* sort_scratch;
  int64_t sort_scratch_bytes;
};
// what the weighted entry adds: per sequence the forward's pixel weights (a NULL entry: none) and the output (H, W) (a
// NULL entry, or a NULL array: not asked for).  The float64 accumulator of the output (nslots) lies behind the
// sequence's scratch of the mode.
struct PbWeightedCall {
  const float* const* weights;
  float* const* weights_bar;
};
static size_t pb_wacc_bytes(int64_t nslots) { return gs_align((size_t)nslots * sizeof(double)); }

extern "C" int64_t gs_projective_icp_weighted_backward_scratch_bytes(int H, int W, int stride, int64_t n_map, int ordered) {
  const int64_t base = ordered ? gs_projective_icp_ordered_backward_scratch_bytes(H, W, stride, n_map)
                               : gs_projective_icp_backward_scratch_bytes(H, W, stride, n_map);
  return base > 0 ? base + (int64_t)pb_wacc_bytes(picp_slots(H, W, stride)) : 0;
}

// the pass behind the entries; delta: the Huber threshold the forward ran with (0: the plain point kernel); taped: the
// robust point kernel with every iteration's threshold from the tape (delta is then not read); oc: the ordered entry's
// sequences and sort scratch (seqs_host is then NULL), or NULL: the atomic mode
// wc: the weighted entry's weights and output (the WEIGHTED point kernels run), or NULL
static int pb_backward(const char* who, const gs_picp_backward_seq* seqs_host, int B, int H, int W,
                       const gs_picp_params* params_host, float delta, bool taped, const PbOrderedCall* oc,
                       void* stream, const PbWeightedCall* wc = nullptr) {
  PICP_REQUIRE(who, (oc ? oc->seqs != nullptr : seqs_host != nullptr) && params_host && B > 0 && H > 0 && W > 0,
               "bad arguments");
  PICP_REQUIRE(who, (int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  const gs_picp_params& prm = *params_host;
  PICP_CHECK_PARAMS(who, prm);
  PICP_CHECK_DELTA(who, delta, "huber_delta");
  const int64_t nslots = picp_slots(H, W, prm.stride), nchunks = gs_ceil_div(nslots, GS_PI_CHUNK);
  const auto seq = [&](int b) -> const gs_picp_backward_seq& { return oc ? oc->seqs[b].base : seqs_host[b]; };
  PICP_REQUIRE(who, !wc || wc->weights, "NULL pointer (weights)");
  // (the scratch of sequence b in front of the weighted entry's accumulator, for the map size it is checked for)
  const auto mode_bytes = [&](int64_t n_map) {
    return oc ? gs_projective_icp_ordered_backward_scratch_bytes(H, W, prm.stride, n_map)
              : gs_projective_icp_backward_scratch_bytes(H, W, prm.stride, n_map);
  };
  // (the accumulator is asked of a sequence only when its output is asked for)
  const auto wacc_bytes = [&](int b) {
    return wc && wc->weights_bar && wc->weights_bar[b] ? (int64_t)pb_wacc_bytes(nslots) : (int64_t)0;
  };
  bool any_map = false;
  for (int b = 0; b < B; ++b) {
    const gs_picp_backward_seq& u = seq(b);
    PICP_REQUIRE(who, u.vertex && u.normal && u.depth && u.K16 && u.index && u.model_pose16 && u.tape && u.pose_bar16 &&
                   u.scratch,
               "NULL pointer");
    PICP_REQUIRE(who, ((uintptr_t)u.tape & 7) == 0 && ((uintptr_t)u.scratch & 7) == 0, "misaligned tape or scratch");
    PICP_REQUIRE(who, u.map.n_bound >= 0, "bad map size");
    PICP_REQUIRE(who, u.map.n_bound == 0 || (u.map.points && u.map.normals), "NULL pointer (map points / normals)");
    const bool want_map = u.points_bar || u.normals_bar;
    any_map = any_map || (want_map && u.map.n_bound > 0);
    if (oc) {
      PICP_REQUIRE(who, u.map.n_bound < PB_NO_KEY, "map too large for int32 row keys (n_bound >= 0x7fffffff)");
    }
    PICP_REQUIRE(who, u.scratch_bytes >= mode_bytes(want_map ? u.map.n_bound : 0) + wacc_bytes(b), "scratch too small");
  }
  if (oc && any_map) {
    PICP_REQUIRE(who, pb_group(B) * nslots < (1ll << 31), "too many slots in a launch group for one sort (sequences x nslots >= 2^31)");
    PICP_REQUIRE(who, oc->sort_scratch && ((uintptr_t)oc->sort_scratch & 7) == 0, "NULL or misaligned sort scratch");
    PICP_REQUIRE(who, oc->sort_scratch_bytes >= gs_projective_icp_ordered_backward_sort_scratch_bytes(B, H, W, prm.stride),
                 "sort scratch too small");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    PbBatch pb;
    picp_fill(pb.g, nb, H, W, prm.stride, prm.dist_th, prm.dot_th, prm.damp);
    PbRecord rec{};
    PbSettle sz{};
    bool ordered = false;   // the group records and sorts: the ordered entry, and a map output asked for in the group
    for (int b = 0; b < nb; ++b) {
      const gs_picp_backward_seq& u = seq(c0 + b);
      PbSeq& s = pb.s[b];
      picp_fill_inputs(s.in, u);
      s.tape = static_cast<const PiTapeRow*>(u.tape);
      s.pose_bar16 = u.pose_bar16; s.vertex_bar = u.vertex_bar; s.init_pose_bar16 = u.init_pose_bar16;
      char* p = static_cast<char*>(u.scratch);
      s.state = reinterpret_cast<PbState*>(p); p += gs_align(sizeof(PbState));
      s.partials = reinterpret_cast<double*>(p); p += pb_partials_bytes(nchunks);
      s.vacc = u.vertex_bar ? reinterpret_cast<double*>(p) : nullptr; p += pb_rows_bytes(nslots);
      const size_t map_bytes = (size_t)u.map.n_bound * 3 * sizeof(double);
      s.pbar = (u.points_bar && u.map.n_bound > 0) ? reinterpret_cast<double*>(p) : nullptr;
      s.mbar = (u.normals_bar && u.map.n_bound > 0) ? reinterpret_cast<double*>(p + pb_rows_bytes(u.map.n_bound)) : nullptr;
      if (s.pbar) GS_HIP(hipMemsetAsync(s.pbar, 0, map_bytes, st));
      if (s.mbar) GS_HIP(hipMemsetAsync(s.mbar, 0, map_bytes, st));
      // pixels off the lattice get no gradient (the last point stage stores the lattice pixels)
      if (u.vertex_bar && prm.stride > 1) GS_HIP(hipMemsetAsync(u.vertex_bar, 0, (size_t)H * W * 3 * sizeof(float), st));
      s.weights_bar = nullptr; s.wacc = nullptr;
      if (wc) {
        s.in.weight = wc->weights[c0 + b];
        s.weights_bar = wc->weights_bar ? wc->weights_bar[c0 + b] : nullptr;
        if (s.weights_bar) {
          s.wacc = reinterpret_cast<double*>(static_cast<char*>(u.scratch) +
                                             mode_bytes((u.points_bar || u.normals_bar) ? u.map.n_bound : 0));
          if (prm.stride > 1) GS_HIP(hipMemsetAsync(s.weights_bar, 0, (size_t)H * W * sizeof(float), st));
        }
      }
      if (oc) {   // the sequence's record, behind the atomic mode's layout for the map size its scratch was checked for
        char* r = static_cast<char*>(u.scratch) +
                  gs_projective_icp_backward_scratch_bytes(H, W, prm.stride, (u.points_bar || u.normals_bar) ? u.map.n_bound : 0);
        rec.contrib[b] = reinterpret_cast<double*>(r);
        rec.key[b] = reinterpret_cast<int32_t*>(r + pb_contrib_bytes(nslots));
        sz.contrib[b] = rec.contrib[b]; sz.pbar[b] = s.pbar; sz.mbar[b] = s.mbar;
        ordered = ordered || s.pbar || s.mbar;
      }
    }
    const unsigned blocks = (unsigned)nb * (unsigned)nchunks;
    const int64_t npairs = (int64_t)nb * nslots;   // (ordered: < 2^31, checked above)
    const unsigned pair_blocks = (unsigned)gs_ceil_div(npairs, 256);
    uint64_t* keys_sorted = nullptr;
    uint32_t *vals = nullptr, *vals_sorted = nullptr;
    void* sort_temp = nullptr;
    size_t sort_temp_bytes = 0;
    if (ordered) {
      char* p = static_cast<char*>(oc->sort_scratch);
      rec.sort_key = reinterpret_cast<uint64_t*>(p); p += gs_align((size_t)npairs * sizeof(uint64_t));
      keys_sorted = reinterpret_cast<uint64_t*>(p); p += gs_align((size_t)npairs * sizeof(uint64_t));
      vals = reinterpret_cast<uint32_t*>(p); p += gs_align((size_t)npairs * sizeof(uint32_t));
      vals_sorted = reinterpret_cast<uint32_t*>(p); p += gs_align((size_t)npairs * sizeof(uint32_t));
      sort_temp = p;
      sort_temp_bytes = pb_sort_temp_bytes(npairs);
      sz.nslots = nslots;
      size_t need = 0;   // (35 key bits: 3 of the sequence above the 32 of the row or PB_NO_KEY)
      GS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, rec.sort_key, keys_sorted, vals, vals_sorted, (int)npairs, 0, 35, st));
      if (need > sort_temp_bytes) {
        gs_set_error("%s: %s", who, "sort scratch too small for hipcub's temporary storage");
        return GS_ERR_INVALID;
      }
      hipLaunchKernelGGL(gs_ordered_picp_bwd_iota_kernel, dim3(pair_blocks), dim3(256), 0, st, vals, npairs);
    }
    for (int it = prm.numiters - 1; it >= 0; --it) {
      const int first = it == prm.numiters - 1, last = it == 0 ? 1 : 0;
      hipLaunchKernelGGL(gs_picp_bwd_scalar_kernel, dim3(nb), dim3(GS_PI_FIN), 0, st, pb, it, first ? 0 : 1);
      const bool robust = delta > 0.0f || taped;
      if (!ordered) {
        if (wc)
          hipLaunchKernelGGL(gs_weighted_picp_bwd_point_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, it, first, last,
                             delta, taped ? 1 : 0);
        else if (robust)
          hipLaunchKernelGGL(gs_robust_picp_bwd_point_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, it, first, last,
                             delta, taped ? 1 : 0);
        else
          hipLaunchKernelGGL(gs_picp_bwd_point_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, it, first, last);
        continue;
      }
      if (wc)
        hipLaunchKernelGGL(gs_ordered_weighted_picp_bwd_point_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, rec, it,
                           first, last, delta, taped ? 1 : 0);
      else if (robust)
        hipLaunchKernelGGL(gs_ordered_robust_picp_bwd_point_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, rec, it, first,
                           last, delta, taped ? 1 : 0);
      else
        hipLaunchKernelGGL(gs_ordered_picp_bwd_point_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, rec, it, first, last);
      for (int b = 0; b < nb; ++b) {   // the record as it stands, for the caller that asked (the tests)
        const gs_picp_ordered_backward_seq& o = oc->seqs[c0 + b];
        if (o.key_out)
          GS_HIP(hipMemcpyAsync(o.key_out + (int64_t)it * nslots, rec.key[b], (size_t)nslots * sizeof(int32_t),
                                hipMemcpyDeviceToDevice, st));
        if (o.contrib_out && (pb.s[b].pbar || pb.s[b].mbar))
          GS_HIP(hipMemcpyAsync(o.contrib_out + (int64_t)it * nslots * 6, rec.contrib[b], (size_t)nslots * 6 * sizeof(double),
                                hipMemcpyDeviceToDevice, st));
      }
      // the settle step: ONE sort for the group, then one thread per run
      size_t tb = sort_temp_bytes;
      GS_HIP(hipcub::DeviceRadixSort::SortPairs(sort_temp, tb, rec.sort_key, keys_sorted, vals, vals_sorted, (int)npairs, 0, 35, st));
      hipLaunchKernelGGL(gs_ordered_picp_bwd_settle_kernel, dim3(pair_blocks), dim3(256), 0, st, sz, keys_sorted, vals_sorted,
                         npairs);
    }
    hipLaunchKernelGGL(gs_picp_bwd_scalar_kernel, dim3(nb), dim3(GS_PI_FIN), 0, st, pb, -1, 1);
    for (int b = 0; b < nb; ++b) {
      const gs_picp_backward_seq& u = seq(c0 + b);
      const int64_t n3 = 3 * u.map.n_bound;
      if (pb.s[b].pbar)
        hipLaunchKernelGGL(gs_picp_bwd_cast_kernel, dim3((unsigned)gs_ceil_div(n3, 256)), dim3(256), 0, st, pb.s[b].pbar, n3,
                           u.points_bar);
      if (pb.s[b].mbar)
        hipLaunchKernelGGL(gs_picp_bwd_cast_kernel, dim3((unsigned)gs_ceil_div(n3, 256)), dim3(256), 0, st, pb.s[b].mbar, n3,
                           u.normals_bar);
    }
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}

extern "C" int gs_projective_icp_backward_batch_f32(const gs_picp_backward_seq* seqs_host, int B, int H, int W,
                                                    const gs_picp_params* params_host, void* stream) {
  return pb_backward(__func__, seqs_host, B, H, W, params_host, 0.0f, false, nullptr, stream);
}

extern "C" int gs_projective_icp_robust_backward_batch_f32(const gs_picp_backward_seq* seqs_host, int B, int H, int W,
                                                           const gs_picp_params* params_host, float huber_delta,
                                                           void* stream) {
  return pb_backward(__func__, seqs_host, B, H, W, params_host, huber_delta, false, nullptr, stream);
}

extern "C" int gs_projective_icp_scaled_backward_batch_f32(const gs_picp_backward_seq* seqs_host, int B, int H, int W,
                                                           const gs_picp_params* params_host, void* stream) {
  return pb_backward(__func__, seqs_host, B, H, W, params_host, 0.0f, true, nullptr, stream);
}

// the ordered mode of the three entries above in one: huber_delta as the robust entry's (0: the plain tape),
// taped_scale != 0 as the scaled entry's (huber_delta is then not read)
extern "C" int gs_projective_icp_ordered_backward_batch_f32(const gs_picp_ordered_backward_seq* seqs_host, int B, int H,
                                                            int W, const gs_picp_params* params_host, float huber_delta,
                                                            int taped_scale, void* sort_scratch,
                                                            int64_t sort_scratch_bytes, void* stream) {
  const PbOrderedCall oc{seqs_host, sort_scratch, sort_scratch_bytes};
  return pb_backward(__func__, nullptr, B, H, W, params_host, taped_scale ? 0.0f : huber_delta, taped_scale != 0, &oc,
                     stream);
}

// the backward of the weighted forward (gs_projective_icp_weighted_batch_f32 with a tape): the three tapes as in the
// ordered entry (huber_delta, taped_scale), atomic (ordered == 0: key_out / contrib_out and the sort scratch are not
// read) or ordered; weights_host as at the forward; weights_bar_host: per sequence the output (H, W) or NULL, or NULL
// for none at all.  scratch per sequence: gs_projective_icp_weighted_backward_scratch_bytes when its output is asked
// for, else the scratch of the mode's unweighted entry.
extern "C" int gs_projective_icp_weighted_backward_batch_f32(const gs_picp_ordered_backward_seq* seqs_host,
                                                             const float* const* weights_host,
                                                             float* const* weights_bar_host, int B, int H, int W,
                                                             const gs_picp_params* params_host, float huber_delta,
                                                             int taped_scale, int ordered, void* sort_scratch,
                                                             int64_t sort_scratch_bytes, void* stream) {
  GS_REQUIRE(seqs_host && B > 0, "bad arguments");
  const PbWeightedCall wc{weights_host, weights_bar_host};
  const float delta = taped_scale ? 0.0f : huber_delta;
  if (ordered) {
    const PbOrderedCall oc{seqs_host, sort_scratch, sort_scratch_bytes};
    return pb_backward(__func__, nullptr, B, H, W, params_host, delta, taped_scale != 0, &oc, stream, &wc);
  }
  std::vector<gs_picp_backward_seq> base(B);
  for (int b = 0; b < B; ++b) base[b] = seqs_host[b].base;
  return pb_backward(__func__, base.data(), B, H, W, params_host, delta, taped_scale != 0, nullptr, stream, &wc);
}
