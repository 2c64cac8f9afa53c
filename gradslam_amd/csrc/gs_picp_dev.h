// gs_picp_dev.h — what the projective ICP (gs_picp.hip), its colour form (gs_picp_color.hip) and its backward pass
// (gs_picp_bwd.hip) share: the lattice geometry, the slot's association at a pose (ONE definition: the backward uses the
// forward's association exactly, at the taped float32 pose), the fixed-shape wave reduction, the Huber weight of the
// robust entries (ONE definition as well), the layout of the forward tape, and -- for the two forward files -- the descriptors of a launch, the body of the finish kernel and the checks of
// the entry points.
#pragma once
#include "gs_assoc_dev.h"
#include "gs_icp_math.h"

constexpr int GS_PI_CHUNK = 256;
constexpr int GS_PI_TRACE = 8;   // floats per trace row: count, (float)S[27], xi(6)
constexpr int GS_PIC_TRACE = 9;  // the colour solve's row: the 8 above (S[27] the joint sum of squares) + the colour rows

// One iteration of the taped forward (gs_projective_icp_tape_batch_f32), written by the finish kernel: the pose the
// iteration linearised at, its 28 sums, the step it took (0 without inliers) and its inlier count.  A tape is numiters
// such rows.
struct PiTapeRow {
  double S[LIN_NV];
  float T[16];
  float xi[6];
  float pad[2];
  int64_t count;
};
static_assert(sizeof(PiTapeRow) == 328, "the tape row is part of the ABI (gs_projective_icp_tape_bytes)");

static inline int64_t picp_slots(int H, int W, int stride) {
  return gs_ceil_div(H, stride) * gs_ceil_div(W, stride);
}

// levels 1..6 of the tree: lane l adds the value of lane l ^ d, d = 1, 2, ..., 32 (every lane ends with the wave's sum)
GS_DEV double pi_wave_tree(double x, const bool any) {
  if (any) {
#pragma unroll
    for (int d = 1; d < GS_WAVE; d <<= 1) x = x + __shfl_xor(x, d, GS_WAVE);
  }
  return x;
}

// ------------------------------------------------------------------ robust (Huber) weights
// ONE definition for the forward kernels (float) and the backward pass (double): a residual r beyond the threshold is
// clipped, its row enters the normal equations with weight delta / |r|, every other row with 1.  delta == 0 switches the
// weight off; a NaN residual is not clipped.  The flag is always taken from the float32 residual of the forward.
GS_DEV bool pi_huber_clipped(const float r, const float delta) { return delta > 0.0f && fabsf(r) > delta; }
template <typename T>
GS_DEV T pi_huber_weight(const bool clipped, const T r, const T delta) {
  return clipped ? delta / (r < T(0) ? -r : r) : T(1);
}
// a term of the normal equations: the exact product of two float32 factors, weighted (one rounding)
GS_DEV double pi_term(const float w, const float x, const float y) { return (double)w * ((double)x * (double)y); }

// The association of lattice pixel p at pose Ts (12 floats): the slot's code (0 used, 1 .. 5 the reject codes of the
// header), the index image's entry where one was read (else -1), the live vertex under Ts and, for a row that was read
// (codes 0, 4, 5), the map point d and normal m.  n_map = min(device count, bound): a stale index is never dereferenced.
GS_DEV int pi_associate(const float* Ts, const GsCamera& cam, const float* __restrict__ vertex,
                        const float* __restrict__ normal, const float* __restrict__ depth,
                        const int64_t* __restrict__ index, const float* __restrict__ points,
                        const float* __restrict__ normals, const int64_t n_map, const int64_t p, const int H, const int W,
                        const float u_hi, const float v_hi, const float dist_th, const float dot_th, int64_t& row,
                        float* s, float4& d, float4& m) {
  row = -1;
  if (!(depth[p] > 0.0f)) return 1;
  float g[3];
  gs_rigid_fma(Ts, vertex[3 * p], vertex[3 * p + 1], vertex[3 * p + 2], s[0], s[1], s[2]);
  const float n0 = normal[3 * p], n1 = normal[3 * p + 1], n2 = normal[3 * p + 2];
  g[0] = gs_dot3_fma(Ts[0], Ts[1], Ts[2], n0, n1, n2);
  g[1] = gs_dot3_fma(Ts[4], Ts[5], Ts[6], n0, n1, n2);
  g[2] = gs_dot3_fma(Ts[8], Ts[9], Ts[10], n0, n1, n2);
  int h2, w2;
  if (!gs_project_point_hw(cam, s[0], s[1], s[2], H, W, u_hi, v_hi, h2, w2)) return 2;
  row = index[(int64_t)h2 * W + w2];
  if (!(row >= 0 && row < n_map)) return 3;
  // the two tests of gs_is_similar_v, apart: which one fails is the slot's code
  d = make_float4(points[3 * row], points[3 * row + 1], points[3 * row + 2], 0.0f);
  m = make_float4(normals[3 * row], normals[3 * row + 1], normals[3 * row + 2], 0.0f);
  const float dist = gs_norm3(s[0] - d.x, s[1] - d.y, s[2] - d.z);
  const float dot = gs_dot3_plain(g[0], g[1], g[2], m.x, m.y, m.z);
  return !(dist < dist_th) ? 4 : (!(dot > dot_th) ? 5 : 0);
}

// ------------------------------------------------------------------ the descriptors of a forward launch
struct PiSeq {
  const float* vertex;
  const float* normal;
  const float* depth;
  const float* K16;
  const int64_t* index;
  const float* model_pose16;
  const float* points;
  const float* normals;
  GsCount n;
  const float* T_in;       // pose estimate the launch reads (iteration 0: the caller's initial pose; then T_out)
  float* T_out;            // finish: the updated estimate (NULL: sums only)
  float* trace_row;        // finish: this iteration's trace row, or NULL
  PiTapeRow* tape_row;     // finish: this iteration's tape row, or NULL
  double* partials;        // (nchunks, 28)
  int32_t* counts;         // (nchunks)
  int32_t* code_out;       // table-level outputs, any may be NULL: (nslots)
  int64_t* row_out;        // (nslots)
  float* a_out;            // (nslots, 6)
  float* b_out;            // (nslots)
  double* sums_out;        // finish: (28), or NULL
  int64_t* count_out;      // finish: (1), or NULL
};
struct PiGeom {
  int B, H, W, stride, Wl, nslots, nchunks;
  float u_hi, v_hi, dist_th, dot_th, damp;
};
struct PiBatch {
  PiSeq s[GS_MAX_BATCH];
  PiGeom g;
};

// ------------------------------------------------------------------ the finish kernel's body
// One block per sequence.  S = the chunk partials in ascending chunk order, starting from the first: a serial chain by
// contract, so what has to be kept off it is the memory latency -- a lane that loaded its partial of chunk c, added it and
// only then asked for chunk c + 1 would pay a trip to memory per chunk (measured: 0.25 us each, 300 us at 1 200 chunks).
// All 256 threads move the table through LDS a tile of 256 chunks at a time (coalesced, 28 loads in flight per thread, the
// next tile on its way while lane i < 28 of wave 0 adds column i of the current one); then wave 0 either hands out the
// sums as they are (the table-level entry) or takes the Gauss-Newton step.
// COLOR: the colour solve's finish also adds up the chunks' colour-row counts (ccounts, an integer sum) and hands the
// total out as the ninth float of the trace row and through ccount_out.
constexpr int GS_PI_FIN = 256;    // threads of the finish block
constexpr int GS_PI_TILE = 256;   // chunks per LDS tile: GS_PI_TILE * 28 doubles = 56 KB

template <bool COLOR>
GS_DEV void pi_finish(const PiSeq& q, const int nchunks, const float damp, const int32_t* __restrict__ ccounts,
                      int64_t* ccount_out) {
  static_assert(GS_PI_TILE * LIN_NV % GS_PI_FIN == 0, "a tile is a whole number of loads per thread");
  constexpr int PER = GS_PI_TILE * LIN_NV / GS_PI_FIN;   // 28
  __shared__ double tile[GS_PI_TILE * LIN_NV];
  __shared__ double S[LIN_NV];
  __shared__ float xi[8];
  __shared__ int64_t cnt[GS_PI_FIN / GS_WAVE];
  __shared__ int64_t ccnt[COLOR ? GS_PI_FIN / GS_WAVE : 1];
  const int tid = threadIdx.x, lane = tid & (GS_WAVE - 1);
  const int64_t total = (int64_t)nchunks * LIN_NV;
  int64_t n = 0;
  for (int c = tid; c < nchunks; c += GS_PI_FIN) n += q.counts[c];
#pragma unroll
  for (int d = 1; d < GS_WAVE; d <<= 1) n += __shfl_xor(n, d, GS_WAVE);
  if (lane == 0) cnt[tid / GS_WAVE] = n;
  int64_t nc = 0;
  if (COLOR) {
    for (int c = tid; c < nchunks; c += GS_PI_FIN) nc += ccounts[c];
#pragma unroll
    for (int d = 1; d < GS_WAVE; d <<= 1) nc += __shfl_xor(nc, d, GS_WAVE);
    if (lane == 0) ccnt[tid / GS_WAVE] = nc;
  }
  double nxt[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int64_t i = tid + GS_PI_FIN * r;
    nxt[r] = i < total ? q.partials[i] : 0.0;
  }
  double s = 0.0;
  for (int base = 0; base < nchunks; base += GS_PI_TILE) {
    __syncthreads();   // (the tile of the round before has been added up)
#pragma unroll
    for (int r = 0; r < PER; ++r) tile[tid + GS_PI_FIN * r] = nxt[r];
    __syncthreads();
    if (base + GS_PI_TILE < nchunks) {
#pragma unroll
      for (int r = 0; r < PER; ++r) {
        const int64_t i = (int64_t)(base + GS_PI_TILE) * LIN_NV + tid + GS_PI_FIN * r;
        nxt[r] = i < total ? q.partials[i] : 0.0;
      }
    }
    if (tid < LIN_NV) {
      const int m = nchunks - base < GS_PI_TILE ? nchunks - base : GS_PI_TILE;
      int c = 0;
      if (base == 0) {   // the sum starts from the first partial, not from 0.0 + it (which would turn a -0.0 into +0.0)
        s = tile[tid];
        c = 1;
      }
#pragma unroll 8
      for (; c < m; ++c) s = s + tile[c * LIN_NV + tid];
    }
  }
  if (tid < LIN_NV) {
    S[tid] = s;
    if (q.sums_out) q.sums_out[tid] = s;
  }
  if (tid < 8) xi[tid] = 0.0f;
  __syncthreads();
  if (tid >= GS_WAVE) return;
  n = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
  if (COLOR) nc = (ccnt[0] + ccnt[1]) + (ccnt[2] + ccnt[3]);
  if (tid == 0 && q.count_out) *q.count_out = n;
  if (COLOR && tid == 0 && ccount_out) *ccount_out = nc;
  if (!q.T_out) return;
  if (n > 0) gs_solve_spd6_wave(S, damp, xi);   // (n is the same in every lane)
  gs_wave_sync_lds();
  if (lane == 0) {
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = q.T_in[i];
    if (q.tape_row) {   // the pose this iteration linearised at (T_out below may be the same buffer)
#pragma unroll
      for (int i = 0; i < 16; ++i) q.tape_row->T[i] = T[i];
    }
    if (n > 0) {   // no inlier: xi = 0 and T keeps its bits (a product with the identity would turn a -0 into +0)
      float Tr[16];
      gs_se3_exp_dev(xi, Tr);
      gs_mm4(Tr, T, T);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) q.T_out[i] = T[i];
    if (q.trace_row) {
      q.trace_row[0] = (float)n;
      q.trace_row[1] = (float)S[27];
#pragma unroll
      for (int i = 0; i < 6; ++i) q.trace_row[2 + i] = xi[i];
      if (COLOR) q.trace_row[8] = (float)nc;
    }
    if (q.tape_row) {
      PiTapeRow& tr = *q.tape_row;
#pragma unroll
      for (int i = 0; i < LIN_NV; ++i) tr.S[i] = S[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) tr.xi[i] = xi[i];
      tr.pad[0] = 0.0f; tr.pad[1] = 0.0f;
      tr.count = n;
    }
  }
}

// ------------------------------------------------------------------ host side: scratch layout, checks, descriptors
static inline size_t picp_partials_bytes(int64_t nchunks) { return gs_align((size_t)nchunks * LIN_NV * sizeof(double)); }
static inline size_t picp_counts_bytes(int64_t nchunks) { return gs_align((size_t)nchunks * sizeof(int32_t)); }

// (the checks of a solve run in a helper shared by several entries: the message names the entry that was called)
#define PICP_REQUIRE(who, cond, msg)           \
  do {                                         \
    if (!(cond)) {                             \
      gs_set_error("%s: %s", who, msg);        \
      return GS_ERR_INVALID;                   \
    }                                          \
  } while (0)
#define PICP_CHECK_SEQ(who, u)                                                                                          \
  do {                                                                                                                  \
    PICP_REQUIRE(who, (u).vertex && (u).normal && (u).depth && (u).K16 && (u).index && (u).model_pose16 &&              \
                          (u).init_pose16 && (u).scratch,                                                               \
                 "NULL pointer");                                                                                       \
    PICP_REQUIRE(who, (u).map.n_bound >= 0, "bad map size");                                                            \
    PICP_REQUIRE(who, (u).map.n_bound == 0 || ((u).map.points && (u).map.normals), "NULL pointer (map points / normals)"); \
  } while (0)
// the parameter checks of a solve (the same for the plain and the colour entry)
#define PICP_CHECK_PARAMS(who, prm)                                                                                     \
  do {                                                                                                                  \
    PICP_REQUIRE(who, (prm).stride >= 1, "stride must be at least 1");                                                  \
    PICP_REQUIRE(who, (prm).numiters >= 1, "numiters must be at least 1");                                              \
    PICP_REQUIRE(who, (prm).damp > 0.0f && (prm).damp < __builtin_inff(), "damp must be positive and finite");          \
    PICP_REQUIRE(who, !((prm).dist_th != (prm).dist_th) && !((prm).dot_th != (prm).dot_th), "a threshold is NaN");      \
  } while (0)
// a Huber threshold of a robust entry (0: off)
#define PICP_CHECK_DELTA(who, d, name) \
  PICP_REQUIRE(who, (d) >= 0.0f && (d) < __builtin_inff(), name " must be finite and not negative")

static inline void picp_fill(PiGeom& g, int H, int W, int stride, float dist_th, float dot_th, float damp) {
  g.H = H; g.W = W; g.stride = stride;
  g.Wl = (int)gs_ceil_div(W, stride);
  g.nslots = (int)picp_slots(H, W, stride);
  g.nchunks = (int)gs_ceil_div(g.nslots, GS_PI_CHUNK);
  g.u_hi = (float)((double)W - 0.999); g.v_hi = (float)((double)H - 0.999);
  g.dist_th = dist_th; g.dot_th = dot_th; g.damp = damp;
}

static inline void picp_fill_seq(PiSeq& s, const gs_picp_seq& u, int nchunks) {
  s.vertex = u.vertex; s.normal = u.normal; s.depth = u.depth; s.K16 = u.K16; s.index = u.index;
  s.model_pose16 = u.model_pose16;
  s.points = u.map.points; s.normals = u.map.normals;
  s.n = GsCount{u.map.n_bound, u.map.n_dev};
  s.partials = static_cast<double*>(u.scratch);
  s.counts = reinterpret_cast<int32_t*>(static_cast<char*>(u.scratch) + picp_partials_bytes(nchunks));
  s.T_in = u.init_pose16; s.T_out = nullptr; s.trace_row = nullptr; s.tape_row = nullptr;
  s.code_out = nullptr; s.row_out = nullptr; s.a_out = nullptr; s.b_out = nullptr;
  s.sums_out = nullptr; s.count_out = nullptr;
}
