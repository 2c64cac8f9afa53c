// gs_picp_dev.h — what the projective ICP (gs_picp.hip), its colour form (gs_picp_color.hip) and its backward pass
// (gs_picp_bwd.hip) share, ONE definition of each: the inputs of a sequence (PiInputs) and the lattice geometry (PiGeom),
// the block prologue of the per-slot kernels (pi_prologue), the slot's association at a pose (pi_associate: the backward
// uses the forward's association exactly, at the taped float32 pose), the fixed-shape chunk reduction (pi_chunk_reduce)
// with the enumeration of the forward's 28 terms (PI_PAIRS), the tiled ascending column sum of the chunk partials
// (pi_column_sums), the Huber weight of the robust entries, the layout of the forward tape, the checks of the entry
// points, and -- for the two forward files -- the descriptors of a launch, the body of the finish kernel and the two host
// drivers (picp_solve, picp_rows) behind the batch and the table-level entries.  The scaled entries (the Huber threshold
// from the residuals' median) add the descriptors and the launcher of gs_picp_scale.hip's two kernels, which the drivers
// enqueue in front of the robust linearisation.
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

// ------------------------------------------------------------------ inputs of a sequence, geometry of a launch
struct PiInputs {
  const float* vertex;
  const float* normal;
  const float* depth;
  const float* K16;
  const int64_t* index;
  const float* model_pose16;
  const float* points;
  const float* normals;
  GsCount n;
  const float* weight;   // per-pixel weights (H, W) of the weighted entries, or NULL: none
};
struct PiGeom {
  int B, H, W, stride, Wl, nslots, nchunks;
  float u_hi, v_hi, dist_th, dot_th, damp;
};

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

// Huber thresholds and weight tables of the robust forward kernels (delta: the point-to-plane residual, metres; cdelta:
// the colour residual r before color_weight is applied, intensity units; 0 = off; the tables (nslots) may be NULL).  The
// plain-geometry kernel ignores the colour half.
struct PiRobust {
  float delta, cdelta;
  float* weight_out;    // w of a used slot, 0 elsewhere
  float* cweight_out;   // wc of a slot with a colour row, 0 elsewhere
};
// the geometric threshold of a sequence in a robust kernel: its own device float where it has one (the median rule of
// gs_picp_scale.hip, written by the select kernel in front of this launch), else the launch's constant
GS_DEV float pi_huber_delta(const float* __restrict__ delta_dev, const PiRobust& rb) {
  return delta_dev ? *delta_dev : rb.delta;
}

// ------------------------------------------------------------------ the block of a per-slot kernel
// what a thread of a per-slot kernel (256 threads = one chunk of lattice slots) knows after the prologue
struct PiSlot {
  int lane, wave, chunk, k;   // k: the slot
  bool in_lattice;            // k < nslots
  int64_t p;                  // the slot's pixel (i stride, j stride), k = i Wl + j; meaningless beyond the lattice
};

// The prologue of a block of a grid of B * nchunks (the caller takes its sequence, blockIdx.x % B): the chunk from
// blockIdx, the camera of the model view (thread 0) and the 12 pose floats (lanes 64 .. 75) into the caller's LDS, ONE
// barrier -- a caller that stages more LDS does so on other lanes before the call -- then the thread's slot.
GS_DEV PiSlot pi_prologue(const PiInputs& in, const PiGeom& g, const float* __restrict__ pose12, GsCamera& cam,
                          float* Ts) {
  if (threadIdx.x == 0) cam = gs_camera(in.model_pose16, in.K16);
  if (threadIdx.x >= GS_WAVE && threadIdx.x < GS_WAVE + 12) Ts[threadIdx.x - GS_WAVE] = pose12[threadIdx.x - GS_WAVE];
  __syncthreads();
  PiSlot t;
  t.lane = threadIdx.x & (GS_WAVE - 1);
  t.wave = threadIdx.x / GS_WAVE;
  t.chunk = blockIdx.x / g.B;
  t.k = t.chunk * GS_PI_CHUNK + (int)threadIdx.x;
  t.in_lattice = t.k < g.nslots;
  const int i = t.k / g.Wl, j = t.k - i * g.Wl;
  t.p = (int64_t)(i * g.stride) * g.W + j * g.stride;
  return t;
}

// The association of lattice pixel p at pose Ts (12 floats): the slot's code (0 used, 1 .. 5 the reject codes of the
// header), the index image's entry where one was read (else -1), the live vertex under Ts and, for a row that was read
// (codes 0, 4, 5), the map point d and normal m.  n_map = min(device count, bound): a stale index is never dereferenced.
// WEIGHTED (the weighted entries; a sequence without weights has in.weight == NULL): behind the depth test the pixel's
// weight wp = in.weight[p] is read, and a weight that is not a positive finite float32 (zero, negative, NaN, +inf) masks
// the slot: code 6.  wp is handed out (1 where none is read).
template <bool WEIGHTED>
GS_DEV int pi_associate(const float* Ts, const GsCamera& cam, const PiInputs& in, const PiGeom& geom, const int64_t n_map,
                        const int64_t p, int64_t& row, float* s, float4& d, float4& m, float& wp) {
  row = -1;
  wp = 1.0f;
  if (!(in.depth[p] > 0.0f)) return 1;
  if (WEIGHTED && in.weight) {
    wp = in.weight[p];
    if (!(wp > 0.0f && wp < __builtin_inff())) return 6;
  }
  float g[3];
  gs_rigid_fma(Ts, in.vertex[3 * p], in.vertex[3 * p + 1], in.vertex[3 * p + 2], s[0], s[1], s[2]);
  const float n0 = in.normal[3 * p], n1 = in.normal[3 * p + 1], n2 = in.normal[3 * p + 2];
  g[0] = gs_dot3_fma(Ts[0], Ts[1], Ts[2], n0, n1, n2);
  g[1] = gs_dot3_fma(Ts[4], Ts[5], Ts[6], n0, n1, n2);
  g[2] = gs_dot3_fma(Ts[8], Ts[9], Ts[10], n0, n1, n2);
  int h2, w2;
  if (!gs_project_point_hw(cam, s[0], s[1], s[2], geom.H, geom.W, geom.u_hi, geom.v_hi, h2, w2)) return 2;
  row = in.index[(int64_t)h2 * geom.W + w2];
  if (!(row >= 0 && row < n_map)) return 3;
  // the two tests of gs_is_similar_v, apart: which one fails is the slot's code
  d = make_float4(in.points[3 * row], in.points[3 * row + 1], in.points[3 * row + 2], 0.0f);
  m = make_float4(in.normals[3 * row], in.normals[3 * row + 1], in.normals[3 * row + 2], 0.0f);
  const float dist = gs_norm3(s[0] - d.x, s[1] - d.y, s[2] - d.z);
  const float dot = gs_dot3_plain(g[0], g[1], g[2], m.x, m.y, m.z);
  return !(dist < geom.dist_th) ? 4 : (!(dot > geom.dot_th) ? 5 : 0);
}

// ------------------------------------------------------------------ the fixed-shape reductions
// levels 1..6 of the tree: lane l adds the value of lane l ^ d, d = 1, 2, ..., 32 (every lane ends with the wave's sum)
GS_DEV double pi_wave_tree(double x, const bool any) {
  if (any) {
#pragma unroll
    for (int d = 1; d < GS_WAVE; d <<= 1) x = x + __shfl_xor(x, d, GS_WAVE);
  }
  return x;
}

// The NV sums of a chunk.  term(t) is this thread's float64 value of term t (+0.0 for a slot that contributes nothing):
// the xor tree in each wave, lane 0 -> LDS, a barrier, (w0 + w1) + (w2 + w3), and thread t stores term t of the chunk's
// partial row.  any: the wave has a contributing slot (a wave without one adds up +0.0 only: its sums are +0.0, no
// shuffle needed).  Integer counts that a caller put into LDS before the call may be read after it.
template <int NV, typename Term>
GS_DEV void pi_chunk_reduce(const Term& term, const bool any, double* __restrict__ partial_row) {
  __shared__ double red[GS_PI_CHUNK / GS_WAVE][NV];
  const int lane = threadIdx.x & (GS_WAVE - 1), wave = threadIdx.x / GS_WAVE;
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    const double x = pi_wave_tree(term(t), any);
    if (lane == 0) red[wave][t] = x;
  }
  __syncthreads();
  if (threadIdx.x < NV)
    partial_row[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// The 28 terms of the forward as index pairs (x, y) into a slot's row z = (a0 .. a5, b): 21 upper-triangular a_x a_y row
// by row, 6 a_x b, b b.  The flavours of the forward differ in what they form of z[x] and z[y], not in this order.
struct PiPairs {
  int x[LIN_NV], y[LIN_NV];
};
constexpr PiPairs pi_pairs() {
  PiPairs p{};
  int t = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c, ++t) { p.x[t] = r; p.y[t] = c; }
  for (int r = 0; r < 6; ++r, ++t) { p.x[t] = r; p.y[t] = 6; }
  p.x[t] = 6; p.y[t] = 6;
  return p;
}
constexpr PiPairs PI_PAIRS = pi_pairs();

// Column i of a table of chunk partial rows (nchunks, NV), added up in ascending chunk order, for thread i < NV of a
// block of 256 (the other threads get 0.0).  A serial chain by contract, so what has to be kept off it is the memory
// latency -- a lane that loaded its partial of chunk c, added it and only then asked for chunk c + 1 would pay a trip to
// memory per chunk (measured: 0.25 us each, 300 us at 1 200 chunks).  All 256 threads move the table through LDS a tile
// of 256 chunks at a time (coalesced, NV loads in flight per thread, the next tile on its way while lane i < NV of wave 0
// adds column i of the current one).  FROM_FIRST: the chain starts from the first partial, not from 0.0 + it (which
// would turn a -0.0 into +0.0); otherwise it starts from 0.0.  Which of the two a caller takes is part of its bitwise
// contract.
constexpr int GS_PI_FIN = 256;    // threads of the block
constexpr int GS_PI_TILE = 256;   // chunks per LDS tile: GS_PI_TILE * NV doubles (56 KB at 28, 24 KB at 12)

template <int NV, bool FROM_FIRST>
GS_DEV double pi_column_sums(const double* __restrict__ partials, const int nchunks) {
  static_assert(GS_PI_TILE * NV % GS_PI_FIN == 0, "a tile is a whole number of loads per thread");
  constexpr int PER = GS_PI_TILE * NV / GS_PI_FIN;   // NV
  __shared__ double tile[GS_PI_TILE * NV];
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)nchunks * NV;
  double nxt[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int64_t i = tid + GS_PI_FIN * r;
    nxt[r] = i < total ? partials[i] : 0.0;
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
        const int64_t i = (int64_t)(base + GS_PI_TILE) * NV + tid + GS_PI_FIN * r;
        nxt[r] = i < total ? partials[i] : 0.0;
      }
    }
    if (tid < NV) {
      const int m = nchunks - base < GS_PI_TILE ? nchunks - base : GS_PI_TILE;
      int c = 0;
      if (FROM_FIRST && base == 0) {
        s = tile[tid];
        c = 1;
      }
#pragma unroll 8
      for (; c < m; ++c) s = s + tile[c * NV + tid];
    }
  }
  return s;
}

// ------------------------------------------------------------------ the descriptors of a forward launch
struct PiSeq {
  PiInputs in;
  const float* T_in;       // pose estimate the launch reads (iteration 0: the caller's initial pose; then T_out)
  const float* delta_dev;  // the sequence's Huber threshold of this iteration (gs_picp_scale.hip), or NULL: PiRobust::delta
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
struct PiBatch {
  PiSeq s[GS_MAX_BATCH];
  PiGeom g;
};

// the geometric table-level outputs of slot k: its code, its row and z = (a0 .. a5, b)
GS_DEV void pi_table_out(const PiSeq& q, const int k, const int code, const int64_t row, const float* z) {
  if (q.code_out) q.code_out[k] = code;
  if (q.row_out) q.row_out[k] = row;
  if (q.a_out) {
#pragma unroll
    for (int c = 0; c < 6; ++c) q.a_out[6 * (int64_t)k + c] = z[c];
  }
  if (q.b_out) q.b_out[k] = z[6];
}

// ------------------------------------------------------------------ the median rule (gs_picp_scale.hip)
// What the two launches in front of a robust linearisation need of a sequence.  The rule serves two residuals, each
// with its own tables: the point-to-plane residual b over the used slots (PS_GEO) and, in the joint solve, the colour
// residual r before color_weight is applied over the slots with a colour row (PS_COLOR).  For every residual asked for
// they find the lower median of its absolute values at T_in and leave max(c * median, floor) in *delta_dev (and in
// *delta_out when not NULL).
constexpr int PS_GEO = 0, PS_COLOR = 1, PS_RESIDUALS = 2;
struct PiScaleRes {
  uint32_t* keys;      // (nslots): bits(|residual|) of a slot that has the row, 0xFFFFFFFF elsewhere
  uint32_t* hist;      // (GS_PS_BINS): such slots per value of the keys' top 11 bits; zero between the iterations (the
                       // residual pass adds to it, the select block reads it and clears it; a call clears it first)
  float* delta_dev;
  float* delta_out;    // this iteration's entry of the caller's threshold table, or NULL
};
struct PiScaleSeq {
  PiInputs in;
  const float* T_in;
  const float* color;     // the colour inputs of the joint solve (gs_picp_color.hip's PicSeq), read for PS_COLOR only
  const float4* model;
  PiScaleRes r[PS_RESIDUALS];
};
struct PiScaleBatch {
  PiScaleSeq s[GS_MAX_BATCH];
  PiGeom g;
};
// what the launches take by value: the residuals asked for are first .. first + count - 1, each with its constant
// c = (float)huber_k * 1.4826f and its floor
struct PiScalePick {
  float c[PS_RESIDUALS], floor[PS_RESIDUALS];
  int first, count;
};
// the caller's side of the rule: which residuals (on), their constants and floors, and per sequence the device table of
// numiters thresholds (deltas_host, or NULL; the rows entry: delta_out, one float)
struct PiScale {
  bool on[PS_RESIDUALS];
  float c[PS_RESIDUALS], floor[PS_RESIDUALS];
  float* const* deltas_host[PS_RESIDUALS];
  float* delta_out[PS_RESIDUALS];
};
// the residual pass and the select, enqueued back to back (defined in gs_picp_scale.hip); first: the call's first use of
// the descriptors: one more launch in front clears every sequence's counters (after it the select blocks leave them
// cleared)
// weighted: the WEIGHTED instances of the residual pass (a masked slot has no key: it is in no median)
void picp_scale_launch(const PiScaleBatch& sb, const PiScalePick& pk, bool first, bool weighted, hipStream_t st);
// ... and its first half alone, the clear (first) and the residual pass: the key tables and the first digit's counters
// for a caller that selects with a kernel of its own (gs_picp_outliers.hip, through gs_picp_scale_dev.h)
void picp_scale_keys_launch(const PiScaleBatch& sb, const PiScalePick& pk, bool first, bool weighted, hipStream_t st);

constexpr int GS_PS_BINS = 2048;   // values of an 11-bit digit of a key
static inline size_t picp_keys_bytes(int64_t nslots) { return gs_align((size_t)nslots * sizeof(uint32_t)); }
static inline size_t picp_hist_bytes() { return gs_align(GS_PS_BINS * sizeof(uint32_t)); }
// scratch of the rule behind a solve's own scratch of `base` bytes: keys (nslots) | hist (2048) | delta (one float)
static inline size_t picp_scaled_bytes(size_t base, int64_t nslots) {
  return base + picp_keys_bytes(nslots) + picp_hist_bytes() + gs_align(sizeof(float));
}
// ... and with the colour residual's tables behind the geometric ones: the same three again
static inline size_t picp_joint_scaled_bytes(size_t base, int64_t nslots) {
  return picp_scaled_bytes(picp_scaled_bytes(base, nslots), nslots);
}
static inline float picp_scale_c(float huber_k) { return huber_k * 1.4826f; }
static inline PiScale picp_scale_joint(float huber_k, float huber_floor, float color_huber_k, float color_huber_floor,
                                       float* const* deltas_host, float* const* cdeltas_host, float* delta_out,
                                       float* cdelta_out) {
  return PiScale{{huber_k > 0.0f, color_huber_k > 0.0f},
                 {picp_scale_c(huber_k), picp_scale_c(color_huber_k)},
                 {huber_floor, color_huber_floor},
                 {deltas_host, cdeltas_host},
                 {delta_out, cdelta_out}};
}
// the geometric threshold alone (the scaled entries of the plain solve; the joint solve with a constant colour threshold)
static inline PiScale picp_scale_geo(float huber_k, float huber_floor, float* const* deltas_host, float* delta_out) {
  return picp_scale_joint(huber_k, huber_floor, 0.0f, 0.0f, deltas_host, nullptr, delta_out, nullptr);
}
static inline PiScalePick picp_scale_pick(const PiScale& sc) {
  PiScalePick pk;
  for (int i = 0; i < PS_RESIDUALS; ++i) { pk.c[i] = sc.c[i]; pk.floor[i] = sc.floor[i]; }
  pk.first = sc.on[PS_GEO] ? PS_GEO : PS_COLOR;
  pk.count = (sc.on[PS_GEO] ? 1 : 0) + (sc.on[PS_COLOR] ? 1 : 0);
  return pk;
}
#define PICP_CHECK_SCALE(who, k, fl)                                                                    \
  do {                                                                                                  \
    PICP_REQUIRE(who, (k) > 0.0f && (k) < __builtin_inff(), "huber_k must be finite and positive");     \
    PICP_REQUIRE(who, (fl) >= 0.0f && (fl) < __builtin_inff(), "huber_floor must be finite and not negative"); \
  } while (0)

// ------------------------------------------------------------------ the finish kernel's body
// One block per sequence.  S = the chunk partials in ascending chunk order, starting from the first
// (pi_column_sums<28, true>); then wave 0 either hands out the sums as they are (the table-level entry) or takes the
// Gauss-Newton step.
// COLOR: the colour solve's finish also adds up the chunks' colour-row counts (ccounts, an integer sum) and hands the
// total out as the ninth float of the trace row and through ccount_out.
template <bool COLOR>
GS_DEV void pi_finish(const PiSeq& q, const int nchunks, const float damp, const int32_t* __restrict__ ccounts,
                      int64_t* ccount_out) {
  __shared__ double S[LIN_NV];
  __shared__ float xi[8];
  __shared__ int64_t cnt[GS_PI_FIN / GS_WAVE];
  __shared__ int64_t ccnt[COLOR ? GS_PI_FIN / GS_WAVE : 1];
  const int tid = threadIdx.x, lane = tid & (GS_WAVE - 1);
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
  const double s = pi_column_sums<LIN_NV, true>(q.partials, nchunks);
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
      tr.pad[0] = q.delta_dev ? *q.delta_dev : 0.0f;   // (the threshold of the median rule; 0 for every other entry)
      tr.pad[1] = 0.0f;
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
// the parameter checks of a solve (the same for the plain, the colour and the backward entries)
#define PICP_CHECK_PARAMS(who, prm)                                                                                     \
  do {                                                                                                                  \
    PICP_REQUIRE(who, (prm).stride >= 1, "stride must be at least 1");                                                  \
    PICP_REQUIRE(who, (prm).numiters >= 1, "numiters must be at least 1");                                              \
    PICP_REQUIRE(who, (prm).damp > 0.0f && (prm).damp < __builtin_inff(), "damp must be positive and finite");          \
    PICP_REQUIRE(who, !((prm).dist_th != (prm).dist_th) && !((prm).dot_th != (prm).dot_th), "a threshold is NaN");      \
  } while (0)
// a Huber threshold of a robust entry (0: off), the weight of the colour term (0 for the plain entries)
#define PICP_CHECK_DELTA(who, d, name) \
  PICP_REQUIRE(who, (d) >= 0.0f && (d) < __builtin_inff(), name " must be finite and not negative")
#define PICP_CHECK_WEIGHT(who, w) \
  PICP_REQUIRE(who, (w) >= 0.0f && (w) < __builtin_inff(), "color_weight must be finite and not negative")

static inline void picp_fill(PiGeom& g, int B, int H, int W, int stride, float dist_th, float dot_th, float damp) {
  g.B = B; g.H = H; g.W = W; g.stride = stride;
  g.Wl = (int)gs_ceil_div(W, stride);
  g.nslots = (int)picp_slots(H, W, stride);
  g.nchunks = (int)gs_ceil_div(g.nslots, GS_PI_CHUNK);
  g.u_hi = (float)((double)W - 0.999); g.v_hi = (float)((double)H - 0.999);
  g.dist_th = dist_th; g.dot_th = dot_th; g.damp = damp;
}

// U: gs_picp_seq or gs_picp_backward_seq (they name the nine common fields alike)
template <typename U>
static inline void picp_fill_inputs(PiInputs& in, const U& u) {
  in.vertex = u.vertex; in.normal = u.normal; in.depth = u.depth; in.K16 = u.K16; in.index = u.index;
  in.model_pose16 = u.model_pose16;
  in.points = u.map.points; in.normals = u.map.normals;
  in.n = GsCount{u.map.n_bound, u.map.n_dev};
  in.weight = nullptr;
}

static inline void picp_fill_seq(PiSeq& s, const gs_picp_seq& u, int nchunks) {
  picp_fill_inputs(s.in, u);
  s.partials = static_cast<double*>(u.scratch);
  s.counts = reinterpret_cast<int32_t*>(static_cast<char*>(u.scratch) + picp_partials_bytes(nchunks));
  s.T_in = u.init_pose16; s.delta_dev = nullptr; s.T_out = nullptr; s.trace_row = nullptr; s.tape_row = nullptr;
  s.code_out = nullptr; s.row_out = nullptr; s.a_out = nullptr; s.b_out = nullptr;
  s.sums_out = nullptr; s.count_out = nullptr;
}

// ------------------------------------------------------------------ the host drivers of the forward entries
// Both drivers are templates over the traits X of a forward file (PiPlain in gs_picp.hip, PiJoint in gs_picp_color.hip):
//   X::Seq, X::Batch      the caller's descriptor of a sequence and the kernels' argument
//   X::TRACE              floats per trace row
//   X::linearize, X::robust_linearize, X::finish     the kernels: (Batch), (Batch, PiRobust), (Batch)
//   X::weighted_linearize  the WEIGHTED instance of the robust kernel: (Batch, PiRobust)
//   X::base(u), X::seq(pb, b)      the gs_picp_seq inside a Seq, the PiSeq inside a Batch
//   X::check(who, u)      the checks of a Seq (GS_OK or the error)
//   X::fill(pb, b, u, color_weight)      sequence b of the batch from u, the scratch carved, every output NULL
//   X::color_outputs(pb, o)       the colour tables of o into sequence 0
//   X::color_scale(pb, b, z, col) the colour inputs of sequence b into z, the descriptor of the median rule; col: the
//                                 sequence reads its colour threshold from z's device float (the plain solve: nothing)
//   X::scratch_bytes(nchunks)     bytes of a sequence's scratch (the median rule's keys and threshold lie behind them)
// The plain entries pass color_weight = cdelta = 0 and no colour tables; the checks of these pass.

// the table-level outputs, any may be NULL (the colour ones are NULL for the plain entries)
struct PiRowsOut {
  int32_t* code;
  int64_t* row;
  float *a6, *b, *ac6, *bc;
  int32_t* colored;
  double* sums28;
  int64_t *count, *color_count;
};

// a sequence's descriptor of the median rule: the inputs of s, the scratch behind the solve's own (16-byte aligned, which
// the scaled entries check: the select block reads the keys four at a time); s then reads its threshold from the rule's
// device float.  The colour residual's tables lie behind the geometric ones (picp_joint_scaled_bytes) and are touched
// only when the colour threshold is asked for
template <typename X>
static void picp_fill_scale(PiScaleSeq& z, typename X::Batch& pb, int b, const gs_picp_seq& u, const PiScale& sc) {
  const PiGeom& g = pb.g;
  PiSeq& s = X::seq(pb, b);
  char* p = static_cast<char*>(u.scratch) + X::scratch_bytes(g.nchunks);
  z.in = s.in;
  z.T_in = s.T_in;
  for (int i = 0; i < PS_RESIDUALS; ++i, p += picp_scaled_bytes(0, g.nslots)) {
    z.r[i].keys = reinterpret_cast<uint32_t*>(p);
    z.r[i].hist = reinterpret_cast<uint32_t*>(p + picp_keys_bytes(g.nslots));
    z.r[i].delta_dev = reinterpret_cast<float*>(p + picp_keys_bytes(g.nslots) + picp_hist_bytes());
    z.r[i].delta_out = nullptr;
  }
  if (sc.on[PS_GEO]) s.delta_dev = z.r[PS_GEO].delta_dev;
  X::color_scale(pb, b, z, sc.on[PS_COLOR]);
}

// the solve behind the batch entries; tapes_host: per sequence the device buffer of numiters tape rows, or NULL
// (untaped); delta / cdelta: the Huber thresholds of the robust entries (both 0: the plain kernel); sc: the median rule
// of the scaled entries (delta is then not read: every sequence has its device threshold), or NULL; weights_host: per
// sequence the device image (H, W) of pixel weights or NULL (that sequence has none), weighted: the weighted entries
// (weights_host must then be there; the WEIGHTED kernels run whatever the thresholds)
template <typename X>
static int picp_solve(const char* who, const typename X::Seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                      const gs_picp_params* params_host, float color_weight, float delta, float cdelta,
                      const PiScale* sc, void* stream, const float* const* weights_host = nullptr, bool weighted = false) {
  PICP_REQUIRE(who, seqs_host && params_host && B > 0 && H > 0 && W > 0, "bad arguments");
  PICP_REQUIRE(who, !weighted || weights_host, "NULL pointer (weights)");
  PICP_REQUIRE(who, (int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  const gs_picp_params& prm = *params_host;
  PICP_CHECK_PARAMS(who, prm);
  PICP_CHECK_WEIGHT(who, color_weight);
  PICP_CHECK_DELTA(who, delta, "huber_delta");
  PICP_CHECK_DELTA(who, cdelta, "color_huber_delta");
  for (int b = 0; b < B; ++b) {
    if (const int err = X::check(who, seqs_host[b])) return err;
    PICP_REQUIRE(who, X::base(seqs_host[b]).out_pose16, "NULL pointer (out_pose16)");
    for (int i = 0; sc && i < PS_RESIDUALS; ++i)
      PICP_REQUIRE(who, !sc->on[i] || !sc->deltas_host[i] || sc->deltas_host[i][b], "NULL pointer (deltas)");
    PICP_REQUIRE(who, !sc || ((uintptr_t)X::base(seqs_host[b]).scratch & 15) == 0, "scratch must be 16-byte aligned");
    PICP_REQUIRE(who, !tapes_host || (tapes_host[b] && ((uintptr_t)tapes_host[b] & 7) == 0), "NULL or misaligned tape");
  }
  hipStream_t st = gs_stream(stream);
  const PiRobust rb{delta, cdelta, nullptr, nullptr};
  const bool robust = delta > 0.0f || cdelta > 0.0f || sc;
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    typename X::Batch pb;
    PiScaleBatch sb;
    picp_fill(pb.g, nb, H, W, prm.stride, prm.dist_th, prm.dot_th, prm.damp);
    sb.g = pb.g;
    for (int b = 0; b < nb; ++b) {
      X::fill(pb, b, seqs_host[c0 + b], color_weight);
      X::seq(pb, b).T_out = X::base(seqs_host[c0 + b]).out_pose16;
      if (weighted) X::seq(pb, b).in.weight = weights_host[c0 + b];
      if (sc) picp_fill_scale<X>(sb.s[b], pb, b, X::base(seqs_host[c0 + b]), *sc);
    }
    const unsigned blocks = (unsigned)nb * (unsigned)pb.g.nchunks;   // < 8 * 2^23
    for (int it = 0; it < prm.numiters; ++it) {
      for (int b = 0; b < nb; ++b) {
        const gs_picp_seq& u = X::base(seqs_host[c0 + b]);
        PiSeq& s = X::seq(pb, b);
        s.T_in = it == 0 ? u.init_pose16 : u.out_pose16;
        s.trace_row = u.trace ? u.trace + (int64_t)X::TRACE * it : nullptr;
        s.tape_row = tapes_host ? static_cast<PiTapeRow*>(tapes_host[c0 + b]) + it : nullptr;
        if (sc) {
          sb.s[b].T_in = s.T_in;
          for (int i = 0; i < PS_RESIDUALS; ++i)
            sb.s[b].r[i].delta_out = sc->on[i] && sc->deltas_host[i] ? sc->deltas_host[i][c0 + b] + it : nullptr;
        }
      }
      if (sc) picp_scale_launch(sb, picp_scale_pick(*sc), it == 0, weighted, st);
      if (weighted)
        hipLaunchKernelGGL(X::weighted_linearize, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, rb);
      else if (robust)
        hipLaunchKernelGGL(X::robust_linearize, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb, rb);
      else
        hipLaunchKernelGGL(X::linearize, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb);
      hipLaunchKernelGGL(X::finish, dim3(nb), dim3(GS_PI_FIN), 0, st, pb);
    }
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}

// the linearisation behind the table-level entries; rb: the thresholds and the weight tables of the robust entries (a
// table with both thresholds 0: the robust kernel writes 1 for every row there is); sc: the median rule, or NULL;
// weights / weighted: the weighted entries' image of pixel weights (the tables then hold the total weights)
template <typename X>
static int picp_rows(const char* who, const typename X::Seq* seq_host, int H, int W, int stride, float dist_th,
                     float dot_th, float color_weight, const PiRobust& rb, const PiRowsOut& o, const PiScale* sc,
                     void* stream, const float* weights = nullptr, bool weighted = false) {
  PICP_REQUIRE(who, seq_host && H > 0 && W > 0, "bad arguments");
  PICP_REQUIRE(who, !weighted || weights, "NULL pointer (weights)");
  PICP_REQUIRE(who, (int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  PICP_REQUIRE(who, stride >= 1, "stride must be at least 1");
  PICP_REQUIRE(who, !(dist_th != dist_th) && !(dot_th != dot_th), "a threshold is NaN");
  PICP_CHECK_WEIGHT(who, color_weight);
  PICP_CHECK_DELTA(who, rb.delta, "huber_delta");
  PICP_CHECK_DELTA(who, rb.cdelta, "color_huber_delta");
  if (const int err = X::check(who, *seq_host)) return err;
  PICP_REQUIRE(who, !sc || ((uintptr_t)X::base(*seq_host).scratch & 15) == 0, "scratch must be 16-byte aligned");
  hipStream_t st = gs_stream(stream);
  typename X::Batch pb;
  picp_fill(pb.g, 1, H, W, stride, dist_th, dot_th, 1.0f);
  X::fill(pb, 0, *seq_host, color_weight);
  PiSeq& s = X::seq(pb, 0);
  s.code_out = o.code; s.row_out = o.row; s.a_out = o.a6; s.b_out = o.b;
  s.sums_out = o.sums28; s.count_out = o.count;
  X::color_outputs(pb, o);
  if (weighted) s.in.weight = weights;
  if (sc) {   // the threshold at init_pose16 first: two launches in front of the robust linearisation
    PiScaleBatch sb;
    sb.g = pb.g;
    picp_fill_scale<X>(sb.s[0], pb, 0, X::base(*seq_host), *sc);
    for (int i = 0; i < PS_RESIDUALS; ++i) sb.s[0].r[i].delta_out = sc->on[i] ? sc->delta_out[i] : nullptr;
    picp_scale_launch(sb, picp_scale_pick(*sc), true, weighted, st);
  }
  if (weighted)
    hipLaunchKernelGGL(X::weighted_linearize, dim3((unsigned)pb.g.nchunks), dim3(GS_PI_CHUNK), 0, st, pb, rb);
  else if (sc || rb.delta > 0.0f || rb.cdelta > 0.0f || rb.weight_out || rb.cweight_out)
    hipLaunchKernelGGL(X::robust_linearize, dim3((unsigned)pb.g.nchunks), dim3(GS_PI_CHUNK), 0, st, pb, rb);
  else
    hipLaunchKernelGGL(X::linearize, dim3((unsigned)pb.g.nchunks), dim3(GS_PI_CHUNK), 0, st, pb);
  if (o.sums28 || o.count || o.color_count) hipLaunchKernelGGL(X::finish, dim3(1), dim3(GS_PI_FIN), 0, st, pb);
  GS_LAUNCH_CHECK();
  return GS_OK;
}
