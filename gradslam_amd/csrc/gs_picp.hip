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
#include "gs_picp_dev.h"

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
struct PiBatch {
  PiSeq s[GS_MAX_BATCH];
  int B, H, W, stride, Wl, nslots, nchunks;
  float u_hi, v_hi, dist_th, dot_th, damp;
};

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_linearize_kernel(const PiBatch pb) {
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  __shared__ double red[GS_PI_CHUNK / GS_WAVE][LIN_NV];
  __shared__ int cnt[GS_PI_CHUNK / GS_WAVE];
  const PiSeq& q = pb.s[blockIdx.x % pb.B];
  const int chunk = blockIdx.x / pb.B;
  if (threadIdx.x == 0) cam = gs_camera(q.model_pose16, q.K16);
  if (threadIdx.x >= GS_WAVE && threadIdx.x < GS_WAVE + 12) Ts[threadIdx.x - GS_WAVE] = q.T_in[threadIdx.x - GS_WAVE];
  __syncthreads();
  const int lane = threadIdx.x & (GS_WAVE - 1), wave = threadIdx.x / GS_WAVE;
  const int k = chunk * GS_PI_CHUNK + (int)threadIdx.x;
  const bool in_lattice = k < pb.nslots;
  const int64_t n_map = gs_count(q.n);
  int code = 1;
  int64_t row = -1;
  float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, b = 0.0f;
  if (in_lattice) {
    const int i = k / pb.Wl, j = k - i * pb.Wl;
    const int64_t p = (int64_t)(i * pb.stride) * pb.W + j * pb.stride;
    float s[3];
    float4 d, m;
    code = pi_associate(Ts, cam, q.vertex, q.normal, q.depth, q.index, q.points, q.normals, n_map, p, pb.H, pb.W, pb.u_hi,
                        pb.v_hi, pb.dist_th, pb.dot_th, row, s, d, m);
    if (code == 0) gn_row_pn(s[0], s[1], s[2], d, m, a, b);
    if (q.code_out) q.code_out[k] = code;
    if (q.row_out) q.row_out[k] = row;
    if (q.a_out) {
#pragma unroll
      for (int c = 0; c < 6; ++c) q.a_out[6 * (int64_t)k + c] = a[c];
    }
    if (q.b_out) q.b_out[k] = b;
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
      const double x = pi_wave_tree((double)a[r] * (double)a[c], any);
      if (lane == 0) red[wave][t] = x;
      ++t;
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double x = pi_wave_tree((double)a[r] * (double)b, any);
    if (lane == 0) red[wave][21 + r] = x;
  }
  {
    const double x = pi_wave_tree((double)b * (double)b, any);
    if (lane == 0) red[wave][27] = x;
  }
  __syncthreads();
  if (threadIdx.x < LIN_NV)
    q.partials[(int64_t)chunk * LIN_NV + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  if (threadIdx.x == GS_WAVE) q.counts[chunk] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}

// One block per sequence.  S = the chunk partials in ascending chunk order, starting from the first: a serial chain by
// contract, so what has to be kept off it is the memory latency -- a lane that loaded its partial of chunk c, added it and
// only then asked for chunk c + 1 would pay a trip to memory per chunk (measured: 0.25 us each, 300 us at 1 200 chunks).
// All 256 threads move the table through LDS a tile of 256 chunks at a time (coalesced, 28 loads in flight per thread, the
// next tile on its way while lane i < 28 of wave 0 adds column i of the current one); then wave 0 either hands out the
// sums as they are (the table-level entry) or takes the Gauss-Newton step.
constexpr int GS_PI_FIN = 256;    // threads of the finish block
constexpr int GS_PI_TILE = 256;   // chunks per LDS tile: GS_PI_TILE * 28 doubles = 56 KB

__global__ void __launch_bounds__(GS_PI_FIN) gs_picp_finish_kernel(const PiBatch pb) {
  static_assert(GS_PI_TILE * LIN_NV % GS_PI_FIN == 0, "a tile is a whole number of loads per thread");
  constexpr int PER = GS_PI_TILE * LIN_NV / GS_PI_FIN;   // 28
  __shared__ double tile[GS_PI_TILE * LIN_NV];
  __shared__ double S[LIN_NV];
  __shared__ float xi[8];
  __shared__ int64_t cnt[GS_PI_FIN / GS_WAVE];
  const PiSeq& q = pb.s[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & (GS_WAVE - 1);
  const int64_t total = (int64_t)pb.nchunks * LIN_NV;
  int64_t n = 0;
  for (int c = tid; c < pb.nchunks; c += GS_PI_FIN) n += q.counts[c];
#pragma unroll
  for (int d = 1; d < GS_WAVE; d <<= 1) n += __shfl_xor(n, d, GS_WAVE);
  if (lane == 0) cnt[tid / GS_WAVE] = n;
  double nxt[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int64_t i = tid + GS_PI_FIN * r;
    nxt[r] = i < total ? q.partials[i] : 0.0;
  }
  double s = 0.0;
  for (int base = 0; base < pb.nchunks; base += GS_PI_TILE) {
    __syncthreads();   // (the tile of the round before has been added up)
#pragma unroll
    for (int r = 0; r < PER; ++r) tile[tid + GS_PI_FIN * r] = nxt[r];
    __syncthreads();
    if (base + GS_PI_TILE < pb.nchunks) {
#pragma unroll
      for (int r = 0; r < PER; ++r) {
        const int64_t i = (int64_t)(base + GS_PI_TILE) * LIN_NV + tid + GS_PI_FIN * r;
        nxt[r] = i < total ? q.partials[i] : 0.0;
      }
    }
    if (tid < LIN_NV) {
      const int m = pb.nchunks - base < GS_PI_TILE ? pb.nchunks - base : GS_PI_TILE;
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
  if (tid == 0 && q.count_out) *q.count_out = n;
  if (!q.T_out) return;
  if (n > 0) gs_solve_spd6_wave(S, pb.damp, xi);   // (n is the same in every lane)
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

static size_t picp_partials_bytes(int64_t nchunks) { return gs_align((size_t)nchunks * LIN_NV * sizeof(double)); }

extern "C" int64_t gs_projective_icp_scratch_bytes(int H, int W, int stride) {
  if (H <= 0 || W <= 0 || stride <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  const int64_t nchunks = gs_ceil_div(picp_slots(H, W, stride), GS_PI_CHUNK);
  return (int64_t)(picp_partials_bytes(nchunks) + gs_align((size_t)nchunks * sizeof(int32_t)));
}

// (the checks of the solve run in a helper shared by two entries: the message names the entry that was called)
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

static void picp_fill(PiBatch& pb, int H, int W, int stride, float dist_th, float dot_th, float damp) {
  pb.H = H; pb.W = W; pb.stride = stride;
  pb.Wl = (int)gs_ceil_div(W, stride);
  pb.nslots = (int)picp_slots(H, W, stride);
  pb.nchunks = (int)gs_ceil_div(pb.nslots, GS_PI_CHUNK);
  pb.u_hi = (float)((double)W - 0.999); pb.v_hi = (float)((double)H - 0.999);
  pb.dist_th = dist_th; pb.dot_th = dot_th; pb.damp = damp;
}

static void picp_fill_seq(PiSeq& s, const gs_picp_seq& u, int nchunks) {
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

extern "C" int64_t gs_projective_icp_tape_bytes(int numiters) {
  return numiters >= 1 ? (int64_t)numiters * (int64_t)sizeof(PiTapeRow) : 0;
}

// the solve behind both entries; tapes_host: per sequence the device buffer of numiters tape rows, or NULL (untaped)
static int picp_solve(const char* who, const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                      const gs_picp_params* params_host, void* stream) {
  PICP_REQUIRE(who, seqs_host && params_host && B > 0 && H > 0 && W > 0, "bad arguments");
  PICP_REQUIRE(who, (int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  const gs_picp_params& prm = *params_host;
  PICP_REQUIRE(who, prm.stride >= 1, "stride must be at least 1");
  PICP_REQUIRE(who, prm.numiters >= 1, "numiters must be at least 1");
  PICP_REQUIRE(who, prm.damp > 0.0f && prm.damp < __builtin_inff(), "damp must be positive and finite");
  PICP_REQUIRE(who, !(prm.dist_th != prm.dist_th) && !(prm.dot_th != prm.dot_th), "a threshold is NaN");
  for (int b = 0; b < B; ++b) {
    PICP_CHECK_SEQ(who, seqs_host[b]);
    PICP_REQUIRE(who, seqs_host[b].out_pose16, "NULL pointer (out_pose16)");
    PICP_REQUIRE(who, !tapes_host || (tapes_host[b] && ((uintptr_t)tapes_host[b] & 7) == 0), "NULL or misaligned tape");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    PiBatch pb;
    pb.B = nb;
    picp_fill(pb, H, W, prm.stride, prm.dist_th, prm.dot_th, prm.damp);
    for (int b = 0; b < nb; ++b) {
      picp_fill_seq(pb.s[b], seqs_host[c0 + b], pb.nchunks);
      pb.s[b].T_out = seqs_host[c0 + b].out_pose16;
    }
    const unsigned blocks = (unsigned)nb * (unsigned)pb.nchunks;   // < 8 * 2^23
    for (int it = 0; it < prm.numiters; ++it) {
      for (int b = 0; b < nb; ++b) {
        const gs_picp_seq& u = seqs_host[c0 + b];
        pb.s[b].T_in = it == 0 ? u.init_pose16 : u.out_pose16;
        pb.s[b].trace_row = u.trace ? u.trace + (int64_t)GS_PI_TRACE * it : nullptr;
        pb.s[b].tape_row = tapes_host ? static_cast<PiTapeRow*>(tapes_host[c0 + b]) + it : nullptr;
      }
      hipLaunchKernelGGL(gs_picp_linearize_kernel, dim3(blocks), dim3(GS_PI_CHUNK), 0, st, pb);
      hipLaunchKernelGGL(gs_picp_finish_kernel, dim3(nb), dim3(GS_PI_FIN), 0, st, pb);
    }
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}

extern "C" int gs_projective_icp_batch_f32(const gs_picp_seq* seqs_host, int B, int H, int W,
                                           const gs_picp_params* params_host, void* stream) {
  return picp_solve(__func__, seqs_host, nullptr, B, H, W, params_host, stream);
}

extern "C" int gs_projective_icp_tape_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                                                const gs_picp_params* params_host, void* stream) {
  GS_REQUIRE(tapes_host, "NULL pointer (tapes)");
  return picp_solve(__func__, seqs_host, tapes_host, B, H, W, params_host, stream);
}

extern "C" int gs_projective_icp_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                          float dot_th, int32_t* code, int64_t* row, float* a6, float* b,
                                          double* sums28, int64_t* count, void* stream) {
  GS_REQUIRE(seq_host && H > 0 && W > 0, "bad arguments");
  GS_REQUIRE((int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  GS_REQUIRE(stride >= 1, "stride must be at least 1");
  GS_REQUIRE(!(dist_th != dist_th) && !(dot_th != dot_th), "a threshold is NaN");
  PICP_CHECK_SEQ(__func__, *seq_host);
  hipStream_t st = gs_stream(stream);
  PiBatch pb;
  pb.B = 1;
  picp_fill(pb, H, W, stride, dist_th, dot_th, 1.0f);
  picp_fill_seq(pb.s[0], *seq_host, pb.nchunks);
  pb.s[0].code_out = code; pb.s[0].row_out = row; pb.s[0].a_out = a6; pb.s[0].b_out = b;
  pb.s[0].sums_out = sums28; pb.s[0].count_out = count;
  hipLaunchKernelGGL(gs_picp_linearize_kernel, dim3((unsigned)pb.nchunks), dim3(GS_PI_CHUNK), 0, st, pb);
  if (sums28 || count) hipLaunchKernelGGL(gs_picp_finish_kernel, dim3(1), dim3(GS_PI_FIN), 0, st, pb);
  GS_LAUNCH_CHECK();
  return GS_OK;
}
