// gs_icp_loop.hip — the device-resident LM loop of point_to_plane_ICP / point_to_plane_gradICP
// (odometry/icputils.py:235-367, :370-545): 2 exact 1-NN searches, one Gauss-Newton linearisation,
// one 6x6 solve, two SE(3) exponentials per iteration, 20 iterations, no host sync.
//
// Normal equations are accumulated in float64 from float32 products (order-independent to ~1e-16,
// so HIP and oracle agree after the single rounding to float32) with fixed-order reductions.
//
// Grid path (large target sets; the SLAM loop): ONE kernel per half-iteration.  Its prologue lets
// every block redundantly finish the PREVIOUS half-iteration (add up the partial rows the previous
// kernel left, then the scalar stage: solve + se3_exp, or LM / gradLM update) so that no separate
// single-block kernels sit on the critical path; block 0 records the state.  Then 8, 4 or 2 lanes per
// source point run the grid search (gs_knn.h), the block finishes unresolved queries by brute
// force, builds the Gauss-Newton rows and emits one partial row per 96 source points.  State and
// partial rows are double-buffered between consecutive kernels.  2 x numiters + 1 launches per solve.
// This is the ONE solve path: the batched localisation adds candidate lists to it (ordinary lists of
// every source point, wide lists of the hard ones: list modes 0 / 1 / 2 of the same kernel), the
// single solve runs it without.
//
// Brute-force path (small problems, GRADSLAM_HIP_KNN=brute): search / linearise / solve / update
// as separate kernels.
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <optional>
#include <type_traits>

#include "gs_env.h"
#include "gs_icp_math.h"
#include "gs_knn.h"
#include "gs_knn_bbox.h"

constexpr int GS_ICP_MAX_ITERS = 1024;  // rows of the per-iteration trace kept in the scratch
struct GsIcpState {
  IcpSmall s[2];                        // double-buffered by the grid path; the brute-force path uses s[0]
  float trace[GS_ICP_MAX_ITERS * 12];   // [err, new_err, damp, sigmoid, xi(6), 0, 0] per iteration
};

// Optional forward tape for gs_icp_backward_f32 (layout: gs_icp_math.h:GsIcpTape).
struct TapePtrs {
  float* src;    // [K][n_src][3]
  int32_t* idx;  // [K][2][n_src]
  float* sys;    // [K][28]
};
GS_DEV void tape_write_sys(float* __restrict__ sys, int it, const double* S, float damp) {
  float* t = sys + 28 * it;
  for (int i = 0; i < 27; ++i) t[i] = (float)S[i];
  t[27] = damp;
}

// ---------------------------------------------------------------- fixed-order sums ------
// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a release fence that also drains the wave's
// outstanding GLOBAL loads (s_waitcnt vmcnt(0)); the list variants of the half-iteration kernel keep the gathers of
// their candidate lists in flight across the whole prologue, which is the point of issuing them there.
GS_DEV void gs_barrier_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
template <bool LDS_ONLY>
GS_DEV void gs_bar() {
  if (LDS_ONLY) gs_barrier_lds();
  else __syncthreads();
}

// Adds up partial rows (nrows x LIN_NV doubles).  Thread t works on value t%32 and the contiguous
// chunk of CH rows number t/32 (then every STEP*CH rows further): its CH loads are 224 B apart, i.e.
// one base address with immediate offsets, all in flight together; the chunk sums are then added in
// chunk order.  Every block that runs this on the same rows gets bit-identical sums.
template <int BLOCK, int CH = 18>
GS_DEV void icp_sum_rows(const double* __restrict__ partials, int nrows, double* S, double (*sub)[32]) {
  constexpr int STEP = BLOCK / 32;
  // CH = rows per thread per round of independent loads: a 640x480 solve of the row-unit engine (200 rows of 96
  // queries, 9 per thread at 768 threads) is ONE round of memory latency with 18; more rows in flight would push
  // the kernel past 80 VGPRs (2 resident blocks per CU).
  const int i = threadIdx.x & 31, j = threadIdx.x >> 5;
  double s = 0.0;
  if (i < LIN_NV) {
    for (int b = j * CH; b < nrows; b += CH * STEP) {
      const double* base = partials + (int64_t)b * LIN_NV + i;
      const int left = nrows - b;
      double a[CH];
#pragma unroll
      for (int u = 0; u < CH; ++u) a[u] = (u < left) ? base[u * LIN_NV] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; ++u) s += a[u];
    }
  }
  sub[j][i] = s;
  __syncthreads();
  if (threadIdx.x < LIN_NV) {
    double t = 0.0;
    for (int k = 0; k < STEP; ++k) t += sub[k][threadIdx.x];
    S[threadIdx.x] = t;
  }
  __syncthreads();
}

// hook(): called by EVERY thread once the first round of loads has been issued and before it is used (the list variants
// of the half-iteration kernel issue their dependent gathers there: behind the row loads in the queue, in front of the
// wait for them).
// The same sums with HALF the loads in flight per thread (9 instead of 18: 18 VGPRs less at the point where the list
// variants of the half-iteration kernel also hold their gathered candidates), bit for bit: a wave owns chunk j = its
// index (and chunk j + BLOCK / 64 in a second pass, which only solves of more than 9 * BLOCK / 32 rows need); lanes
// 0-31 add the first nine rows of the chunk in order, hand the running sum to lanes 32-63, which add the other nine --
// the order of icp_sum_rows<BLOCK, 18>, whose thread j adds its 18 rows one after the other.
template <int BLOCK, class Hook>
GS_DEV void icp_sum_rows_split(const double* __restrict__ partials, int nrows, double* S, double (*sub)[32], Hook hook) {
  constexpr int CH = 18, HC = CH / 2, STEP = BLOCK / 32, NW = BLOCK / GS_WAVE;
  static_assert(2 * NW == STEP, "two chunks per wave");
  // (an opaque copy of the thread index: merged with the uses at the far end of the kernel, the wave index computed
  // here would be the one value the register allocator spills -- and a spill is a store in the memory queue of the
  // prologue, behind which every wait for a load drains the queue)
  unsigned tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int ln = tid & (GS_WAVE - 1), i = ln & 31, half = ln >> 5, w = tid / GS_WAVE;
  const bool act = i < LIN_NV;
  double tot[2];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int j = w + pass * NW;   // wave-uniform
    double t = 0.0;
    if (pass == 0 || j * CH < nrows) {
      for (int b = j * CH, r = 0; r == 0 || b < nrows; b += CH * STEP, ++r) {   // (r > 0: solves of more than 432 rows)
        // UNCONDITIONAL loads, masked afterwards: a load under a branch may not have been issued, and the compiler then
        // has to wait for ALL outstanding loads wherever it needs an older one -- here that would drain the gathers the
        // hook puts in flight.  Rows beyond nrows (at most 24 x 18 of them from the start of the buffer, 97 KB; the
        // single-column variant below: FS_BLOCK rows, 172 KB) are read from what follows the rows in the caller's
        // scratch (the second row buffer, the grid, the lists -- loc_lists_fit checks that they cover it before a
        // solve with lists is planned) and never looked at; one base address + immediate offsets, as in icp_sum_rows.
        const int b0 = b + half * HC;
        const int left = act ? nrows - b0 : 0;
        const double* base = partials + (int64_t)b0 * LIN_NV + i;
        double a[HC];
#pragma unroll
        for (int u = 0; u < HC; ++u) a[u] = base[u * LIN_NV];
        if (pass == 0 && r == 0) hook();
#pragma unroll
        for (int u = 0; u < HC; ++u) a[u] = (u < left) ? a[u] : 0.0;
        const double carry = __shfl(t, i + 32, GS_WAVE);   // the running sum of the chunk lives in the upper half-wave
        if (half == 0) {
          t = carry;
#pragma unroll
          for (int u = 0; u < HC; ++u) t += a[u];
        }
        const double lo = __shfl(t, i, GS_WAVE);
        if (half == 1) {
          t = lo;
#pragma unroll
          for (int u = 0; u < HC; ++u) t += a[u];
        }
      }
    }
    tot[pass] = t;
  }
  if (half == 1) {
    sub[w][i] = tot[0];
    sub[w + NW][i] = tot[1];
  }
  gs_barrier_lds();
  if (threadIdx.x < LIN_NV) {
    double t = 0.0;
    for (int k = 0; k < STEP; ++k) t += sub[k][threadIdx.x];
    S[threadIdx.x] = t;
  }
  gs_barrier_lds();
}

// Same for the single residual column (value 27): all threads share the rows.
template <int BLOCK>
GS_DEV double icp_sum_col27(const double* __restrict__ partials, int nrows, double* red) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nrows; b += BLOCK) s += partials[(int64_t)b * LIN_NV + 27];
  s = gs_wave_sum_f64(s);
  if ((threadIdx.x & (GS_WAVE - 1)) == 0) red[threadIdx.x / GS_WAVE] = s;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < BLOCK / GS_WAVE; ++w) t += red[w];
  __syncthreads();
  return t;
}
// ... with the hook of icp_sum_rows_split and barriers that order LDS only (the same additions in the same order)
template <int BLOCK, class Hook>
GS_DEV double icp_sum_col27_hook(const double* __restrict__ partials, int nrows, double* red, Hook hook) {
  double s = 0.0;
  {
    const bool has = (int)threadIdx.x < nrows;   // (unconditional load, masked afterwards: see icp_sum_rows_split)
    double a0 = partials[(int64_t)threadIdx.x * LIN_NV + 27];
    hook();
    a0 = has ? a0 : 0.0;
    s += a0;
  }
  for (int b = threadIdx.x + BLOCK; b < nrows; b += BLOCK) s += partials[(int64_t)b * LIN_NV + 27];
  s = gs_wave_sum_f64(s);
  if ((threadIdx.x & (GS_WAVE - 1)) == 0) red[threadIdx.x / GS_WAVE] = s;
  gs_barrier_lds();
  double t = 0.0;
  for (int w = 0; w < BLOCK / GS_WAVE; ++w) t += red[w];
  gs_barrier_lds();
  return t;
}

// ---------------------------------------------------------------- grid path -------------
constexpr int FS_BLOCK = 768;            // 12 waves; 2 blocks per CU keep all 200 blocks of a 640x480 solve resident
                                         // (measured alternatives at 8 lanes per query: 512 threads 11.8 us,
                                         // 1024 threads 11.2 us, 768 threads 10.7 us per kernel)
constexpr int FS_HARD_RINGS = 5;         // cube radius (cells) the 16-lane groups go to before the brute-force fallback
constexpr int FS_BQ = 4;                 // queries per pass of the block-wide brute-force fallback
constexpr int FS_QPB = FS_BLOCK / GQ_G;  // 96 queries per block, their rows are built by the first two waves
constexpr int FS_RPG = (FS_QPB / 4) * LIN_NV <= FS_BLOCK ? 4 : 8;  // rows per group in the block reduction
constexpr int FS_RG = FS_QPB / FS_RPG;                            // row groups
constexpr int FS_HG = 16;  // lanes per query of the shell search for queries the 2x2x2 stage leaves open
constexpr int FS_LISTS_FROM = 1;   // iteration behind whose look-ahead search the candidate lists of ordinary queries are built
static_assert(FS_QPB <= 2 * GS_WAVE && FS_QPB % FS_RPG == 0 && FS_RG * LIN_NV <= FS_BLOCK, "block shape");

// FULL = true : first half of iteration `it`  (prologue: LM update of iteration it-1, then search
//               with T_step applied, full normal equations)
// FULL = false: look-ahead half              (prologue: solve + se3_exp, then search with Tr
//               applied, residual only)
// Workgroups are dealt round-robin to the 8 XCDs (block i runs on XCD i % 8), each with its own L2.
// Logical block ids are therefore assigned so that every XCD works on ONE contiguous eighth of the
// query rows: consecutive queries are neighbouring pixels of the frame, so the slice of the binned
// target set an XCD touches is an eighth of the whole (+ halo) and stays resident in its L2 across
// the 2 x numiters kernels of a solve (the full set of a 1296x968 frame is larger than one L2).
constexpr unsigned GS_XCDS = 8;
// b-th of nb blocks that are dealt round-robin to X XCDs -> logical block such that every XCD owns one contiguous
// range of logical blocks
GS_DEV unsigned gs_xcd_block(unsigned b, unsigned nb, unsigned X = GS_XCDS) {
  const unsigned q = nb / X, r = nb % X, x = b % X;
  return x * q + (x < r ? x : r) + b / X;
}

// What one sequence contributes to a half-iteration launch (the batched launch carries up to GS_MAX_BATCH of them).
struct IcpHalfSeq {
  const float* src_in;
  float* src_out;
  const float* tgt;
  const float* tn;
  GsCount n_tgt;
  const GsGrid* gp;
  const int* cell_start;
  const float4* sorted;
  const float4* sorted_n;   // normals binned with the targets (NULL: gather from tn)
  float* d2prev;            // [n_src] squared distance of every source point's neighbour in the previous half-iteration
                            // (written by every launch, read by the next; NULL: no search bound)
  const double* partials_in;
  double* partials_out;
  const IcpSmall* st_in;
  IcpSmall* st_out;
  float* trace;
  int64_t* out_idx;
  int32_t* tape_idx;
  float* tape_sys;
};
// WIDE lists of hard queries (round 5, gs_knn.h: far_write_from_top / block_brute_min_list_multi; cq == NULL: none kept):
// cq[s] = (position the list of source point s was made at, exactness radius; 0: no list), c[GS_FAR_SLOTS * s ..] = its
// slots.  Written by whatever serves a hard query (cube scan, block-wide pass) in any launch of the solve, checked first
// thing by the 16-lane group that serves it in every later launch; the prep launch of a frame clears every point's radius
// (nothing of an earlier frame is ever read).
struct IcpHalfWide {
  float4* cq;
  uint32_t* c;
};
// candidate lists of ordinary queries (gs_knn.h: gl_*; lq == NULL: none): lq[s] = (position the list of source point s
// was built at, exactness radius), ls[GL_SLOTS * s ..] = its slots of `sorted`, lstat = failure counters per launch
struct IcpHalfLists {
  float4* lq;
  uint32_t* ls;
  int* lstat;
  unsigned* weak_n;   // (list-building launch with GRADSLAM_HIP_ICP_WEAK_ROOM) weak lists flagged (IcpScratch::weak_n)
};

// An entry of the block's list of left-over queries (hard_q) is a slot; its two top bits were flags once and are still
// masked off where it is read: without that one AND the compiler allocates the registers of the whole left-over pass anew
// (profiles/retired_engines_isa.txt), and these kernels change only with a measurement.
constexpr int FS_HQ_SLOT = 0x3fffffff;

// index pairs (into [a0..a5, res]) of the 28 accumulated products: 21 upper-triangular a_i a_k, 6 a_i res, res res
// (three bits per entry in two 64-bit literals for the 21 matrix products; entries 21..27 are (i - 21, 6).  A table in
// constant memory would pin two 64-bit addresses in VGPRs across the whole kernel, which sits at the 80-VGPR limit.)
constexpr unsigned long long FS_PA_BITS = 0x591b692449240000ull;  // 0 0 0 0 0 0 1 1 1 1 1 2 2 2 2 3 3 3 4 4 5
constexpr unsigned long long FS_PB_BITS = 0x5b2c76356346c688ull;  // 0 1 2 3 4 5 1 2 3 4 5 2 3 4 5 3 4 5 4 5 5
GS_DEV int fs_pa(int i) { return i < 21 ? (int)((FS_PA_BITS >> (3 * i)) & 7ull) : i - 21; }
GS_DEV int fs_pb(int i) { return i < 21 ? (int)((FS_PB_BITS >> (3 * i)) & 7ull) : 6; }

// One half-iteration for one sequence.  G lanes serve a query, so a block holds NQ = FS_BLOCK / G query slots =
// NU row units of FS_QPB (96) queries.  Every unit produces ONE partial row, always with the same fixed-order sums,
// so the normal equations do not depend on G, on the number of blocks or on which block works on which unit: a
// block owns the contiguous units [lb * upb, (lb + 1) * upb) and walks them NU at a time (grids smaller than the
// unit count are how a GPU shared by 8 sequences keeps every block resident and pays the prologue once per block).
// LISTS (round 4): candidate lists of ordinary queries (gs_knn.h: gl_*), lmode = what this launch does with them:
//   0  nothing (the first search of a solve: the large step of iteration 0 follows)
//   1  every group builds the list of its point behind the search (the look-ahead of iteration 0)
//   2  the lists are tried first: their slots, the list centre and the listed points are fetched BEFORE the prologue
//      waits for the partial rows of the previous launch (the gathers ride behind the row loads and stay in flight
//      across the scalar stage: its barriers order LDS only), so a launch whose lists all prove has no search on its
//      critical path.  A list that gives no proof sends its point to the left-over pass, where a 16-lane group
//      scans the 2x2x2 block and writes a new list.
// Results do not depend on any of it: a proof is exact, everything else is the search that ran before.
template <bool FULL, int G, int LMODE>
GS_DEV void icp_half_body(const IcpHalfSeq& q, const IcpHalfLists& ql, const IcpHalfWide& qw, const GsCount n_src_c, const float dist_thresh,
                          const gs_icp_params& prm, const int it, const int rows_in_reduced, const unsigned lb,
                          const int upb, unsigned long long* __restrict__ tl_arg = nullptr, const float weak_room = 0.0f) {
  constexpr bool LISTS = LMODE != 0;
#ifdef GS_ICP_TIMELINE
  unsigned long long* __restrict__ tl = tl_arg;
#else
  constexpr unsigned long long* tl = nullptr;  // per-block timeline stamps: debugging builds only (-DGS_ICP_TIMELINE)
#endif
  constexpr int NQ = FS_BLOCK / G, NU = NQ / FS_QPB;
  constexpr int LK = gl_k<G>(), LM = G * LK;   // list entries per lane / per source point
  static_assert(NQ % FS_QPB == 0 && 2 * NU <= FS_BLOCK / GS_WAVE && LM <= GL_SLOTS, "block shape");
  const float* __restrict__ src_in = q.src_in;
  float* __restrict__ src_out = q.src_out;
  const float* __restrict__ tgt = q.tgt;
  const float* __restrict__ tn = q.tn;
  const int* __restrict__ cell_start = q.cell_start;
  const float4* __restrict__ sorted = q.sorted;
  const float4* __restrict__ sorted_n = q.sorted_n;
  float* __restrict__ d2prev = q.d2prev;
  const double* __restrict__ partials_in = q.partials_in;
  double* __restrict__ partials_out = q.partials_out;
  int64_t* __restrict__ out_idx = q.out_idx;
  int32_t* __restrict__ tape_idx = q.tape_idx;

  __shared__ alignas(16) IcpSmall sm;
  __shared__ double S[32];
  __shared__ double sub[FS_BLOCK / 32][32];
  __shared__ unsigned long long keys_s[NQ];
  __shared__ int bslot_s[NQ];     // slot of the winning candidate in the binned arrays
  __shared__ float qs[NQ][3];
  __shared__ float qa_s[NQ][8];   // a0..a5, residual of every query of the block (zero when filtered out)
  __shared__ double sub_s[NU][FS_RG][LIN_NV];
  __shared__ int unres_q[NQ], hard_q[NQ];
  __shared__ int unres_n, hard_n;
  // (LMODE 2) points whose list gave no proof: re-searched after the check by 16-lane groups (the 2x2x2 block as one flat
  // candidate list, 4 candidates per lane at 65 per block in a mature map: two round trips instead of the eight a 2-lane
  // group needs inline -- a launch with failing lists is as slow as its slowest group)
  __shared__ int fail_q[LMODE == 2 ? NQ : 1];
  __shared__ int fail_n;
  __shared__ unsigned long long red[FS_BLOCK / GS_WAVE];
  // (LMODE 2) source point and (list centre, radius) of every group, parked across the scalar stage of the prologue: its
  // one-lane float64 code needs the registers, the lanes that wait for it do not
  __shared__ float4 park_s[LMODE == 2 ? 2 * NQ : 1];
  __shared__ int lfail_s[3];   // (LMODE 2) lists of this block that gave no proof / were empty / points without a list
  __shared__ uint8_t rowdone_s[LMODE == 2 ? NQ : 1];   // (LMODE 2) the row of this slot was built by the lane that won its list check
  float4* __restrict__ lq = LISTS ? ql.lq : nullptr;
  uint32_t* __restrict__ ls = LISTS ? ql.ls : nullptr;

  const int64_t n_src = gs_count(n_src_c), n_tgt = gs_count(q.n_tgt);
  const int nunits = (int)((n_src + FS_QPB - 1) / FS_QPB);
  // rows the previous kernel produced (already added up to one row by gs_icp_reduce_rows_kernel for large solves)
  const int nrows_in = rows_in_reduced ? 1 : nunits;
  const int u_first = (int)lb * upb, u_last = (u_first + upb < nunits) ? u_first + upb : nunits;
  if (u_first >= nunits && lb != 0) return;  // beyond the actual count (bound-sized grid)
  // lists are read by blocks that serve ONE group of units (the host plans it so whenever it asks for them)
  // (LMODE is a template parameter: one kernel per mode keeps each of them within the register budget)
  constexpr bool verify = LMODE == 2;
  constexpr bool build_all = LMODE == 1;
  constexpr bool NPREF = LMODE == 2;   // the list check also fetches the normal of the likely match
  // the source point of the first slot does not depend on the prologue: issue its load first so that
  // the global-memory latency hides behind the scalar stage
  const int lane = threadIdx.x & (G - 1), slot = threadIdx.x / G;
  float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
  // the first search of a solve has no predecessor; a list check needs none
  const bool bounded = d2prev != nullptr && !(FULL && it == 0) && !LISTS;   // (the list variants scan whole regions)
  float dprev = __builtin_inff();
  float4 lqv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // (verify) list centre and exactness radius of this group's point
  uint32_t sl[LK];                                     // (verify) this lane's slots of the list
  float4 cv[LK];                                       // (verify) the points in those slots
  float4 cn0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // (verify) the normal of the first of them (the list's nearest
                                                       // when it was built: almost always the match again)
  typedef float gs_v4f __attribute__((ext_vector_type(4)));
  gs_v4f stv = {0.0f, 0.0f, 0.0f, 0.0f};             // (verify) this lane's 16 bytes of the state of the previous half
  int st_idx = 0;
  static_assert(sizeof(IcpSmall) % 16 == 0, "state copy");
  const bool st_lane = threadIdx.x >= GS_WAVE && threadIdx.x < GS_WAVE + (int)(sizeof(IcpSmall) / 16);
  if (LMODE == 2) {
    // Everything this variant loads before its prologue is UNCONDITIONAL (clamped addresses, masked afterwards): a load
    // under a branch may not have been issued, so wherever the compiler needs an OLDER load it has to wait for every
    // outstanding one -- and a conditional load next to a zero-initialised register is waited for on the spot.  The
    // copy of the state (the one conditional transfer) therefore goes first.
    // (hand-issued: a DMA into LDS makes the compiler drain the memory queue at every later wait -- it treats the
    // transfer as a flat access that may complete out of order -- and a plain load is sunk to its use, behind the
    // gathers.  The hook below waits for it by count and stores it.)
    // (an opaque copy of the thread index for the state's addresses: 16 x index merged with its uses at the far end of
    // the kernel is what the register allocator would spill -- a store in the memory queue of the prologue)
    st_idx = (int)threadIdx.x - GS_WAVE;
    asm volatile("" : "+v"(st_idx));
    if (st_lane)
      asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(stv) : "v"(reinterpret_cast<const float4*>(q.st_in) + st_idx) : "memory");
    const int64_t s = (int64_t)u_first * FS_QPB + slot;
    const bool vlive = slot / FS_QPB + u_first < u_last && s < n_src;
    const int64_t sc = vlive ? s : 0;   // (source point 0 stands in; masked below)
    p0 = src_in[3 * sc];
    p1 = src_in[3 * sc + 1];
    p2 = src_in[3 * sc + 2];
    lqv = lq[sc];
    const uint32_t* __restrict__ w = ls + GL_SLOTS * sc + LK * lane;
#pragma unroll
    for (int j = 0; j < LK; ++j) sl[j] = w[j];
    // (lanes without a source point carry point 0's values until the hook drops its list; they are not `live` below)
  } else {
#pragma unroll
    for (int j = 0; j < LK; ++j) { sl[j] = ~0u; cv[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    const int64_t s = (int64_t)u_first * FS_QPB + slot;
    if (slot / FS_QPB + u_first < u_last && s < n_src) {
      p0 = src_in[3 * s];
      p1 = src_in[3 * s + 1];
      p2 = src_in[3 * s + 2];
      if (bounded) dprev = d2prev[s];
    }
  }

  // the state of the previous half and the grid header are fetched while the partial rows are summed
  // (their latency is off the critical path; the sums' barriers publish sm)
  // (the variant that tries lists first needs the grid for its left-overs only and fetches the header there: twelve
  // registers less across its prologue)
  GsGrid g = {};
  if (LMODE != 2) g = *q.gp;
  // (global -> LDS directly, 16 bytes per lane of the second wave: a copy through registers made that wave wait for
  // its loads before it had even requested the partial rows, and the block waits for its slowest wave)
  if (LMODE != 2 && st_lane) it_load_lds16(reinterpret_cast<const float4*>(q.st_in) + (threadIdx.x - GS_WAVE), &sm);
  // behind the row loads of the prologue: the listed points (the slots have arrived with the source point: same round
  // trip).  A slot is dereferenced only below the capacity of `sorted` (a list is always written by an earlier launch of
  // the SAME solve; the clamp costs one compare and keeps a stale word from faulting).
  const uint32_t nsl = (uint32_t)(q.n_tgt.host < 0x7fffffffll ? q.n_tgt.host : 0x7fffffffll);
  auto hook = [&]() {
    if (LISTS) {
      if (LMODE == 2 && verify) {
        const bool try_list = (slot / FS_QPB + u_first < u_last && (int64_t)u_first * FS_QPB + slot < n_src) &&
                              p0 == p0 && lqv.w > 0.0f;
#pragma unroll
        for (int j = 0; j < LK; ++j) {
          if (!try_list || !(sl[j] < nsl)) sl[j] = ~0u;
          cv[j] = sorted[sl[j] != ~0u ? sl[j] : 0u];   // (unconditional: slot 0 stands in for an empty entry, never looked at)
        }
        // (look-ahead half only: in the first half the four registers do not fit next to its scalar stage)
        if (NPREF && sorted_n) cn0 = sorted_n[sl[0] != ~0u ? sl[0] : 0u];   // (block-uniform: every lane issues it or none)
        if (lane == 0) {
          int slot_p = slot;   // (opaque: merged with the address of qa_s[slot] at the far end of the kernel it would be spilled)
          asm volatile("" : "+v"(slot_p));
          park_s[2 * slot_p] = make_float4(p0, p1, p2, 0.0f);
          park_s[2 * slot_p + 1] = lqv;
          rowdone_s[slot_p] = 0;
        }
      }
      // The barriers of this variant do not drain the memory queue, so the copy of the state (hand-issued before
      // everything else, or a DMA into LDS in the building variant) is waited for by hand: loads complete in the order
      // of issue, and exactly LK (verify) vector-memory instructions -- the unconditional gathers right above -- have
      // been issued since everything else.  The row sums are consumed next anyway, so this wait costs nothing.
      if (LMODE == 2 && verify) {
        if (NPREF && sorted_n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LK + 1) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LK) : "memory");
        if (st_lane) *reinterpret_cast<gs_v4f*>(reinterpret_cast<float4*>(&sm) + st_idx) = stv;
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  };

  // ---- prologue: finish the previous half-iteration (identical in every block)
  if (FULL) {
    double e1 = 0.0;
    if (LISTS) {
      // (unconditionally: under `it > 0` the compiler hoists the head of the hook -- the wait for the source point and
      // the list -- in front of the branch, i.e. in front of the row load.  The sum of a first iteration is not used:
      // its rows are whatever the buffer holds.)
      e1 = icp_sum_col27_hook<FS_BLOCK>(partials_in, nrows_in, reinterpret_cast<double*>(red), hook);
    } else if (it > 0) {
      e1 = icp_sum_col27<FS_BLOCK>(partials_in, nrows_in, reinterpret_cast<double*>(red));
    } else {
      __syncthreads();
    }
    if (tl && threadIdx.x == 0) { tl[8] = wall_clock64(); tl[9] = tl[8]; }   // sums done (no solve in this half)
    if (threadIdx.x < GS_WAVE) {  // scalar stage by wave 0, in place on the LDS copy of the state
      if (it > 0)
        icp_update_math_wave((float)e1, sm, prm,
                             (lb == 0 && it - 1 < GS_ICP_MAX_ITERS) ? q.trace + 12 * (it - 1) : nullptr, (int)threadIdx.x);
      if (threadIdx.x == 0) {
        unres_n = 0;
        hard_n = 0;
        fail_n = 0;
        lfail_s[0] = lfail_s[1] = lfail_s[2] = 0;
      }
    }
  } else {
    if (LISTS) icp_sum_rows_split<FS_BLOCK>(partials_in, nrows_in, S, sub, hook);
    else icp_sum_rows<FS_BLOCK>(partials_in, nrows_in, S, sub);
    if (tl && threadIdx.x == 0) tl[8] = wall_clock64();   // sums done
    if (threadIdx.x < GS_WAVE) {   // 6x6 solve and the exponential of the step across the lanes of wave 0
      gs_solve_spd6_wave(S, sm.damp, sm.xi);
      if (tl && threadIdx.x == 0) tl[9] = wall_clock64();   // solve done
      icp_solve_finish_wave(S, sm, (int)threadIdx.x);
      if (threadIdx.x == 0) {
        if (q.tape_sys && lb == 0) tape_write_sys(q.tape_sys, it, S, sm.damp);
        unres_n = 0;
        hard_n = 0;
        fail_n = 0;
        lfail_s[0] = lfail_s[1] = lfail_s[2] = 0;
      }
    }
  }
  gs_bar<LISTS>();
  if (lb == 0 && threadIdx.x < (int)(sizeof(IcpSmall) / 4))
    reinterpret_cast<float*>(q.st_out)[threadIdx.x] = reinterpret_cast<const float*>(&sm)[threadIdx.x];
  if (tl && threadIdx.x == 0) { tl[4] = wall_clock64(); tl[7] = 0; tl[2] = 0; }
  if (LMODE == 2) g = *q.gp;   // (in flight while the lists are checked; re-scans and the left-over pass need it)

  // (the list variants serve ONE group of units per block -- the host plans them only then -- and say so to the
  // compiler: nothing is carried around a loop)
  int u0 = u_first;
  if (u0 < u_last) do {
    const int64_t s = (int64_t)u0 * FS_QPB + slot;
    const bool live = (u0 + slot / FS_QPB < u_last) && s < n_src;  // this slot holds a source point
    if (!LISTS && u0 != u_first) {
      p0 = p1 = p2 = 0.0f;
      dprev = __builtin_inff();
      if (live) {
        p0 = src_in[3 * s];
        p1 = src_in[3 * s + 1];
        p2 = src_in[3 * s + 2];
        if (bounded) dprev = d2prev[s];
      }
    }
    // ---- search: one source point per G-lane group, pending transform applied to the loaded point.
    // A NaN source point (empty slot of an un-compacted lattice, gs_lattice_source_f32) is skipped: it stays
    // NaN through every transform, is never searched and contributes no row.
    if (LMODE == 2 && live) {   // (parked by this group's first lane: same wave, LDS accesses of a wave are ordered)
      int slot_p = slot;   // (opaque, as where it was parked)
      asm volatile("" : "+v"(slot_p));
      const float4 pp = park_s[2 * slot_p];
      p0 = pp.x; p1 = pp.y; p2 = pp.z;
      lqv = park_s[2 * slot_p + 1];
    }
    if (live && p0 != p0) {
      if (lane == 0) {
        if (FULL) { src_out[3 * s] = p0; src_out[3 * s + 1] = p0; src_out[3 * s + 2] = p0; }
        qs[slot][0] = p0; qs[slot][1] = p0; qs[slot][2] = p0;
        keys_s[slot] = ~0ull;
      }
    } else if (live) {
      const float* T = FULL ? sm.T_step : sm.Tr;
      float qx, qy, qz;
      gs_rigid_fma(T, p0, p1, p2, qx, qy, qz);
      bool done;
      bool refail = false;   // (LMODE 2) the list gave no proof: 16-lane re-search of the 2x2x2 block behind the check
      bool weak = false;     // (list-building launch) the list leaves the neighbour too little room: the cube scans re-make it
      int win;
      unsigned long long key;
      if (LMODE == 2 && verify) {
        // the list: every listed point against the query, the same key order as every other engine
        key = ~0ull;
        int wsl = -1;
        bool first = false;   // this lane's best is its first entry (whose normal it holds)
#pragma unroll
        for (int j = 0; j < LK; ++j) {
          const unsigned long long k2 = sl[j] != ~0u ? grid_key(qx, qy, qz, cv[j]) : ~0ull;
          if (k2 < key) { key = k2; wsl = (int)sl[j]; first = j == 0; }
        }
        const unsigned long long kmin = grid_group_min<G>(key);
        win = (key == kmin && wsl >= 0) ? wsl : -1;
        key = kmin;
        const float bd = __uint_as_float((uint32_t)(key >> 32));   // NaN: empty list
        const float ex = qx - lqv.x, ey = qy - lqv.y, ez = qz - lqv.z;
        const float delta = sqrtf(ex * ex + ey * ey + ez * ez);
        done = lqv.w > 0.0f && sqrtf(bd) + delta < lqv.w * 0.9999f;   // false for NaN
        // the lane that holds the match and its normal builds the Gauss-Newton row right here (the same operations on the
        // same values as the row pass below, which then has nothing to gather for this slot)
        if (NPREF && done && win >= 0 && first && sorted_n) {
          float a[6], res;
          gn_row_pn(qx, qy, qz, cv[0], cn0, a, res);
          const bool keep = (dist_thresh < 0.0f) || (bd < dist_thresh);
#pragma unroll
          for (int i = 0; i < 6; ++i) qa_s[slot][i] = keep ? a[i] : 0.0f;
          qa_s[slot][6] = keep ? res : 0.0f;
          rowdone_s[slot] = 1;
        }
        if (!done) {
          key = ~0ull;
          win = -1;
          // (failure counters: per block in LDS, three global atomics per block below -- thousands of failing groups
          // adding to ONE global word serialise at ~12 ns each, which made a launch with many failures three times as long)
          if (lane == 0) atomicAdd(&lfail_s[lqv.w < 0.0f ? 2 : (lqv.w == 0.0f ? 1 : 0)], 1);
          // No proof from the list: the point is re-searched behind the check by a 16-lane group, which scans the 2x2x2
          // block as one flat candidate list and leaves a new list for where the point is now (round 5; round 4 had the
          // point's own G lanes do it right here: in a mature map the block holds ~65 candidates, eight dependent round
          // trips for two lanes with four gathers in flight, and every block of a launch with failing lists waited for
          // that; the cube scans of the left-over pass, which round 4 tried instead, are slower still).
          // (R < 0: the 2x2x2 stage could not prove this point when it was last tried -- straight to the cube scans)
          refail = lqv.w >= 0.0f;
        }
      } else {
        if (build_all) {
          // the whole 2x2x2 block, every lane remembering its nearest candidates: the list is a by-product of the search
          GlTop<LK> top;
          gl_top_reset<LK>(top);
          float rc2;
          key = grid_search_stage0_top<G, LK>(g, cell_start, sorted, qx, qy, qz, lane, &done, &win, top, &rc2);
          if (done) {
            gl_write_lanes<G, LK>(top, rc2, qx, qy, qz, lane, ls + GL_SLOTS * s, lq + s);
            // A WEAK list: the bound of the 2x2x2 block (half a cell to a cell: 15 - 18 mm) caps the radius, and a source point
            // whose nearest target is 12 - 15 mm away -- its lattice neighbour in the map is a zeroed pixel -- is left with
            // millimetres of room: it loses its proof in every look-ahead of a solve that still moves (5 % of the points of
            // seed 0 / frame 8, each time a re-search pass for its whole block).  Such a point goes through the cube scans
            // below, ONCE: their bound is a whole cell (29 mm), and they leave it a wide list as well.
            if (weak_room > 0.0f) {
              const float out2 = gl_group_minf<G>(top.d[LK]);
              const float R2 = out2 < rc2 ? out2 : rc2;
              const float bdw = __uint_as_float((uint32_t)(key >> 32));
              weak = !(sqrtf(bdw) + weak_room * g.c < sqrtf(R2));
            }
          } else if (lane == 0) lq[s] = make_float4(qx, qy, qz, -1.0f);   // (the cubes below may still give it a list)
        } else {
          // search bound: the previous neighbour of this source point is still a target; the previous query was Tr * p
          // in the look-ahead half (this half: T_step * p) resp. p itself in the first half (this half: Tr * p)
          float rball;
          {
            float ox = p0, oy = p1, oz = p2;
            if (FULL) gs_rigid_fma(sm.Tr, p0, p1, p2, ox, oy, oz);
            const float ex = qx - ox, ey = qy - oy, ez = qz - oz;
            rball = sqrtf(dprev) + sqrtf(ex * ex + ey * ey + ez * ez);  // inf without a predecessor, NaN after a NaN match
          }
          key = grid_search_stage0<G>(g, cell_start, sorted, qx, qy, qz, lane, &done, &win, rball);
        }
      }
      if (win >= 0 || (lane == 0 && key == ~0ull)) bslot_s[slot] = win;  // one writer: the winning lane
      if (build_all && weak_room > 0.0f) {
        // (diagnostics, gs_localize_solve_stats_i64: weak lists, one atomic per wave by its first active lane)
        const unsigned long long wm = __ballot(weak && lane == 0);
        if (wm && __builtin_amdgcn_mbcnt_hi((unsigned)(__builtin_amdgcn_read_exec() >> 32),
                                            __builtin_amdgcn_mbcnt_lo((unsigned)__builtin_amdgcn_read_exec(), 0u)) == 0u)
          atomicAdd(ql.weak_n, (unsigned)__popcll(wm));
      }
      if (lane == 0) {
        if (FULL) {  // the transformed cloud of this iteration
          src_out[3 * s] = qx;
          src_out[3 * s + 1] = qy;
          src_out[3 * s + 2] = qz;
        }
        qs[slot][0] = qx; qs[slot][1] = qy; qs[slot][2] = qz;
        keys_s[slot] = key;
        if (!done || weak) {
          if (LMODE == 2 && refail) fail_q[atomicAdd(&fail_n, 1)] = slot;
          else hard_q[atomicAdd(&hard_n, 1)] = slot;
        }
      }
    }
    __syncthreads();
    if (tl && threadIdx.x == 0 && u0 == u_first) tl[10] = wall_clock64();   // list check / search done
    if (LMODE == 2) {
      const int nf = fail_n;   // block-uniform
      if (tl && threadIdx.x == 0 && u0 == u_first) tl[12] = (unsigned long long)nf;
      // lanes per re-searched point by how many there are (block-uniform): 32 lanes see the ~65 candidates of a mature map
      // in two or three round trips (up to 24 points in one round of groups); beyond that 8 lanes with two gathers in
      // flight each (four or five round trips, 96 points per round: the look-aheads of a solve that wanders lose 50 - 200
      // lists per block, profiles/r05_c_failing_lookahead_timeline.txt; 16 lanes served 48 per round in as many trips)
      auto research = [&](auto fg_tag) {
        constexpr int FG = decltype(fg_tag)::value;
        for (int i = threadIdx.x / FG; i < nf; i += FS_BLOCK / FG) {
          const int hs = fail_q[i], lf = threadIdx.x & (FG - 1);
          const float hx = qs[hs][0], hy = qs[hs][1], hz = qs[hs][2];
          const int64_t sq = (int64_t)u0 * FS_QPB + hs;
          constexpr int KF = 2;   // candidates a lane remembers for the new list (the M nearest of 2 FG)
          GlTop<KF> top;
          gl_top_reset<KF>(top);
          float rc2;
          bool fdone;
          int fwin;
          const unsigned long long fkey = grid_search_stage0_top<FG, KF, (FG >= 16 ? 1 : 2)>(g, cell_start, sorted, hx, hy, hz, lf, &fdone, &fwin, top, &rc2);
          if (fdone) gl_select_write<FG, KF>(top, rc2, hx, hy, hz, lf, LM, ls + GL_SLOTS * sq, lq + sq);
          else if (lf == 0) lq[sq] = make_float4(hx, hy, hz, -1.0f);   // (the cubes below may still give it a list)
          if (fwin >= 0) bslot_s[hs] = fwin;   // one writer: the winning lane
          if (lf == 0) {
            keys_s[hs] = fkey;
            if (!fdone) hard_q[atomicAdd(&hard_n, 1)] = hs;
          }
        }
      };
      if (nf > FS_BLOCK / 32) research(std::integral_constant<int, 8>{});
      else if (nf) research(std::integral_constant<int, 32>{});
      if (nf) {
        __syncthreads();
        if (threadIdx.x == 0) fail_n = 0;
        __syncthreads();
      }
    }
    if (tl && threadIdx.x == 0 && u0 == u_first) tl[11] = wall_clock64();   // failed lists re-searched
    if (LMODE == 2 && threadIdx.x < 3 && ql.lstat) {   // failure counters of this launch (diagnostics)
      const int hl = 2 * it + (FULL ? 0 : 1);         // launch index within the solve
      const int c = lfail_s[threadIdx.x];
      if (c && hl < GL_STAT_LAUNCHES) atomicAdd(ql.lstat + threadIdx.x * GL_STAT_LAUNCHES + hl, c);
    }
    // ---- the few queries the 2x2x2 stage did not resolve (neighbour farther than ~half a cell): Chebyshev shells
    // by groups of FS_HG lanes, so that they do not hold up the waves of the common case
    const int nh = hard_n;  // block-uniform
    // wide lists of hard queries (gs_knn.h; IcpHalfWide): kept by the variants with ordinary lists only -- the plain variants
    // (the first three launches of a solve) are at their scalar-register limit, where two more pointers spill scalars into
    // vector registers and those to memory; the pointers are read here, where the rare path starts, not at the top of the
    // kernel
    constexpr bool WL = LISTS;
    float4* __restrict__ wl_cq = WL ? qw.cq : nullptr;
    uint32_t* __restrict__ wl_c = WL ? qw.c : nullptr;
    const bool wl_on = WL && wl_cq != nullptr;
    for (int i = threadIdx.x / FS_HG; i < nh; i += FS_BLOCK / FS_HG) {
      const int hs = hard_q[i] & FS_HQ_SLOT, l16 = threadIdx.x & (FS_HG - 1);
      const float hx = qs[hs][0], hy = qs[hs][1], hz = qs[hs][2];
      const int64_t sq = (int64_t)u0 * FS_QPB + hs;   // the query's source point
      bool done = false, listed = false;
      int win = -1;
      unsigned long long key = keys_s[hs];
      if (WL && wl_on) {   // the wide list an earlier launch of this solve left for the point, if any
        const float4 c0R = wl_cq[sq];
        if (c0R.w > 0.0f) {   // (group-uniform)
          const unsigned long long kl = wide_list_search<FS_HG>(c0R, wl_c + GS_FAR_SLOTS * sq, sorted, hx, hy, hz, l16, &done, &win);
          if (done) { key = kl; listed = true; }
          else win = -1;
        }
      }
      constexpr int KH = 2;   // candidates a lane of the 16-lane group remembers for the new list
      GlTop<KH> top;
      float rc2 = 0.0f;
      if (!done) {
        if (LISTS) key = grid_search_rings_top<FS_HG, KH>(g, cell_start, sorted, hx, hy, hz, l16, key, &done, &win, FS_HARD_RINGS, top, &rc2);
        else key = grid_search_rings<FS_HG>(g, cell_start, sorted, hx, hy, hz, l16, key, &done, &win, FS_HARD_RINGS);
      }
      // (list variants) the scan that served the point leaves its list; what only the brute-force pass can serve keeps none
      if (LISTS && !(WL && listed)) {   // (a point its wide list served keeps what it has: no ordinary list, R < 0)
        if (done) {
          // (whatever the lanes remember of the proving cube is the point's wide list from now on)
          if (WL && wl_on) far_write_from_top<FS_HG, KH>(top, rc2, hx, hy, hz, l16, wl_c + GS_FAR_SLOTS * sq, wl_cq + sq);
          gl_select_write<FS_HG, KH>(top, rc2, hx, hy, hz, l16, LM, ls + GL_SLOTS * sq, lq + sq);
        } else if (l16 == 0) lq[sq] = make_float4(hx, hy, hz, -1.0f);
      }
      if (win >= 0) bslot_s[hs] = win;  // a candidate of the list / the cubes beat the 2x2x2 stage
      if (l16 == 0) {
        keys_s[hs] = key;
        if (!done) unres_q[atomicAdd(&unres_n, 1)] = hs;
      }
    }
    if (nh) {
      __syncthreads();
      if (threadIdx.x == 0) hard_n = 0;
      __syncthreads();
    }
    if (tl && threadIdx.x == 0 && u0 == u_first) { tl[5] = wall_clock64(); tl[2] += (unsigned long long)nh; }
    const int nun = unres_n;  // block-uniform
    if (tl && threadIdx.x == 0) { tl[7] += (unsigned long long)nun; if (u0 == u_first) tl[6] = wall_clock64(); }
    // FS_BQ queries per pass over the binned targets; with wide lists the pass also leaves the lists of its queries
    constexpr int BQL = 2;   // (two queries per list-leaving pass: four cost the 4-lane look-ahead variant a spill; such a pass
                             // now happens once per solve and far point, not once per launch)
    if (WL && wl_on) {   // (block-uniform)
      for (int u = 0; u < nun; u += BQL)
        block_brute_min_list_multi<FS_BLOCK, BQL>(qs, unres_q + u, nun - u < BQL ? nun - u : BQL, sorted, cell_start[g.ncell],
                                                  keys_s, bslot_s, (int64_t)u0 * FS_QPB, wl_cq, wl_c);
    } else {
      for (int u = 0; u < nun; u += FS_BQ)
        block_brute_min_sorted_multi<FS_BLOCK, FS_BQ>(qs, unres_q + u, nun - u < FS_BQ ? nun - u : FS_BQ, sorted,
                                                      cell_start[g.ncell], keys_s, bslot_s);
    }
    if (nun) {
      __syncthreads();
      __syncthreads();   // (a second barrier, from when a pass stood between the two: kept with the instruction text, as FS_HQ_SLOT)
      if (threadIdx.x == 0) unres_n = 0;
      __syncthreads();
    }

    // ---- Gauss-Newton row of every query: its own group's first lane gathers the match and leaves [a, res] in LDS
    if (lane == 0) {
      // (list variants: the index of the source point is formed again here; kept from the top of the kernel it is the
      // one value the register allocator spills -- the opaque copy keeps the compiler from merging the two)
      int u0r = u0;
      if (LISTS) asm volatile("" : "+v"(u0r));   // (a vector register: the unit index is a quotient, i.e. vector arithmetic)
      const int64_t s = LISTS ? (int64_t)u0r * FS_QPB + slot : (int64_t)u0 * FS_QPB + slot;
      float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, res = 0.0f;
      bool rowdone = false;
      if (live && qs[slot][0] != qs[slot][0]) {  // skipped (NaN) source point
        if (FULL && out_idx) out_idx[s] = -1;
        if (tape_idx) tape_idx[s] = -1;
      } else if (live) {
        const unsigned long long bb = keys_s[slot];
        if (d2prev) d2prev[s] = __uint_as_float((uint32_t)(bb >> 32));   // NaN bits when nothing was found
        int64_t j = (int64_t)(bb & 0xffffffffull);
        if (j >= n_tgt) j = 0;  // only when every distance was NaN
        const float d2 = __uint_as_float((uint32_t)(bb >> 32));
        const bool keep = (dist_thresh < 0.0f) || (d2 < dist_thresh);
        const int bsl = bslot_s[slot];
        if (NPREF && rowdone_s[slot]) rowdone = true;   // (built by the lane that won the list check)
        else if (sorted_n && bsl >= 0 && bb != ~0ull)   // matched point and normal from the binned copies (same bits)
          gn_row_pn(qs[slot][0], qs[slot][1], qs[slot][2], sorted[bsl], sorted_n[bsl], a, res);
        else
          gn_row(qs[slot][0], qs[slot][1], qs[slot][2], tgt, tn, j, a, res);
        if (FULL && out_idx) out_idx[s] = j;
        if (tape_idx) tape_idx[s] = keep ? (int32_t)j : -1;
        if (!keep) {
#pragma unroll
          for (int i = 0; i < 6; ++i) a[i] = 0.0f;
          res = 0.0f;
        }
      }
      if (!rowdone) {
#pragma unroll
        for (int i = 0; i < 6; ++i) qa_s[slot][i] = a[i];
        qa_s[slot][6] = res;
      }
    }
    __syncthreads();
    if (!FULL) {  // residual only: per unit the wave-sum tree over its 96 values (64 + 32), then the two wave sums
      double* red2 = reinterpret_cast<double*>(red);
      const int wave = threadIdx.x / GS_WAVE, wl = threadIdx.x & (GS_WAVE - 1);
      if (wave < 2 * NU) {
        const int r = (wave & 1) * GS_WAVE + wl;   // row within the unit
        double rr = 0.0;
        if (r < FS_QPB) {
          const float res = qa_s[(wave >> 1) * FS_QPB + r][6];
          rr = (double)res * (double)res;
        }
        const double sum = gs_wave_sum_f64(rr);
        if (wl == 0) red2[wave] = sum;
      }
      __syncthreads();
      if (threadIdx.x < NU && u0 + (int)threadIdx.x < u_last)
        partials_out[(int64_t)(u0 + threadIdx.x) * LIN_NV + 27] = red2[2 * threadIdx.x] + red2[2 * threadIdx.x + 1];
      __syncthreads();
      continue;
    }
    // FS_QPB rows x 28 values per unit: FS_RG groups of 28 threads add the products of 4 rows each, then 28
    // threads add the sub-sums, always in index order.
    for (int w = threadIdx.x; w < NU * FS_RG * LIN_NV; w += FS_BLOCK) {
      const int i = w % LIN_NV, part = (w / LIN_NV) % FS_RG, un = w / (LIN_NV * FS_RG);
      const int ia = fs_pa(i), ib = fs_pb(i);
      const float* r0 = qa_s[un * FS_QPB + FS_RPG * part];
      double t = (double)r0[ia] * (double)r0[ib];
#pragma unroll
      for (int u = 1; u < FS_RPG; ++u) t += (double)r0[8 * u + ia] * (double)r0[8 * u + ib];
      sub_s[un][part][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < NU * LIN_NV) {
      const int i = threadIdx.x % LIN_NV, un = threadIdx.x / LIN_NV;
      if (u0 + un < u_last) {
        double t = sub_s[un][0][i];
#pragma unroll
        for (int k = 1; k < FS_RG; ++k) t += sub_s[un][k][i];
        partials_out[(int64_t)(u0 + un) * LIN_NV + i] = t;
      }
    }
    __syncthreads();
  } while (!LISTS && (u0 += NU) < u_last);
}

// Batched: block b works for sequence b % B (with B = 8 a sequence lives on one XCD: its binned targets, cell table
// and partial rows stay in that XCD's L2) as that sequence's block b / B; when B divides 8 the 8 / B XCDs of a
// sequence each own a contiguous range of its query rows.
struct IcpHalfBatch {
  int B;
  int upb;  // row units per block
  float weak_room;   // (list-building launch) cells of room between a point's neighbour and the radius of its list below which
                     // the list is re-made by the cube scans (0: never)
  unsigned long long* timeline;  // debugging aid (GRADSLAM_HIP_ICP_TIMELINE): per block [start, end, hw id, xcc id]
  IcpHalfSeq s[GS_MAX_BATCH];
  IcpHalfLists l[GS_MAX_BATCH];   // (read by the list variants only)
  IcpHalfWide w[GS_MAX_BATCH];    // (read in the left-over pass of the list variants only)
};
template <bool FULL, int G, int LMODE>
__global__ void __launch_bounds__(FS_BLOCK, 6) gs_icp_half_batch_kernel(const IcpHalfBatch hb, GsCount n_src_c,
                                                                        float dist_thresh, gs_icp_params prm, int it,
                                                                        int rows_in_reduced) {
  const unsigned B = (unsigned)hb.B, blk = blockIdx.x / B, nblk = gridDim.x / B;
  const unsigned X = (GS_XCDS % B == 0) ? GS_XCDS / B : 1u;
#ifdef GS_ICP_TIMELINE
  unsigned long long t0 = 0;
  if (hb.timeline && threadIdx.x == 0) t0 = wall_clock64();
#endif
  icp_half_body<FULL, G, LMODE>(hb.s[blockIdx.x % B], hb.l[blockIdx.x % B], hb.w[blockIdx.x % B], n_src_c, dist_thresh, prm, it, rows_in_reduced,
                                gs_xcd_block(blk, nblk, X), hb.upb,
                                hb.timeline ? hb.timeline + 72 * (size_t)blockIdx.x : nullptr, hb.weak_room);
#ifdef GS_ICP_TIMELINE
  if (hb.timeline && threadIdx.x == 0) {
    unsigned long long* r = hb.timeline + 72 * (size_t)blockIdx.x;
    r[0] = t0;
    r[1] = wall_clock64();
  }
#endif
}

static size_t icp_rows(int64_t n_src) { return (size_t)gs_ceil_div(n_src, FS_QPB); }  // >= ceil(n_src / LIN_BLOCK)

// What the host asks of a device, once per device: its CU count.
struct IcpDevice { int cus = 256; };
static IcpDevice icp_device() {
  constexpr int MAX_DEV = 64;
  static IcpDevice facts[MAX_DEV]; static std::once_flag asked[MAX_DEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return IcpDevice{};
  std::call_once(asked[dev], [dev] {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) facts[dev].cus = v;
  });
  return facts[dev];
}

// Launch geometry of a half-iteration: lanes per query G, blocks per sequence nb and row units per block upb.
// Every sequence of the batch gets an equal share of the blocks; the largest G whose blocks all fit that share wins
// (more lanes per query = shorter searches, but only while every query of the sequence is in flight at once); if not
// even G = 2 fits, blocks walk several unit groups.  The share is ONE block per CU when some G fits it (round 6: every
// block pays the prologue -- row sums, float64 scalar stage -- and two of them on a CU pay it in each other's way:
// 4 lanes instead of 8 at two sequences per GPU is +11 %, 2 instead of 4 at four sequences +6 %, same bits), two per CU
// otherwise (8 sequences of 640x480: 400 blocks at 2 lanes per point).
// GRADSLAM_HIP_ICP_LANES = 2 | 4 | 8 forces G, GRADSLAM_HIP_ICP_BLOCKS_PER_CU the share (A/B runs: the results do not
// depend on either).
struct IcpHalfPlan { int G, nb, upb; };
static IcpHalfPlan icp_half_plan(const GsEnv& env, int cus, int64_t n_src, int B) {
  constexpr int g_max = 8;   // the most lanes per query a variant exists for
  const int forced = env.icp_lanes;
  const int nunits = (int)icp_rows(n_src);
  int share = env.icp_blocks_per_cu;   // (not set: one block per CU if some G fits that, else two)
  if (share <= 0) {
    const int NU2 = FS_BLOCK / 2 / FS_QPB;   // (the fewest blocks a single group of units per block needs: G = 2)
    share = (nunits + NU2 - 1) / NU2 <= cus / B ? 1 : 2;
  }
  const int budget = (share * cus) / B > 0 ? (share * cus) / B : 1;
  IcpHalfPlan pl{2, 1, 1};
  for (int G = g_max; G >= 2; G >>= 1) {
    const int NU = FS_BLOCK / G / FS_QPB, need = (nunits + NU - 1) / NU;
    if ((forced == 0 && need <= budget) || forced == G || (forced == 0 && G == 2) || (forced > g_max && G == g_max)) {
      pl.G = G;
      pl.nb = need <= budget ? need : budget;
      pl.upb = NU * ((nunits + NU * pl.nb - 1) / (NU * pl.nb));
      pl.nb = (nunits + pl.upb - 1) / pl.upb;
      break;
    }
  }
  return pl;
}

#include "gs_icp_timeline.h"

// lmode: what the launch does with the candidate lists of ordinary queries (icp_half_body; 0 = the variant without them)
template <bool FULL>
static void icp_half_launch(const IcpHalfPlan& pl, IcpHalfBatch& hb, GsCount n_src_c, const gs_icp_params* prm, int it,
                            int rows_in_reduced, hipStream_t st, int lmode = 0) {
  hb.upb = pl.upb;
  hb.timeline = icp_tl_arm(FULL, hb.B * pl.nb, it, prm->numiters, st);
  const dim3 grid((unsigned)(hb.B * pl.nb)), block(FS_BLOCK);
#define GS_HALF_LAUNCH(G_, LMODE_)                                                                                     \
  hipLaunchKernelGGL((gs_icp_half_batch_kernel<FULL, G_, LMODE_>), grid, block, 0, st, hb, n_src_c, prm->dist_thresh,  \
                     *prm, it, rows_in_reduced)
#define GS_HALF_LAUNCH_L(G_)                                                 \
  do {                                                                       \
    if (lmode == 2) GS_HALF_LAUNCH(G_, 2);                                   \
    else if (lmode == 1) GS_HALF_LAUNCH(G_, 1);                              \
    else GS_HALF_LAUNCH(G_, 0);                                              \
  } while (0)
  if (pl.G == 8) GS_HALF_LAUNCH_L(8);
  else if (pl.G == 4) GS_HALF_LAUNCH_L(4);
  else GS_HALF_LAUNCH_L(2);
#undef GS_HALF_LAUNCH_L
#undef GS_HALF_LAUNCH
  if (hb.timeline && !FULL) icp_tl_dump(hb, pl, lmode, st);   // (synchronous: both launches' block records)
  hb.timeline = nullptr;
}

// Large solves (more rows than FS_REDUCE_ROWS): every block of the next kernel adding up all rows is
// O(rows^2) L2 traffic.  One extra launch of a block per sequence adds them up once, in the same order, into a one-row
// buffer.  The threshold sits above the 815 rows of a 1296x968 frame at dsratio 4: there the 20 extra launches per
// solve cost more than the 182 KB of rows per block (measured 2 % of the frame).
constexpr int FS_REDUCE_ROWS = 1024;
struct IcpRowsBatch {
  int B;
  const double* in[GS_MAX_BATCH];
  double* out[GS_MAX_BATCH];
};
__global__ void __launch_bounds__(FS_BLOCK) gs_icp_reduce_rows_batch_kernel(const IcpRowsBatch rb, GsCount n_src_c) {
  __shared__ double S[32];
  __shared__ double sub[FS_BLOCK / 32][32];
  const int nrows = (int)((gs_count(n_src_c) + FS_QPB - 1) / FS_QPB);
  icp_sum_rows<FS_BLOCK>(rb.in[blockIdx.x], nrows, S, sub);
  if (threadIdx.x < LIN_NV) rb.out[blockIdx.x][threadIdx.x] = S[threadIdx.x];
}

// After the last look-ahead: final LM / gradLM update and the (composed) result.
struct IcpFinishBatch {
  int B;
  const double* partials_in[GS_MAX_BATCH];
  GsIcpState* st[GS_MAX_BATCH];
  const float* compose16[GS_MAX_BATCH];
  float* out_T16[GS_MAX_BATCH];
};
__global__ void __launch_bounds__(FS_BLOCK) gs_icp_finish_batch_kernel(const IcpFinishBatch fb, GsCount n_src_c, int buf,
                                                                       gs_icp_params prm) {
  __shared__ double red[FS_BLOCK / GS_WAVE];
  const int b = blockIdx.x;
  const int nrows_in = (int)((gs_count(n_src_c) + FS_QPB - 1) / FS_QPB);
  const double e1 = icp_sum_col27<FS_BLOCK>(fb.partials_in[b], nrows_in, red);
  if (threadIdx.x != 0) return;
  GsIcpState* st = fb.st[b];
  IcpSmall sm = st->s[buf];
  const int it = prm.numiters - 1;
  icp_update_math((float)e1, sm, prm, it < GS_ICP_MAX_ITERS ? st->trace + 12 * it : nullptr);
  st->s[buf ^ 1] = sm;
  icp_write_result(sm, fb.compose16[b], fb.out_T16[b]);
}

// ---------------------------------------------------------------- brute-force path ------
constexpr int LIN_BLOCK = 256;
constexpr int SUM_BLOCK = 1024;

// Reads the KNN result of every source point (and re-arms best[] for the next search), builds
// its row and reduces the normal equations.  FULL = false: residual only (look-ahead).
template <bool FULL>
__global__ void __launch_bounds__(LIN_BLOCK) gs_icp_linearize_kernel(
    const float* __restrict__ src, const float* __restrict__ Tapply, int64_t n_src,
    const float* __restrict__ tgt, const float* __restrict__ tn, int64_t n_tgt,
    unsigned long long* __restrict__ best, float dist_thresh, double* __restrict__ partials,
    int64_t* __restrict__ out_idx, int32_t* __restrict__ tape_idx) {
  __shared__ double red[LIN_BLOCK / GS_WAVE][LIN_NV];
  const int64_t s = (int64_t)blockIdx.x * LIN_BLOCK + threadIdx.x;
  double v[LIN_NV];
#pragma unroll
  for (int i = 0; i < LIN_NV; ++i) v[i] = 0.0;
  if (s < n_src) {
    const unsigned long long bb = best[s];
    best[s] = ~0ull;
    int64_t j = (int64_t)(bb & 0xffffffffull);
    if (j >= n_tgt) j = 0;  // (never taken behind the brute-force kernel: it wrote (+inf, 0), see gs_knn_unpack_kernel)
    const float d2 = __uint_as_float((uint32_t)(bb >> 32));
    const bool keep = (dist_thresh < 0.0f) || (d2 < dist_thresh);
    float p0 = src[3 * s], p1 = src[3 * s + 1], p2 = src[3 * s + 2];
    if (Tapply) {
      float T[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) T[i] = Tapply[i];
      float q0, q1, q2;
      gs_rigid_fma(T, p0, p1, p2, q0, q1, q2);
      p0 = q0; p1 = q1; p2 = q2;
    }
    float a[6], r;
    gn_row(p0, p1, p2, tgt, tn, j, a, r);
    if (FULL && out_idx) out_idx[s] = j;
    if (tape_idx) tape_idx[s] = keep ? (int32_t)j : -1;
    if (keep) {
      if (FULL) {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int k = i; k < 6; ++k) v[q++] = (double)a[i] * (double)a[k];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[21 + i] = (double)a[i] * (double)r;
      }
      v[27] = (double)r * (double)r;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = FULL ? 0 : 27; i < LIN_NV; ++i) {
    const double sum = gs_wave_sum_f64(v[i]);
    if (lane == 0) red[wave][i] = sum;
  }
  __syncthreads();
  if (threadIdx.x < LIN_NV && (FULL || threadIdx.x == 27)) {
    const int i = threadIdx.x;
    partials[(int64_t)blockIdx.x * LIN_NV + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

__global__ void __launch_bounds__(SUM_BLOCK) gs_icp_solve_kernel(const double* __restrict__ partials, int nrows,
                                                                 GsIcpState* __restrict__ st, int it,
                                                                 float* __restrict__ tape_sys) {
  __shared__ double S[32];
  __shared__ double sub[SUM_BLOCK / 32][32];
  __shared__ float xi_s[8];
  icp_sum_rows<SUM_BLOCK>(partials, nrows, S, sub);
  if (threadIdx.x >= GS_WAVE) return;
  gs_solve_spd6_wave(S, st->s[0].damp, xi_s);  // same wave: LDS accesses of a wave are ordered
  __builtin_amdgcn_wave_barrier();
  if (threadIdx.x != 0) return;
  IcpSmall sm = st->s[0];
  if (tape_sys) tape_write_sys(tape_sys, it, S, sm.damp);
  for (int k = 0; k < 6; ++k) sm.xi[k] = xi_s[k];
  icp_solve_finish(S, sm);
  st->s[0] = sm;
}

__global__ void __launch_bounds__(SUM_BLOCK) gs_icp_update_kernel(const double* __restrict__ partials, int nrows,
                                                                  GsIcpState* __restrict__ st, gs_icp_params prm,
                                                                  int it, const float* __restrict__ compose16,
                                                                  float* __restrict__ out_T16) {
  __shared__ double red[SUM_BLOCK / GS_WAVE];
  const double e1 = icp_sum_col27<SUM_BLOCK>(partials, nrows, red);
  if (threadIdx.x != 0) return;
  IcpSmall sm = st->s[0];
  icp_update_math((float)e1, sm, prm, it < GS_ICP_MAX_ITERS ? st->trace + 12 * it : nullptr);
  st->s[0] = sm;
  if (it == prm.numiters - 1) icp_write_result(sm, compose16, out_T16);
}

// ---------------------------------------------------------------- host side ------------
// the state a solve starts from (both buffers): nothing accumulated, the initial transform pending
GS_DEV IcpSmall icp_state_init(const float* __restrict__ init16, float damp) {
  IcpSmall sm;
  for (int i = 0; i < 16; ++i) {
    sm.T_total[i] = init16[i];
    sm.T_step[i] = init16[i];  // the first search applies the initial transform
    sm.Tr[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  }
  for (int i = 0; i < 8; ++i) sm.xi[i] = 0.0f;
  sm.damp = damp;
  sm.err = 0.0f;
  sm.pad[0] = sm.pad[1] = 0.0f;
  return sm;
}
__global__ void gs_icp_init_kernel(GsIcpState* __restrict__ st, const float* __restrict__ init16, float damp,
                                   int numiters, const float* __restrict__ compose16, float* __restrict__ out_T16) {
  if (threadIdx.x != 0) return;
  const IcpSmall sm = icp_state_init(init16, damp);
  st->s[0] = sm;
  st->s[1] = sm;
  if (numiters == 0) icp_write_result(sm, compose16, out_T16);  // degenerate: the (composed) initial transform
}

template <class T>
static T* gs_at(void* base, size_t offset) { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + offset); }
struct GsTake { size_t end = 0; size_t operator()(size_t n) { end += n; return end - n; } };   // consecutive byte ranges

// Scratch of one solve as byte offsets from its start: state | rowred | best | srcA | srcB | partials[2] | grid | spare.
// The ONE description of it: gs_icp_scratch_bytes returns its total, icp_carve applies it to a base pointer.
constexpr int ICP_ROWRED_DOUBLES = 32;
constexpr int ICP_WEAK_WORD = 3;   // the weak-list counter: this 32-bit word of the padding behind the one row of rowred
struct IcpLayout { size_t state, rowred, weak_n, best, srcA, srcB, partials[2], grid, total; };
static IcpLayout icp_layout(int64_t n_src, int64_t n_tgt) {
  GsTake take;
  IcpLayout L;
  L.state = take(gs_align(sizeof(GsIcpState)));
  L.rowred = take(gs_align(sizeof(double) * ICP_ROWRED_DOUBLES));
  L.weak_n = L.rowred + sizeof(double) * LIN_NV + 4 * ICP_WEAK_WORD;
  static_assert(8 * ICP_ROWRED_DOUBLES >= 8 * LIN_NV + 4 * (ICP_WEAK_WORD + 1), "the weak-list counter does not fit behind rowred + LIN_NV");
  L.best = take(gs_align(8 * (size_t)n_src));
  L.srcA = take(gs_align(12 * (size_t)n_src)); L.srcB = take(gs_align(12 * (size_t)n_src));
  for (int k = 0; k < 2; ++k) L.partials[k] = take(gs_align(sizeof(double) * LIN_NV * icp_rows(n_src)));
  L.grid = take(gs_knn_grid_scratch_bytes(n_src, n_tgt));
  L.total = take.end + 4096;
  return L;
}
struct IcpScratch {
  GsIcpState* state;
  double* rowred;  // one partial row (large solves: gs_icp_reduce_rows_batch_kernel)
  unsigned* weak_n;  // weak lists the list-building launch flagged (GRADSLAM_HIP_ICP_WEAK_ROOM; gs_localize_solve_stats_i64)
  unsigned long long* best; float *srcA, *srcB;
  double* partials[2]; void* grid;
};
static IcpScratch icp_carve(void* p, const IcpLayout& L) {
  return IcpScratch{gs_at<GsIcpState>(p, L.state), gs_at<double>(p, L.rowred), gs_at<unsigned>(p, L.weak_n),
                    gs_at<unsigned long long>(p, L.best), gs_at<float>(p, L.srcA), gs_at<float>(p, L.srcB),
                    {gs_at<double>(p, L.partials[0]), gs_at<double>(p, L.partials[1])}, gs_at<void>(p, L.grid)};
}

extern "C" int64_t gs_icp_scratch_bytes(int64_t n_src, int64_t n_tgt) { return (int64_t)icp_layout(n_src < 1 ? 1 : n_src, n_tgt).total; }

// the per-iteration trace [err, new_err, damp_after, sigmoid, xi(6), 0, 0] completes the tape
static int icp_tape_finish(void* tape, const GsIcpState* state, int64_t n_src, int numiters, hipStream_t st) {
  GsIcpTape t = gs_icp_tape_carve(tape, n_src, numiters);
  if (numiters > 0)
    GS_HIP(hipMemcpyAsync(t.trace, state->trace, sizeof(float) * 12 * (size_t)numiters, hipMemcpyDeviceToDevice, st));
  return GS_OK;
}

// Algorithmic (compulsory) bytes of the 2 x numiters half-iteration kernels of one solve: per slot of
// the source array 12 B read; per searched query 12 B written (first half: the transformed cloud) + 24 B matched target
// point and normal; one partial row (28 / 1 doubles) per FS_QPB queries; one 16 B pass over the binned targets
// per half-iteration.  Cell-bound look-ups and candidate gathers beyond that are traffic, not compulsory bytes.
static double icp_alg_bytes(int numiters, int64_t n_slots, int64_t n_queries, int64_t n_binned) {
  const double rows = (double)gs_ceil_div(n_slots, FS_QPB);
  const double full = 12.0 * n_slots + 36.0 * n_queries + 8.0 * LIN_NV * rows + 16.0 * n_binned;
  const double look = 12.0 * n_slots + 24.0 * n_queries + 8.0 * rows + 16.0 * n_binned;
  return (double)numiters * (full + look);
}

// ---------------------------------------------------------------- batched localisation -----
// ICPSLAM._localize (slam/icpslam.py:238-247) for B independent sequences in ONE chain of launches: every kernel
// below runs for all sequences at once (block b -> sequence b % B), so the dependent-launch floor of the 2 x numiters
// half-iteration kernels, which bounds a single 640x480 sequence, is paid once per B frames and the chip
// is filled by B x the blocks.  Per sequence the arithmetic is that of gs_lattice_source_f32 + gs_project_map_dc_f32
// + gs_icp_map_dc_f32, bit for bit (same device functions).
struct LocSeq {
  const float* vertex;   // may be NULL: the local vertex of a lattice pixel is fm_vertex of its depth (the same bits)
  const float* K16;      // read only then
  const float* depth;
  const float* pose16;   // previous pose: lattice transform, projection and the composed result
  float* lattice;        // [n_lat][3] ICP source (NaN = no depth)
  GsIcpState* state;
  float* out_pose16;
  char* clear_ptr;       // grid scratch bytes that must be zero before the build
  int64_t* n_valid;      // number of lattice slots with depth (profiling / roofline accounting)
  int* lstat;            // [3 * GL_STAT_LAUNCHES] failure counters of the ordinary candidate lists, zeroed here
  float4* wl_cq;         // [n_lat] wide lists of hard queries: every radius cleared here (NULL: none kept)
  unsigned* weak_n;      // the weak-list counter of the solve (IcpScratch::weak_n), zeroed here
};
struct LocBatch {
  int B, W, ds, Wl;
  int64_t n_lat;
  size_t clear_bytes;
  float damp;
  int numiters;
  int count_valid;       // profile passes: count the lattice slots with depth
  LocSeq s[GS_MAX_BATCH];
};
constexpr int LP_CLEAR_ITEMS = 8;  // 16-byte stores per thread of a clearing block (32 KB per block)

// lattice source (gs_lattice_source_kernel) + solver state (gs_icp_init_kernel) + zeroing of the grid scratch
GS_DEV void loc_prep_block(const LocBatch& lb, const unsigned bid, const unsigned nb_lat) {
  const LocSeq& q = lb.s[bid % lb.B];
  const unsigned blk = bid / lb.B;
  if (blk < nb_lat) {
    const int64_t e = (int64_t)blk * 256 + threadIdx.x;
    int valid = 0;
    if (e < lb.n_lat) {
      const int64_t p = (e / lb.Wl) * lb.ds * (int64_t)lb.W + (e % lb.Wl) * lb.ds;
      float g0 = __builtin_nanf(""), g1 = g0, g2 = g0;
      const float d = q.depth[p];
      if (d > 0.0f) {
        float T[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = q.pose16[i];
        float v0, v1, v2;
        if (q.vertex) {
          v0 = q.vertex[3 * p]; v1 = q.vertex[3 * p + 1]; v2 = q.vertex[3 * p + 2];
        } else {
          fm_vertex(d, (int)(e / lb.Wl) * lb.ds, (int)(e % lb.Wl) * lb.ds, gs_kinv(q.K16), v0, v1, v2);
        }
        gs_rigid_fma(T, v0, v1, v2, g0, g1, g2);
        valid = 1;
      }
      q.lattice[3 * e] = g0; q.lattice[3 * e + 1] = g1; q.lattice[3 * e + 2] = g2;
      if (q.wl_cq) q.wl_cq[e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // (no wide list of an earlier frame is ever read)
    }
    const unsigned long long m = lb.count_valid ? __ballot(valid) : 0ull;
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(q.n_valid), (unsigned long long)__popcll(m));
    if (blk == 0 && threadIdx.x == 0) {  // gs_icp_init_kernel with init = identity
      float id[16];
      for (int i = 0; i < 16; ++i) id[i] = (i % 5 == 0) ? 1.0f : 0.0f;
      const IcpSmall sm = icp_state_init(id, lb.damp);
      q.state->s[0] = sm;
      q.state->s[1] = sm;
      if (q.lstat)
        for (int i = 0; i < 3 * GL_STAT_LAUNCHES; ++i) q.lstat[i] = 0;
      if (q.weak_n) *q.weak_n = 0u;
      if (lb.numiters == 0) icp_write_result(sm, q.pose16, q.out_pose16);
    }
    return;
  }
  float4* dst = reinterpret_cast<float4*>(q.clear_ptr);
  const size_t n16 = lb.clear_bytes / 16;
  const size_t base = (size_t)(blk - nb_lat) * 256 * LP_CLEAR_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LP_CLEAR_ITEMS; ++u) {
    const size_t i = base + (size_t)u * 256;
    if (i < n16) dst[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}
__global__ void __launch_bounds__(256) gs_loc_prep_kernel(const LocBatch lb, unsigned nb_lat) {
  loc_prep_block(lb, blockIdx.x, nb_lat);
}
// The one-call step clears the grid scratch in its frame-map launch (gs_frame_maps_batch_clear): the lattice blocks
// then have nothing to wait for and share a launch with the first pass of the grid build (projection of the map under
// the previous pose + bounding box + target list), which does not read what they write.
static_assert(GB_BLOCK == 256, "lattice and bbox blocks share a launch");
__global__ void __launch_bounds__(256) gs_loc_prep_bbox_kernel(const LocBatch lb, const GsGridBatch gb, const unsigned nb_lat,
                                                               const float u_hi, const float v_hi) {
  const unsigned n_prep = (unsigned)lb.B * nb_lat;
  if (blockIdx.x < n_prep) loc_prep_block(lb, blockIdx.x, nb_lat);
  else gridb_bbox_block(gb, blockIdx.x - n_prep, u_hi, v_hi);
}

static int64_t loc_lattice(int H, int W, int ds) { return (int64_t)((H + ds - 1) / ds) * ((W + ds - 1) / ds); }

// candidate lists of ordinary queries (gs_knn.h: gl_*), behind the ICP scratch of a sequence
struct ListMem {
  float4* lq;      // [n_lat] (position the list was built at, exactness radius; 0: no list, < 0: no list and the 2x2x2
                   // stage cannot prove this point -- cube scans)
  uint32_t* ls;    // [n_lat][GL_SLOTS] slots of `sorted` (~0: empty)
  int* stat;       // [3 * GL_STAT_LAUNCHES] per launch of the solve: lists that failed their proof, points whose list
                   // is empty (nothing fitted), points the 2x2x2 stage cannot prove (no list)
};

// wide lists of hard queries (gs_knn.h), behind the lists of the ordinary ones
struct FarMem {
  uint32_t* c;    // [n_lat][GS_FAR_SLOTS] slots of `sorted`
  float4* cq;     // [n_lat] (position the list was made at, exactness radius; 0: no list)
};

static int64_t loc_rows(const gs_map_view& m) { return m.capacity > m.n_bound ? m.capacity : m.n_bound; }

// Scratch of one sequence of the batched localisation as byte offsets from its start: lattice | n_valid | the solve's
// scratch (IcpLayout sc, counted from `icp`; it holds the grid) | lists of ordinary queries (ListMem) | wide lists of hard
// queries (FarMem).  The ONE description of it: gs_localize_scratch_bytes returns its
// total, loc_carve applies it to a base pointer.  `rows` is the map's CAPACITY (what the scratch was sized for), not the count
// bound of a frame: every pointer then stays where it is from frame to frame while the map grows (the fast path keeps one
// scratch per sequence and checks buffer identity), and the stats exporters, given the capacity, find what the solve left.
struct LocLayout {
  int64_t n_lat, rows;
  IcpLayout sc;
  size_t lattice, n_valid, icp, lq, ls, lstat, far_c, far_cq, total;
};
static LocLayout loc_layout(int64_t n_lat, int64_t rows) {
  GsTake take;
  LocLayout L;
  L.n_lat = n_lat; L.rows = rows > 0 ? rows : 1;
  L.lattice = take(gs_align(12 * (size_t)n_lat));
  L.n_valid = take(256);
  L.sc = icp_layout(n_lat, L.rows);
  L.icp = take(L.sc.total);
  L.lq = take(gs_align(16 * (size_t)n_lat));
  L.ls = take(gs_align(4 * GL_SLOTS * (size_t)n_lat));
  L.lstat = take(gs_align(4 * 3 * GL_STAT_LAUNCHES));
  L.far_c = take(gs_align(4 * GS_FAR_SLOTS * (size_t)n_lat));
  L.far_cq = take(gs_align(16 * (size_t)n_lat));
  L.total = take.end;
  return L;
}
// The list variants sum the partial rows with UNCONDITIONAL loads, masked afterwards (icp_sum_col27_hook: row threadIdx.x
// of every thread; icp_sum_rows_split: 24 x 18 rows): FS_BLOCK rows of LIN_NV doubles from the start of a row buffer
// whatever the row count.  What follows the LAST row buffer in the scratch (the grid, the lists; rowred and the first
// buffer have more behind them) must cover that, or the solve keeps no lists.
static bool loc_lists_fit(const LocLayout& L) { return L.total - (L.icp + L.sc.partials[1]) >= sizeof(double) * LIN_NV * FS_BLOCK; }

extern "C" int64_t gs_localize_scratch_bytes(int H, int W, int ds, int64_t n_map_bound) {
  if (H < 1 || W < 1 || ds < 1) return 0;
  return (int64_t)loc_layout(loc_lattice(H, W, ds), n_map_bound).total;
}

struct LocCarve {
  float* lattice; int64_t* n_valid;
  IcpScratch sc; GridMem gm; ListMem lm; FarMem fm;
};
static LocCarve loc_carve(void* p, const LocLayout& L) {
  const IcpScratch sc = icp_carve(gs_at<char>(p, L.icp), L.sc);
  return LocCarve{gs_at<float>(p, L.lattice), gs_at<int64_t>(p, L.n_valid), sc,
                  grid_carve(sc.grid, L.n_lat, L.rows),
                  ListMem{gs_at<float4>(p, L.lq), gs_at<uint32_t>(p, L.ls), gs_at<int>(p, L.lstat)},
                  FarMem{gs_at<uint32_t>(p, L.far_c), gs_at<float4>(p, L.far_cq)}};
}
// (the stats exporters and the one-call step: the scratch of a solve of HxW images at dsratio ds against map_rows rows)
static LocCarve loc_carve_of(const void* scratch, int H, int W, int ds, int64_t map_rows) {
  return loc_carve(const_cast<void*>(scratch), loc_layout(loc_lattice(H, W, ds), map_rows));
}

// Which engines a batched solve runs, decided ONCE, before its first launch (icp_engine_plan: no HIP call in there).
struct IcpEnginePlan {
  bool wide_on, lists_on;   // wide lists of hard queries / candidate lists of ordinary queries
  bool binned_normals;  // the matches' normals come from the binned copy, not from the map
  bool reduce_rows;     // large solves: one extra launch per iteration adds the rows up once (FS_REDUCE_ROWS)
  int lists_from;       // the lists are built behind the look-ahead search of this iteration, tried from the next on
  IcpHalfPlan half;     // geometry of the half-iteration launches
  float weak_room;
  // what a launch does with the ordinary lists (icp_half_body: LMODE): 0 nothing, 1 build them, 2 try them
  int lmode(int it, bool look_ahead) const {
    if (!lists_on || it < lists_from) return 0;
    if (it > lists_from) return 2;
    return look_ahead ? 1 : 0;
  }
};
static IcpEnginePlan icp_engine_plan(const GsEnv& env, const IcpDevice& dev, int B, int64_t n_lat, int numiters,
                                     const LocLayout* layouts) {
  IcpEnginePlan p;
  const int64_t rows = (int64_t)icp_rows(n_lat);
  p.binned_normals = env.icp_binned_normals; p.weak_room = env.icp_weak_room;
  p.lists_from = env.icp_lists_from >= 0 ? env.icp_lists_from : FS_LISTS_FROM;
  p.reduce_rows = rows > FS_REDUCE_ROWS;
  p.wide_on = env.icp_wide && numiters > 0;
  p.half = icp_half_plan(env, dev.cus, n_lat, B);
  // (a block reads the lists of ONE group of row units: solves whose blocks walk several groups keep none)
  p.lists_on = env.icp_lists && p.half.upb * p.half.G * FS_QPB <= FS_BLOCK;
  for (int b = 0; b < B && p.lists_on; ++b) p.lists_on = loc_lists_fit(layouts[b]);
  return p;
}
// the plan of a solve with every engine off (the single solve): two plain launches per iteration
static IcpEnginePlan icp_plain_plan(const IcpHalfPlan& half, int64_t n_src) {
  IcpEnginePlan p{};   // (no lists of any kind, no weak room)
  p.binned_normals = true; p.reduce_rows = icp_rows(n_src) > FS_REDUCE_ROWS;
  p.half = half;
  return p;
}

// Where the solve of one sequence lives, filled once per call: the single solve fills one from its arguments (icp_run),
// the batched localisation one per sequence from its carved scratch (loc_bind).  What a solve does not keep is NULL.
struct IcpSolveView {
  const float* src0;                     // source of the first iteration (later ones: icp_cloud)
  const float *tgt, *tn; GsCount n_tgt;  // targets and their normals
  IcpScratch sc; GridMem gm;
  int64_t* out_idx;                      // (optional) match of every source point in the last iteration
  TapePtrs tape;                         // (optional) forward tape
  IcpHalfLists lists; IcpHalfWide wide;   // (optional) candidate lists: ordinary, wide
  const float* compose16; float* out_T16;
};

// ---- the steps of a chunk: bind, prep + grid build, half-iterations, finish (c[b]: the carved scratch
// of sequence b, v[b]: the view of its solve)
static void loc_bind(const gs_localize_seq* seqs, int B, int H, int W, int ds, const gs_icp_params* prm,
                     const IcpEnginePlan& plan, LocCarve* c, LocBatch& lb, GsGridBatch& gb, IcpSolveView* v) {
  lb.B = gb.B = B; lb.W = gb.W = W; gb.H = H; lb.ds = gb.ds = ds;
  gb.listed = 1;   // the ICP targets are the map rows that project onto the lattice under the previous pose
  lb.Wl = (W + ds - 1) / ds; lb.n_lat = loc_lattice(H, W, ds); lb.damp = prm->damp; lb.numiters = prm->numiters;
  gb.cells_cap = gs_knn_grid_cells_cap(lb.n_lat);
  for (int b = 0; b < B; ++b) {
    const gs_localize_seq& q = seqs[b];
    if (!plan.binned_normals) c[b].gm.sorted_n = nullptr;
    // (the prep launch zeroes the counters of the ordinary lists whether or not this solve keeps such lists)
    lb.s[b] = LocSeq{q.vertex, q.K16, q.depth, q.prev_pose16, c[b].lattice, c[b].sc.state, q.out_pose16,
                     reinterpret_cast<char*>(c[b].gm.g), c[b].n_valid, c[b].lm.stat,
                     plan.wide_on ? c[b].fm.cq : nullptr, c[b].sc.weak_n};
    gb.s[b] = GsGridSeq{q.map.points, GsCount{q.map.n_bound, q.map.n_dev}, nullptr, q.prev_pose16, q.K16,
                        plan.binned_normals ? q.map.normals : nullptr, c[b].gm};
    v[b] = IcpSolveView{c[b].lattice, q.map.points, q.map.normals, GsCount{q.map.n_bound, q.map.n_dev}, c[b].sc, c[b].gm,
                        nullptr, TapePtrs{nullptr, nullptr, nullptr},
                        plan.lists_on ? IcpHalfLists{c[b].lm.lq, c[b].lm.ls, c[b].lm.stat, c[b].sc.weak_n}
                                      : IcpHalfLists{nullptr, nullptr, nullptr, nullptr},
                        plan.wide_on ? IcpHalfWide{c[b].fm.cq, c[b].fm.c} : IcpHalfWide{nullptr, nullptr},
                        q.prev_pose16, q.out_pose16};
  }
  lb.count_valid = g_gs_prof_on ? 1 : 0;
  lb.clear_bytes = gs_knn_grid_clear_bytes(c[0].gm, gb.cells_cap);  // same layout offsets for every sequence
}

// grid_cleared: the caller has zeroed the first gs_knn_grid_clear_bytes() bytes of every sequence's grid scratch
// (loc_carve().gm.g) on the stream already
static int loc_prep(const gs_localize_seq* seqs, const LocBatch& lb, const GsGridBatch& gb, hipStream_t st, bool grid_cleared) {
  const int B = lb.B;
  if (g_gs_prof_on)
    for (int b = 0; b < B; ++b) GS_HIP(hipMemsetAsync(lb.s[b].n_valid, 0, 8, st));
  const unsigned nb_lat = (unsigned)gs_ceil_div(lb.n_lat, 256);
  const unsigned nb_clear = (unsigned)gs_ceil_div((int64_t)(lb.clear_bytes / 16), 256 * LP_CLEAR_ITEMS);
  // lattice 28 B per slot; projection 12 B read per map row (it is not stored: the count and scatter passes walk the list of
  // the rows that passed, which the 16 B per cell below more than cover); cell table
  double bytes = 0.0;
  for (int b = 0; b < B; ++b) bytes += 28.0 * lb.n_lat + 12.0 * seqs[b].map.n_bound + 16.0 * gb.cells_cap;
  GsProf prof(GS_PROF_COMPACT, bytes, st, grid_cleared ? 4 : 5);
  if (grid_cleared) {
    const float u_hi = (float)((double)gb.W - 0.999), v_hi = (float)((double)gb.H - 0.999);   // (as gs_knn_grid_build_batch)
    hipLaunchKernelGGL(gs_loc_prep_bbox_kernel, dim3((unsigned)B * nb_lat + gs_knn_gridb_bbox_blocks(gb)), dim3(256), 0, st,
                       lb, gb, nb_lat, u_hi, v_hi);
    return gs_knn_grid_build_batch(gb, st, true);
  }
  hipLaunchKernelGGL(gs_loc_prep_kernel, dim3((unsigned)B * (nb_lat + nb_clear)), dim3(256), 0, st, lb, nb_lat);
  return gs_knn_grid_build_batch(gb, st);
}

// profile passes only (one sync per sequence): exact counts for the roofline line
static int loc_prof_bytes(int B, const LocCarve* c, int64_t n_lat, int numiters, hipStream_t st, double* bytes) {
  for (int b = 0; b < B; ++b) {
    unsigned hits = 0; int64_t nv = 0;
    GS_HIP(hipMemcpyAsync(&hits, c[b].gm.bbox + 6, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipMemcpyAsync(&nv, c[b].n_valid, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    *bytes += icp_alg_bytes(numiters, n_lat, nv, hits);
  }
  return GS_OK;
}

// what every entry point asks of the solver's parameters: NULL, or what is wrong with them
static const char* icp_params_error(const gs_icp_params* prm) {
  if (!(prm->numiters >= 0 && prm->numiters <= GS_ICP_MAX_ITERS)) return "numiters must be in [0, 1024]";
  return prm->mode == 0 || prm->mode == 1 ? nullptr : "mode must be 0 (ICP) or 1 (gradICP)";
}

// The half-iteration indexing, written once for every client.  A solve of numiters iterations is 2 x numiters
// half-iterations h = 2 * it (first half: search with T_step applied, full normal equations) and h = 2 * it + 1 (look-ahead:
// search with Tr applied, residual only), then the finish at h = 2 * numiters.  State and partial rows are double-buffered
// between consecutive launches: half-iteration h (and the finish) reads the state s[h & 1] and the rows
// partials[(h + 1) & 1] that h - 1 left and writes the others; large solves put one launch in front of a look-ahead that
// adds the rows it reads up to the one row `rowred`.  Iteration `it` reads the cloud of iteration it - 1 (the first one:
// the caller's source) and writes its own, which its look-ahead reads: srcA / srcB in turn, or slot `it` of the tape when
// one is recorded.
struct IcpHalfIo { const double* rows_in; double* rows_out; const IcpSmall* st_in; IcpSmall* st_out; };
static IcpHalfIo icp_half_io(const IcpScratch& sc, int h) {
  return IcpHalfIo{sc.partials[(h + 1) & 1], sc.partials[h & 1], &sc.state->s[h & 1], &sc.state->s[(h + 1) & 1]};
}
static float* icp_cloud(const IcpSolveView& v, int it, int64_t n_src) {
  return v.tape.src ? v.tape.src + (size_t)it * 3 * (size_t)n_src : ((it & 1) ? v.sc.srcB : v.sc.srcA);
}
static int32_t* icp_tape_idx(const IcpSolveView& v, int it, int look_ahead, int64_t n_src) {
  return v.tape.idx ? v.tape.idx + ((size_t)it * 2 + look_ahead) * (size_t)n_src : nullptr;
}

// every iteration of B solves: two launches each (+ the row sums of large solves)
// prof_rows: the row sums get a profile record of their own (the single solve)
static void loc_half_iterations(const IcpSolveView* v, int B, const IcpEnginePlan& plan, GsCount n_src_c,
                                const gs_icp_params* prm, hipStream_t st, bool prof_rows) {
  const int64_t n_src = n_src_c.host;
  IcpHalfBatch hb;
  hb.B = B; hb.weak_room = plan.weak_room;
  for (int b = 0; b < B; ++b) { hb.w[b] = v[b].wide; hb.l[b] = v[b].lists; }
  for (int it = 0; it < prm->numiters; ++it) {
    int h = 2 * it;
    for (int b = 0; b < B; ++b) {
      const IcpSolveView& q = v[b];
      const IcpHalfIo io = icp_half_io(q.sc, h);
      hb.s[b] = IcpHalfSeq{it == 0 ? q.src0 : icp_cloud(q, it - 1, n_src), icp_cloud(q, it, n_src), q.tgt, q.tn, q.n_tgt, q.gm.g,
                           q.gm.cell_start, q.gm.sorted, q.gm.sorted_n, reinterpret_cast<float*>(q.sc.best),
                           io.rows_in, io.rows_out, io.st_in, io.st_out, q.sc.state->trace, q.out_idx,
                           icp_tape_idx(q, it, 0, n_src), nullptr};
    }
    icp_half_launch<true>(plan.half, hb, n_src_c, prm, it, 0, st, plan.lmode(it, false));
    ++h;
    if (plan.reduce_rows) {
      std::optional<GsProf> prof;
      if (prof_rows) prof.emplace(GS_PROF_SOLVE, 1.0, st);
      IcpRowsBatch rb; rb.B = B;
      for (int b = 0; b < B; ++b) { rb.in[b] = icp_half_io(v[b].sc, h).rows_in; rb.out[b] = v[b].sc.rowred; }
      hipLaunchKernelGGL(gs_icp_reduce_rows_batch_kernel, dim3((unsigned)B), dim3(FS_BLOCK), 0, st, rb, n_src_c);
    }
    for (int b = 0; b < B; ++b) {
      const IcpSolveView& q = v[b];
      const IcpHalfIo io = icp_half_io(q.sc, h);
      IcpHalfSeq& u = hb.s[b];
      u.src_in = icp_cloud(q, it, n_src); u.src_out = nullptr;
      u.partials_in = plan.reduce_rows ? q.sc.rowred : io.rows_in; u.partials_out = io.rows_out;
      u.st_in = io.st_in; u.st_out = io.st_out;
      u.out_idx = nullptr; u.tape_idx = icp_tape_idx(q, it, 1, n_src); u.tape_sys = q.tape.sys;
    }
    icp_half_launch<false>(plan.half, hb, n_src_c, prm, it, plan.reduce_rows ? 1 : 0, st, plan.lmode(it, true));
  }
}

// final LM / gradLM update and the composed result
static void loc_finish(const IcpSolveView* v, int B, GsCount n_src_c, const gs_icp_params* prm, hipStream_t st) {
  const int h = 2 * prm->numiters;
  GsProf prof(GS_PROF_SOLVE, 1.0, st);
  IcpFinishBatch fb;
  fb.B = B;
  for (int b = 0; b < B; ++b) {
    fb.partials_in[b] = icp_half_io(v[b].sc, h).rows_in;
    fb.st[b] = v[b].sc.state; fb.compose16[b] = v[b].compose16; fb.out_T16[b] = v[b].out_T16;
  }
  hipLaunchKernelGGL(gs_icp_finish_batch_kernel, dim3((unsigned)B), dim3(FS_BLOCK), 0, st, fb, n_src_c, h & 1, *prm);   // (reads s[h & 1])
}

// ---- the single solve: one sequence through the same driver and finish, every engine off (grid path), or the brute-force
// path of small problems
static int icp_run(const float* src, int64_t n_src, const float* tgt, const float* tgt_normals,
                   int64_t n_tgt, const float* init16, const float* compose16,
                   const gs_icp_params* prm, float* out_T16, int64_t* out_idx, void* icp_scratch,
                   void* tape, void* stream, const int64_t* n_src_dev = nullptr,
                   const int64_t* n_tgt_dev = nullptr, GsTargetFilter flt = GsTargetFilter{nullptr, 1, 1, 0}) {
  GS_REQUIRE(prm, "params_host must not be NULL");
  GS_REQUIRE(n_src > 0 && n_tgt > 0, "empty point set");
  GS_REQUIRE(n_tgt < 0x7fffffffll && n_src < 0x7fffffffll, "too many points");
  GS_REQUIRE(src && tgt && tgt_normals && init16 && out_T16 && icp_scratch, "NULL pointer");
  GS_REQUIRE(!icp_params_error(prm), icp_params_error(prm));
  hipStream_t st = gs_stream(stream);
  IcpScratch sc = icp_carve(icp_scratch, icp_layout(n_src, n_tgt));
  hipLaunchKernelGGL(gs_icp_init_kernel, dim3(1), dim3(64), 0, st, sc.state, init16, prm->damp, prm->numiters,
                     compose16, out_T16);
  // device-side counts (n_src / n_tgt are then upper bounds) always take the grid path
  const bool dev_counts = n_src_dev || n_tgt_dev || flt.listed;  // a target filter exists only in the grid path
  const bool use_grid = prm->numiters > 0 && (dev_counts || (!gs_env().knn_brute && gs_knn_use_grid(n_src, n_tgt)));
  const GsCount n_src_c{n_src, n_src_dev}, n_tgt_c{n_tgt, n_tgt_dev};
  TapePtrs tp = {nullptr, nullptr, nullptr};
  if (tape) {
    GsIcpTape t = gs_icp_tape_carve(tape, n_src, prm->numiters);
    tp.src = t.src; tp.idx = t.idx; tp.sys = t.sys;
  }
  // the solve as the shared driver sees it: one sequence, no candidate lists
  const IcpSolveView v{src, tgt, tgt_normals, n_tgt_c, sc, grid_carve(sc.grid, n_src, n_tgt), out_idx, tp,
                       IcpHalfLists{nullptr, nullptr, nullptr, nullptr}, IcpHalfWide{nullptr, nullptr}, compose16, out_T16};
  auto cloud = [&](int it) { return icp_cloud(v, it, n_src); };
  auto tidx = [&](int it, int which) { return icp_tape_idx(v, it, which, n_src); };

  if (use_grid) {
    // the target set is fixed for all 2*numiters searches of this solve: bin it once
    int rc = gs_knn_grid_build(tgt, n_tgt_c, n_src, sc.grid, st, flt, tgt_normals);
    if (rc != GS_OK) return rc;
    // one event pair around the 2 x numiters half-iteration kernels; work = algorithmic bytes (icp_alg_bytes).
    // With a target filter n_tgt is the whole map: the binned count is read back (profile passes only).
    double prof_bytes = 0.0;
    if (g_gs_prof_on) {
      int64_t n_binned = n_tgt;
      if (flt.listed) {
        unsigned hits = 0;
        GS_HIP(hipMemcpyAsync(&hits, v.gm.bbox + 6, 4, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        n_binned = hits;
      }
      prof_bytes = icp_alg_bytes(prm->numiters, n_src, n_src, n_binned);
    }
    // the B = 1, engines-off client of the batched driver
    const IcpEnginePlan plan = icp_plain_plan(icp_half_plan(gs_env(), icp_device().cus, n_src, 1), n_src);
    {
      GsProf prof(GS_PROF_ICP_FUSED, prof_bytes, st, 2 * prm->numiters);
      loc_half_iterations(&v, 1, plan, n_src_c, prm, st, true);
    }   // closing event right behind the last half-iteration kernel
    loc_finish(&v, 1, n_src_c, prm, st);
    GS_LAUNCH_CHECK();
    if (tape) return icp_tape_finish(tape, sc.state, n_src, prm->numiters, st);
    return GS_OK;
  }

  // ---- brute-force path
  GS_HIP(hipMemsetAsync(sc.best, 0xff, 8 * (size_t)n_src, st));
  const int nblk = (int)gs_ceil_div(n_src, LIN_BLOCK);
  double* partials = sc.partials[0];
  const float* cur_in = src;
  for (int it = 0; it < prm->numiters; ++it) {
    float* cur = cloud(it);
    // apply the pending transform (initial transform or last T_step) while searching
    gs_knn_brute_launch(cur_in, sc.state->s[0].T_step, cur, n_src, tgt, n_tgt, sc.best, st);
    {
      GsProf prof(GS_PROF_LINEARIZE, 44.0 * (double)n_src, st);  // 8 B best + 12 B src + 24 B gather
      hipLaunchKernelGGL((gs_icp_linearize_kernel<true>), dim3(nblk), dim3(LIN_BLOCK), 0, st, cur, nullptr, n_src,
                         tgt, tgt_normals, n_tgt, sc.best, prm->dist_thresh, partials, out_idx, tidx(it, 0));
    }
    {
      GsProf prof(GS_PROF_SOLVE, 1.0, st);
      hipLaunchKernelGGL(gs_icp_solve_kernel, dim3(1), dim3(SUM_BLOCK), 0, st, partials, nblk, sc.state, it, tp.sys);
    }
    // look-ahead: one_step = Tr * cur, searched and reduced without materialising it
    gs_knn_brute_launch(cur, sc.state->s[0].Tr, nullptr, n_src, tgt, n_tgt, sc.best, st);
    {
      GsProf prof(GS_PROF_LINEARIZE, 44.0 * (double)n_src, st);
      hipLaunchKernelGGL((gs_icp_linearize_kernel<false>), dim3(nblk), dim3(LIN_BLOCK), 0, st, cur,
                         sc.state->s[0].Tr, n_src, tgt, tgt_normals, n_tgt, sc.best, prm->dist_thresh, partials,
                         nullptr, tidx(it, 1));
    }
    {
      GsProf prof(GS_PROF_SOLVE, 1.0, st);
      hipLaunchKernelGGL(gs_icp_update_kernel, dim3(1), dim3(SUM_BLOCK), 0, st, partials, nblk, sc.state, *prm, it,
                         compose16, out_T16);
    }
    cur_in = cur;
  }
  GS_LAUNCH_CHECK();
  if (tape) return icp_tape_finish(tape, sc.state, n_src, prm->numiters, st);
  return GS_OK;
}

extern "C" int gs_icp_f32(const float* src, int64_t n_src, const float* tgt, const float* tgt_normals,
                          int64_t n_tgt, const float* init16, const float* compose16,
                          const gs_icp_params* prm, float* out_T16, int64_t* out_idx, void* icp_scratch,
                          void* stream) {
  return icp_run(src, n_src, tgt, tgt_normals, n_tgt, init16, compose16, prm, out_T16, out_idx, icp_scratch, nullptr,
                 stream);
}

extern "C" int gs_icp_dc_f32(const float* src, int64_t n_src_bound, const int64_t* n_src_dev, const float* tgt,
                             const float* tgt_normals, int64_t n_tgt_bound, const int64_t* n_tgt_dev,
                             const float* init16, const float* compose16, const gs_icp_params* prm, float* out_T16,
                             int64_t* out_idx, void* icp_scratch, void* stream) {
  return icp_run(src, n_src_bound, tgt, tgt_normals, n_tgt_bound, init16, compose16, prm, out_T16, out_idx,
                 icp_scratch, nullptr, stream, n_src_dev, n_tgt_dev);
}

extern "C" int gs_icp_map_dc_f32(const float* src, int64_t n_src_bound, const int64_t* n_src_dev,
                                 const float* map_points, const float* map_normals, const int32_t* pix,
                                 int64_t n_map_bound, const int64_t* n_map_dev, int W, int ds, const float* init16,
                                 const float* compose16, const gs_icp_params* prm, float* out_T16,
                                 void* icp_scratch, void* stream) {
  GS_REQUIRE(pix && W > 0 && ds > 0, "bad target filter");
  return icp_run(src, n_src_bound, map_points, map_normals, n_map_bound, init16, compose16, prm, out_T16, nullptr,
                 icp_scratch, nullptr, stream, n_src_dev, n_map_dev, GsTargetFilter{pix, W, ds, 1});
}

static int localize_chunk(const gs_localize_seq* seqs, int B, int H, int W, int ds, const gs_icp_params* prm,
                          hipStream_t st, bool grid_cleared) {
  const int64_t n_lat = loc_lattice(H, W, ds);
  LocLayout layouts[GS_MAX_BATCH]; LocCarve c[GS_MAX_BATCH];
  for (int b = 0; b < B; ++b) {
    layouts[b] = loc_layout(n_lat, loc_rows(seqs[b].map));
    c[b] = loc_carve(seqs[b].scratch, layouts[b]);
  }
  const IcpEnginePlan plan = icp_engine_plan(gs_env(), icp_device(), B, n_lat, prm->numiters, layouts);
  LocBatch lb; GsGridBatch gb; IcpSolveView v[GS_MAX_BATCH];
  loc_bind(seqs, B, H, W, ds, prm, plan, c, lb, gb, v);
  int rc = loc_prep(seqs, lb, gb, st, grid_cleared);
  if (rc != GS_OK) return rc;
  if (prm->numiters == 0) { GS_LAUNCH_CHECK(); return GS_OK; }
  double prof_bytes = 0.0;
  if (g_gs_prof_on && (rc = loc_prof_bytes(B, c, n_lat, prm->numiters, st, &prof_bytes)) != GS_OK) return rc;
  {
    GsProf prof(GS_PROF_ICP_FUSED, prof_bytes, st, 2 * prm->numiters);
    loc_half_iterations(v, B, plan, GsCount{n_lat, nullptr}, prm, st, false);
  }
  loc_finish(v, B, GsCount{n_lat, nullptr}, prm, st);
  GS_LAUNCH_CHECK();
  return GS_OK;
}

static int localize_batch(const gs_localize_seq* seqs_host, int B, int H, int W, int ds, const gs_icp_params* prm,
                          void* stream, bool grid_cleared, bool vertex_optional = false) {
  GS_REQUIRE(seqs_host && prm && B > 0 && H > 0 && W > 0 && ds > 0, "bad arguments");
  GS_REQUIRE(!icp_params_error(prm), icp_params_error(prm));
  GS_REQUIRE((int64_t)H * W < (1ll << 31), "image too large for int32 pixel ids");
  for (int b = 0; b < B; ++b) {
    const gs_localize_seq& q = seqs_host[b];
    GS_REQUIRE((q.vertex || vertex_optional) && q.depth && q.K16 && q.prev_pose16 && q.out_pose16 && q.scratch, "NULL pointer");
    GS_REQUIRE(q.map.points && q.map.normals && q.map.n_bound > 0 && q.map.n_bound < 0x7fffffffll,
               "every sequence needs a non-empty map (points + normals)");
    GS_REQUIRE(q.map.capacity <= 0 || q.map.n_bound <= q.map.capacity, "map.n_bound exceeds map.capacity");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    const int rc = localize_chunk(seqs_host + c0, nb, H, W, ds, prm, st, grid_cleared);
    if (rc != GS_OK) return rc;
  }
  return GS_OK;
}
extern "C" int gs_localize_batch_f32(const gs_localize_seq* seqs_host, int B, int H, int W, int ds,
                                     const gs_icp_params* prm, void* stream) {
  return localize_batch(seqs_host, B, H, W, ds, prm, stream, false);
}

extern "C" int gs_localize_list_stats_i64(const void* scratch, int H, int W, int ds, int64_t map_rows, int64_t* out192_host,
                                          void* stream) {
  GS_REQUIRE(scratch && out192_host && H > 0 && W > 0 && ds > 0 && map_rows > 0, "bad arguments");
  const LocCarve cv = loc_carve_of(scratch, H, W, ds, map_rows);
  int h[3 * GL_STAT_LAUNCHES];
  hipStream_t st = gs_stream(stream);
  GS_HIP(hipMemcpyAsync(h, cv.lm.stat, sizeof(h), hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < 3 * GL_STAT_LAUNCHES; ++i) out192_host[i] = h[i];
  if (gs_env().debug_grid) {
    GsGrid g;
    GS_HIP(hipMemcpy(&g, cv.gm.g, sizeof(g), hipMemcpyDeviceToHost));
    fprintf(stderr, "grid: box (%.3f %.3f %.3f)-(%.3f %.3f %.3f) c %.4f cells %d x %d x %d = %d\n", g.ox, g.oy, g.oz, g.mx,
            g.my, g.mz, g.c, g.nx, g.ny, g.nz, g.ncell);
  }
  return GS_OK;
}

extern "C" int gs_localize_solve_stats_i64(const void* scratch, int H, int W, int ds, int64_t map_rows, int64_t* out8_host,
                                           void* stream) {
  GS_REQUIRE(scratch && out8_host && H > 0 && W > 0 && ds > 0 && map_rows > 0, "bad arguments");
  const LocCarve cv = loc_carve_of(scratch, H, W, ds, map_rows);
  unsigned weak = 0;
  hipStream_t st = gs_stream(stream);
  GS_HIP(hipMemcpyAsync(&weak, cv.sc.weak_n, sizeof(weak), hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < 8; ++i) out8_host[i] = i == ICP_WEAK_WORD ? (int64_t)weak : 0;
  return GS_OK;
}

extern "C" int gs_pointfusion_step_batch_f32(const gs_step_seq* seqs_host, int B, int H, int W, int ds,
                                             const gs_icp_params* prm, float two_sigma_sq, float dist_th, float dot_th,
                                             int renorm_all, void* stream) {
  GS_REQUIRE(seqs_host && prm && B > 0 && H > 0 && W > 0 && ds > 0, "bad arguments");
  const int64_t P = (int64_t)H * W;
  const gs_step_seq& s0 = seqs_host[0];
  const int64_t dstride = B > 1 ? seqs_host[1].depth - s0.depth : P;
  for (int b = 0; b < B; ++b) {
    const gs_step_seq& q = seqs_host[b];
    GS_REQUIRE(q.depth && q.rgb && q.K16 && q.prev_pose16 && q.out_pose16 && q.normal && q.new_count_out && q.loc_scratch &&
                   q.upd_scratch, "NULL pointer");
    GS_REQUIRE((q.gvertex != nullptr) == (q.gnormal != nullptr) && (q.gvertex != nullptr) == (s0.gvertex != nullptr),
               "gvertex / gnormal: both or none, the same choice for every sequence");
    GS_REQUIRE((q.vertex != nullptr) == (q.alpha != nullptr) && (q.vertex != nullptr) == (s0.vertex != nullptr),
               "vertex / alpha: both or none, the same choice for every sequence");
    GS_REQUIRE(q.vertex || !q.gvertex, "global maps are made from the vertex map: vertex / alpha must be given with them");
    GS_REQUIRE((q.best_pix != nullptr) == (s0.best_pix != nullptr), "best_pix: the same choice for every sequence");
    GS_REQUIRE(q.out_pose16 != q.prev_pose16, "out_pose16 must not alias prev_pose16");
    GS_REQUIRE(q.normal == s0.normal + 3 * P * b && (!q.vertex || (q.vertex == s0.vertex + 3 * P * b && q.alpha == s0.alpha + P * b)),
               "vertex / normal / alpha of the batch must be dense");
    GS_REQUIRE(q.depth == s0.depth + dstride * b && q.K16 == s0.K16 + 16 * (int64_t)b, "depth / K16 must be equally strided");
  }
  GS_REQUIRE(dstride >= P || B == 1, "overlapping depth images");
  // the sequences are independent: chunk by chunk through the frame maps and the localisation; the map update is ONE
  // call for the whole batch (its merge looks at the correspondences of every sequence of the call)
  // Global maps not asked for (gvertex == NULL): they are never written -- the update computes the global vertex / normal
  // of a pixel where it uses them -- and the frame-map launch initialises the update's per-pixel tables, so that the
  // update has no per-pixel pass at all (it was 26 us of a 1.05 ms frame at 8 x 640x480).
  // Local vertex and alpha not asked for (vertex == alpha == NULL, which needs the global maps implicit): not written either
  // -- the lattice source and the update compute the local vertex of a pixel from its depth (fm_vertex: the same bits) and
  // its alpha from that.  best_pix == NULL: the table is no output; the update keeps its tie marks in its scratch.
  const bool implicit_global = s0.gvertex == nullptr;
  std::unique_ptr<gs_update_seq[]> us(new gs_update_seq[B]);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    const gs_step_seq* sq = seqs_host + c0;
    gs_localize_seq ls[GS_MAX_BATCH];
    for (int b = 0; b < nb; ++b) {
      const gs_step_seq& q = sq[b];
      ls[b].vertex = q.vertex; ls[b].depth = q.depth; ls[b].K16 = q.K16; ls[b].prev_pose16 = q.prev_pose16;
      ls[b].map = q.map; ls[b].out_pose16 = q.out_pose16; ls[b].scratch = q.loc_scratch;
      gs_update_seq& u = us[c0 + b];
      u.map = q.map; u.vertex = q.vertex; u.normal = q.normal; u.depth = q.depth; u.rgb = q.rgb;
      u.alpha = q.alpha; u.pose16 = q.out_pose16; u.K16 = q.K16; u.gvertex = q.gvertex;
      u.gnormal = q.gnormal; u.best_pix = q.best_pix; u.new_count_out = q.new_count_out;
      u.scratch = q.upd_scratch;
    }
    // the frame-map launch also zeroes the grid scratch of this chunk's localisation (which then starts with ONE launch
    // for the source lattice and the map projection instead of a clearing launch followed by the projection)
    GsClearJob job;
    job.n = nb;
    for (int b = 0; b < nb; ++b) {
      GS_REQUIRE(ls[b].map.points && ls[b].map.n_bound > 0, "every sequence needs a non-empty map");
      const LocCarve cv = loc_carve_of(ls[b].scratch, H, W, ds, loc_rows(ls[b].map));
      job.ptr[b] = reinterpret_cast<char*>(cv.gm.g);
      if (b == 0) job.bytes = gs_knn_grid_clear_bytes(cv.gm, gs_knn_grid_cells_cap(loc_lattice(H, W, ds)));
    }
    GsPixelTables tabs{};
    tabs.n = implicit_global ? nb : 0;
    tabs.call_flag = c0 == 0 ? gs_update_map_call_flag(seqs_host[0].upd_scratch) : nullptr;
    for (int b = 0; b < tabs.n; ++b) {
      int32_t* best_scratch;
      gs_update_map_tables(sq[b].upd_scratch, P, &tabs.any_flag[b], &tabs.key_pix[b], &best_scratch);
      tabs.best_pix[b] = sq[b].best_pix ? sq[b].best_pix : best_scratch;
    }
    int rc = gs_frame_maps_batch_clear(sq[0].depth, dstride, P, sq[0].K16, nb, 1, H, W, two_sigma_sq, sq[0].vertex,
                                       sq[0].normal, sq[0].alpha, &job, stream, &tabs);
    if (rc != GS_OK) return rc;
    rc = localize_batch(ls, nb, H, W, ds, prm, stream, true, true);
    if (rc != GS_OK) return rc;
  }
  // (two_sigma_sq: with the global maps implicit the update computes the alpha of a pixel from the local vertex it holds,
  // as the frame-map launch above did, instead of gathering alpha[p])
  return gs_update_map_fusion_batch_impl(us.get(), B, H, W, dist_th, dot_th, renorm_all, stream, implicit_global,
                                         two_sigma_sq);
}

extern "C" int64_t gs_icp_tape_bytes(int64_t n_src, int numiters) { return (int64_t)gs_icp_tape_size(n_src, numiters); }

extern "C" int gs_icp_tape_f32(const float* src, int64_t n_src, const float* tgt, const float* tgt_normals,
                               int64_t n_tgt, const float* init16, const float* compose16,
                               const gs_icp_params* prm, float* out_T16, int64_t* out_idx, void* icp_scratch,
                               void* tape, void* stream) {
  GS_REQUIRE(tape, "tape must not be NULL");
  return icp_run(src, n_src, tgt, tgt_normals, n_tgt, init16, compose16, prm, out_T16, out_idx, icp_scratch, tape,
                 stream);
}

extern "C" int gs_icp_trace_f32(const void* icp_scratch, int numiters, float* trace_out, void* stream) {
  GS_REQUIRE(icp_scratch && trace_out && numiters >= 0 && numiters <= GS_ICP_MAX_ITERS, "bad arguments");
  const GsIcpState* st = reinterpret_cast<const GsIcpState*>(icp_scratch);
  GS_HIP(hipMemcpyAsync(trace_out, st->trace, sizeof(float) * 12 * (size_t)numiters, hipMemcpyDeviceToDevice,
                        gs_stream(stream)));
  return GS_OK;
}
