// gs_picp_scale.hip — the Huber threshold of the projective ICP from the residuals themselves (the scaled entries of
// gs_picp.hip / gs_picp_color.hip): per sequence and per iteration, at the pose T the iteration linearises at,
//
//   delta = max(c * med, floor),   c = (float)huber_k * 1.4826f,   med = the LOWER MEDIAN of |b| over the used slots
//
// and, for the joint solve, the same rule on the COLOUR residual r before color_weight is applied (gs_picp_color_dev.h:
// pic_color_row, the linearise kernel's own function), over the slots that have a colour row:
//
//   cdelta = max(c_c * med_c, cfloor),   c_c = (float)color_huber_k * 1.4826f;   n == 0: cdelta = cfloor
//
// Either rule alone or both: the launches are the same.  Below, "used" reads "coloured" and b reads r for that residual.
// (1.4826 * median|b| estimates the residuals' standard deviation, huber_k = 1.345 is the usual Huber constant).  med is
// the element of 0-based rank (n - 1) / 2 of the n values in ascending order: an element of the set, never an average,
// so it is exact; non-negative floats order like their bit patterns read as uint32, which is what is selected.  n == 0:
// delta = +0.0f.  c * med is one float32 product; a product that is not above the floor (a NaN included) gives the floor.
// Two launches in front of the robust linearisation, nothing read back, no float atomics:
//
//   keys    (ps_keys<GEO, COL>: one instance per set of residuals asked for; one pi_associate serves both, each has its
//           own key table, LDS histogram and counters)
//           one thread per lattice slot (256 per block = one chunk, batched like the linearise kernel): pi_associate +
//           gn_row_pn at T -- the linearise kernel's own device functions on the same operands, so b has its bits --,
//           key = bits(|b|) of a used slot, 0xFFFFFFFF elsewhere, into the sequence's table (nslots); and the first
//           digit's histogram: the block counts the top 11 bits of its used keys in LDS and adds its non-empty bins to
//           the sequence's 2048 counters (integer atomics: exact in any order)
//   select  one block of 1024 per sequence and residual asked for (PiScalePick: block x serves residual first + x / B of
//           sequence x % B, with that residual's tables, constant, floor and destination): a radix selection of the key
//           of rank (n - 1) / 2 over the 32 key bits, 11 + 11 + 10.  The first digit comes from the counters the residual pass left (n is their total; the block
//           clears them for the next iteration, one small launch per call clears them in front of the first); each of the other two is one pass over the key table: a histogram in
//           LDS of the pass's digit over the keys that share the digits found so far (LDS integer atomics), an
//           exclusive scan of the 2048 bins (two bins per thread, a wave scan, the 16 wave totals), the bin that holds
//           the rank.  Counts and ranks are uint32: they are bounded by nslots < 2^31.  A lone block reads the table
//           from L2 at the latency of its loads, so every thread has eight 16-byte loads in flight.
//
// The threshold goes to the sequence's device float, which the robust linearise kernels read (PiSeq::delta_dev; the
// colour one: PicSeq::cdelta_dev of gs_picp_color.hip) and the
// finish kernel copies to the tape row's pad[0], and to the caller's table of thresholds when there is one.
// The selection itself (ps_pick, ps_select_median) is gs_picp_scale_dev.h's, shared with gs_picp_outliers.hip.
#include "gs_picp_color_dev.h"
#include "gs_picp_scale_dev.h"


// The residual pass.  GEO / COL: the residuals asked for (at least one); for the other one nothing is computed, loaded
// or stored.  One pi_associate per slot serves both.  Each residual has its own first-digit histogram in LDS (8 KB; both:
// 16 KB a block, which at 256 threads still leaves room for the 8 waves a SIMD can hold).
// WEIGHTED (the weighted entries): pi_associate<true>, so a slot whose pixel weight masks it (code 6) has no key and is
// in no median; the residuals themselves are the unweighted ones.
template <bool GEO, bool COL, bool WEIGHTED = false>
GS_DEV void ps_keys(const PiScaleBatch& sb) {
  static_assert(GEO || COL, "a residual pass without a residual");
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  __shared__ uint32_t top[(GEO ? 1 : 0) + (COL ? 1 : 0)][GS_PS_BINS];
  constexpr int CTOP = GEO ? 1 : 0;   // the colour residual's histogram
  const PiScaleSeq& q = sb.s[blockIdx.x % sb.g.B];
#pragma unroll
  for (int r = 0; r < GS_PS_BINS / GS_PI_CHUNK; ++r) {   // (the prologue's barrier)
    top[0][threadIdx.x + GS_PI_CHUNK * r] = 0u;
    if (GEO && COL) top[CTOP][threadIdx.x + GS_PI_CHUNK * r] = 0u;
  }
  const PiSlot t = pi_prologue(q.in, sb.g, q.T_in, cam, Ts);
  const int64_t n_map = gs_count(q.in.n);
  if (t.in_lattice) {
    int64_t row;
    float s[3];
    float4 d, m;
    float wp;
    const bool used = pi_associate<WEIGHTED>(Ts, cam, q.in, sb.g, n_map, t.p, row, s, d, m, wp) == 0;
    if (GEO) {
      float a[6], b = 0.0f;
      if (used) gn_row_pn(s[0], s[1], s[2], d, m, a, b);
      const uint32_t key = used ? __float_as_uint(fabsf(b)) : GS_PS_UNUSED;
      q.r[PS_GEO].keys[t.k] = key;
      if (used) atomicAdd(&top[0][key >> GS_PS_TOP_SHIFT], 1u);
    }
    if (COL) {
      // the colour residual before the weight: the linearise kernel's device function on its operands (the row's other
      // seven values depend on the weight and are not formed)
      float zc[7], r = 0.0f;
      const bool colored = used && pic_color_row(cam, sb.g, q.color, q.model, t.p, s, 1.0f, zc, r);
      const uint32_t key = colored ? __float_as_uint(fabsf(r)) : GS_PS_UNUSED;
      q.r[PS_COLOR].keys[t.k] = key;
      if (colored) atomicAdd(&top[CTOP][key >> GS_PS_TOP_SHIFT], 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < GS_PS_BINS / GS_PI_CHUNK; ++r) {
    const int bin = threadIdx.x + GS_PI_CHUNK * r;
    if (GEO) {
      const uint32_t c = top[0][bin];
      if (c != 0u) atomicAdd(&q.r[PS_GEO].hist[bin], c);
    }
    if (COL) {
      const uint32_t c = top[CTOP][bin];
      if (c != 0u) atomicAdd(&q.r[PS_COLOR].hist[bin], c);
    }
  }
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_scale_keys_kernel(const PiScaleBatch sb) { ps_keys<true, false>(sb); }
__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_scale_color_keys_kernel(const PiScaleBatch sb) {
  ps_keys<false, true>(sb);
}
__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_scale_joint_keys_kernel(const PiScaleBatch sb) {
  ps_keys<true, true>(sb);
}

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_weighted_picp_scale_keys_kernel(const PiScaleBatch sb) {
  ps_keys<true, false, true>(sb);
}
__global__ void __launch_bounds__(GS_PI_CHUNK) gs_weighted_picp_scale_color_keys_kernel(const PiScaleBatch sb) {
  ps_keys<false, true, true>(sb);
}
__global__ void __launch_bounds__(GS_PI_CHUNK) gs_weighted_picp_scale_joint_keys_kernel(const PiScaleBatch sb) {
  ps_keys<true, true, true>(sb);
}

// A grid of B * pk.count blocks: block x selects residual pk.first + x / B of sequence x % B, with that residual's keys,
// counters, constant, floor and destination.
__global__ void __launch_bounds__(GS_PS_THREADS) gs_picp_scale_select_kernel(const PiScaleBatch sb,
                                                                             const PiScalePick pk) {
  const int which = pk.first + (int)blockIdx.x / sb.g.B;
  const PiScaleRes& q = sb.s[blockIdx.x % sb.g.B].r[which];
  const float c = pk.c[which], floor = pk.floor[which];
  const int tid = threadIdx.x;
  uint32_t n;
  const uint32_t med = ps_select_median(q, sb.g.nslots, n);
  // no slot has the row: +0.0 for the geometric threshold, the floor for the colour one (no weight is read then)
  float delta = which == PS_COLOR ? floor : 0.0f;
  if (n > 0u) {   // (block-uniform)
    delta = c * __uint_as_float(med);
    if (!(delta > floor)) delta = floor;
  }
  if (tid == 0) {
    *q.delta_dev = delta;
    if (q.delta_out) *q.delta_out = delta;
  }
}

// the counters of every sequence of the batch, cleared: one block per sequence and residual asked for (the select's grid)
__global__ void __launch_bounds__(GS_PS_THREADS) gs_picp_scale_clear_kernel(const PiScaleBatch sb, const PiScalePick pk) {
  uint32_t* hist = sb.s[blockIdx.x % sb.g.B].r[pk.first + (int)blockIdx.x / sb.g.B].hist;
  hist[2 * threadIdx.x] = 0u;
  hist[2 * threadIdx.x + 1] = 0u;
}

void picp_scale_keys_launch(const PiScaleBatch& sb, const PiScalePick& pk, const bool first, const bool weighted,
                             hipStream_t st) {
  const dim3 per_res((unsigned)sb.g.B * (unsigned)pk.count), chunks((unsigned)sb.g.B * (unsigned)sb.g.nchunks);
  if (first) hipLaunchKernelGGL(gs_picp_scale_clear_kernel, per_res, dim3(GS_PS_THREADS), 0, st, sb, pk);
  const auto keys = pk.count == 2 ? (weighted ? gs_weighted_picp_scale_joint_keys_kernel : gs_picp_scale_joint_keys_kernel)
                    : pk.first == PS_COLOR
                        ? (weighted ? gs_weighted_picp_scale_color_keys_kernel : gs_picp_scale_color_keys_kernel)
                        : (weighted ? gs_weighted_picp_scale_keys_kernel : gs_picp_scale_keys_kernel);
  hipLaunchKernelGGL(keys, chunks, dim3(GS_PI_CHUNK), 0, st, sb);
}

void picp_scale_launch(const PiScaleBatch& sb, const PiScalePick& pk, const bool first, const bool weighted,
                       hipStream_t st) {
  picp_scale_keys_launch(sb, pk, first, weighted, st);
  hipLaunchKernelGGL(gs_picp_scale_select_kernel, dim3((unsigned)sb.g.B * (unsigned)pk.count), dim3(GS_PS_THREADS), 0, st,
                     sb, pk);
}
