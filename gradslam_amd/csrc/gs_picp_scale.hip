// gs_picp_scale.hip — the Huber threshold of the projective ICP from the residuals themselves (the scaled entries of
// gs_picp.hip / gs_picp_color.hip): per sequence and per iteration, at the pose T the iteration linearises at,
//
//   delta = max(c * med, floor),   c = (float)huber_k * 1.4826f,   med = the LOWER MEDIAN of |b| over the used slots
//
// (1.4826 * median|b| estimates the residuals' standard deviation, huber_k = 1.345 is the usual Huber constant).  med is
// the element of 0-based rank (n - 1) / 2 of the n values in ascending order: an element of the set, never an average,
// so it is exact; non-negative floats order like their bit patterns read as uint32, which is what is selected.  n == 0:
// delta = +0.0f.  c * med is one float32 product; a product that is not above the floor (a NaN included) gives the floor.
// Two launches in front of the robust linearisation, nothing read back, no float atomics:
//
//   keys    one thread per lattice slot (256 per block = one chunk, batched like the linearise kernel): pi_associate +
//           gn_row_pn at T -- the linearise kernel's own device functions on the same operands, so b has its bits --,
//           key = bits(|b|) of a used slot, 0xFFFFFFFF elsewhere, into the sequence's table (nslots); and the first
//           digit's histogram: the block counts the top 11 bits of its used keys in LDS and adds its non-empty bins to
//           the sequence's 2048 counters (integer atomics: exact in any order)
//   select  one block of 1024 per sequence: a radix selection of the key of rank (n - 1) / 2 over the 32 key bits, 11 +
//           11 + 10.  The first digit comes from the counters the residual pass left (n is their total; the block
//           clears them for the next iteration, one small launch per call clears them in front of the first); each of the other two is one pass over the key table: a histogram in
//           LDS of the pass's digit over the keys that share the digits found so far (LDS integer atomics), an
//           exclusive scan of the 2048 bins (two bins per thread, a wave scan, the 16 wave totals), the bin that holds
//           the rank.  Counts and ranks are uint32: they are bounded by nslots < 2^31.  A lone block reads the table
//           from L2 at the latency of its loads, so every thread has eight 16-byte loads in flight.
//
// The threshold goes to the sequence's device float, which the robust linearise kernels read (PiSeq::delta_dev) and the
// finish kernel copies to the tape row's pad[0], and to the caller's table of thresholds when there is one.
#include "gs_picp_dev.h"

constexpr int GS_PS_THREADS = 1024;
static_assert(GS_PS_BINS == 2 * GS_PS_THREADS, "two bins per thread of the select block");
static_assert(GS_PS_BINS % GS_PI_CHUNK == 0, "the residual pass clears and flushes whole rounds of bins");
constexpr uint32_t GS_PS_UNUSED = 0xFFFFFFFFu;
constexpr int GS_PS_TOP_SHIFT = 21;   // the first digit: the top 11 bits

__global__ void __launch_bounds__(GS_PI_CHUNK) gs_picp_scale_keys_kernel(const PiScaleBatch sb) {
  __shared__ GsCamera cam;
  __shared__ float Ts[12];
  __shared__ uint32_t top[GS_PS_BINS];
  const PiScaleSeq& q = sb.s[blockIdx.x % sb.g.B];
#pragma unroll
  for (int r = 0; r < GS_PS_BINS / GS_PI_CHUNK; ++r) top[threadIdx.x + GS_PI_CHUNK * r] = 0u;   // (the prologue's barrier)
  const PiSlot t = pi_prologue(q.in, sb.g, q.T_in, cam, Ts);
  const int64_t n_map = gs_count(q.in.n);
  if (t.in_lattice) {
    int64_t row;
    float s[3], a[6], b = 0.0f;
    float4 d, m;
    const bool used = pi_associate(Ts, cam, q.in, sb.g, n_map, t.p, row, s, d, m) == 0;
    if (used) gn_row_pn(s[0], s[1], s[2], d, m, a, b);
    const uint32_t key = used ? __float_as_uint(fabsf(b)) : GS_PS_UNUSED;
    q.keys[t.k] = key;
    if (used) atomicAdd(&top[key >> GS_PS_TOP_SHIFT], 1u);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < GS_PS_BINS / GS_PI_CHUNK; ++r) {
    const int bin = threadIdx.x + GS_PI_CHUNK * r;
    const uint32_t c = top[bin];
    if (c != 0u) atomicAdd(&q.hist[bin], c);
  }
}

// The bin of a 2048-bin histogram that holds `rank` (0-based, below the histogram's total) and the rank inside it, for
// every thread of the select block; h0, h1: the counts of the thread's bins 2 tid, 2 tid + 1.  total: the histogram's.
GS_DEV void ps_pick(const uint32_t h0, const uint32_t h1, const uint32_t rank, const bool have_rank, uint32_t* wsum,
                    uint32_t* sel, uint32_t& bin, uint32_t& inside, uint32_t& total) {
  const int tid = threadIdx.x, lane = tid & (GS_WAVE - 1), wave = tid / GS_WAVE;
  const uint32_t v = h0 + h1;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < GS_WAVE; d <<= 1) {
    const uint32_t y = __shfl_up(inc, d, GS_WAVE);
    if (lane >= d) inc += y;
  }
  if (lane == GS_WAVE - 1) wsum[wave] = inc;
  __syncthreads();
  uint32_t excl = inc - v;
  total = 0u;
#pragma unroll
  for (int w = 0; w < GS_PS_THREADS / GS_WAVE; ++w) {
    if (w < wave) excl += wsum[w];
    total += wsum[w];
  }
  // the rank of the first digit is known only with the total: (total - 1) / 2
  const uint32_t want = have_rank ? rank : (total > 0u ? (total - 1u) / 2u : 0u);
  // exactly one thread when total > 0: the bins are disjoint ranges of ranks
  if (want >= excl && want - excl < v) {
    const bool second = want - excl >= h0;
    sel[0] = 2u * (uint32_t)tid + (second ? 1u : 0u);
    sel[1] = want - excl - (second ? h0 : 0u);
  }
  __syncthreads();
  bin = sel[0];
  inside = sel[1];
  __syncthreads();   // (wsum and sel are rewritten by the next call)
}

__global__ void __launch_bounds__(GS_PS_THREADS) gs_picp_scale_select_kernel(const PiScaleBatch sb, const float c,
                                                                             const float floor) {
  __shared__ uint32_t hist[GS_PS_BINS];
  __shared__ uint32_t wsum[GS_PS_THREADS / GS_WAVE];
  __shared__ uint32_t sel[2];
  const PiScaleSeq& q = sb.s[blockIdx.x];
  const int tid = threadIdx.x;
  const int nslots = sb.g.nslots;
  if (tid == 0) { sel[0] = 0u; sel[1] = 0u; }
  // the first digit: the counters of the residual pass, cleared for the next iteration
  uint32_t h0 = q.hist[2 * tid], h1 = q.hist[2 * tid + 1];
  q.hist[2 * tid] = 0u;
  q.hist[2 * tid + 1] = 0u;
  uint32_t bin, rank, n;
  ps_pick(h0, h1, 0u, false, wsum, sel, bin, rank, n);
  float delta = 0.0f;
  if (n > 0u) {   // (block-uniform)
    uint32_t prefix = bin << GS_PS_TOP_SHIFT, known = (uint32_t)(GS_PS_BINS - 1) << GS_PS_TOP_SHIFT;
    const uint4* keys4 = reinterpret_cast<const uint4*>(q.keys);   // (16-byte aligned: the entries check the scratch, the offsets are multiples of 256)
    const int n4 = nslots / 4;
    constexpr int DEPTH = 8;   // 16-byte loads in flight per thread
#pragma unroll 1
    for (int pass = 1; pass < 3; ++pass) {
      const int shift = pass == 1 ? 10 : 0;
      const uint32_t digit = pass == 1 ? 2047u : 1023u;
      hist[tid] = 0u;
      hist[tid + GS_PS_THREADS] = 0u;
      __syncthreads();
      const auto count = [&](const uint32_t k) {
        if ((k & known) == prefix) atomicAdd(&hist[(k >> shift) & digit], 1u);
      };
      int i = tid;
      for (; i + (DEPTH - 1) * GS_PS_THREADS < n4; i += DEPTH * GS_PS_THREADS) {
        uint4 k[DEPTH];
#pragma unroll
        for (int r = 0; r < DEPTH; ++r) k[r] = keys4[i + r * GS_PS_THREADS];
#pragma unroll
        for (int r = 0; r < DEPTH; ++r) { count(k[r].x); count(k[r].y); count(k[r].z); count(k[r].w); }
      }
      for (; i < n4; i += GS_PS_THREADS) {
        const uint4 k = keys4[i];
        count(k.x); count(k.y); count(k.z); count(k.w);
      }
      for (int j = 4 * n4 + tid; j < nslots; j += GS_PS_THREADS) count(q.keys[j]);
      __syncthreads();
      uint32_t total;
      ps_pick(hist[2 * tid], hist[2 * tid + 1], rank, true, wsum, sel, bin, rank, total);
      prefix |= bin << shift;
      known |= digit << shift;
    }
    delta = c * __uint_as_float(prefix);
    if (!(delta > floor)) delta = floor;
  }
  if (tid == 0) {
    *q.delta_dev = delta;
    if (q.delta_out) *q.delta_out = delta;
  }
}

// the counters of every sequence of the batch, cleared: one block per sequence
__global__ void __launch_bounds__(GS_PS_THREADS) gs_picp_scale_clear_kernel(const PiScaleBatch sb) {
  uint32_t* hist = sb.s[blockIdx.x].hist;
  hist[2 * threadIdx.x] = 0u;
  hist[2 * threadIdx.x + 1] = 0u;
}

void picp_scale_launch(const PiScaleBatch& sb, const float c, const float floor, const bool first, hipStream_t st) {
  if (first) hipLaunchKernelGGL(gs_picp_scale_clear_kernel, dim3((unsigned)sb.g.B), dim3(GS_PS_THREADS), 0, st, sb);
  hipLaunchKernelGGL(gs_picp_scale_keys_kernel, dim3((unsigned)sb.g.B * (unsigned)sb.g.nchunks), dim3(GS_PI_CHUNK), 0, st,
                     sb);
  hipLaunchKernelGGL(gs_picp_scale_select_kernel, dim3((unsigned)sb.g.B), dim3(GS_PS_THREADS), 0, st, sb, c, floor);
}
