// gs_picp_scale_dev.h -- what the median rule's select kernel (gs_picp_scale.hip) and the outlier mask's threshold
// kernel (gs_picp_outliers.hip) share, ONE definition: the constants of the key tables, the bin of a histogram that holds
// a rank (ps_pick) and the radix selection of the lower median's key over a sequence's key table (ps_select_median).
#pragma once
#include "gs_picp_dev.h"

constexpr int GS_PS_THREADS = 1024;
static_assert(GS_PS_BINS == 2 * GS_PS_THREADS, "two bins per thread of the select block");
static_assert(GS_PS_BINS % GS_PI_CHUNK == 0, "the residual pass clears and flushes whole rounds of bins");
constexpr uint32_t GS_PS_UNUSED = 0xFFFFFFFFu;
constexpr int GS_PS_TOP_SHIFT = 21;   // the first digit: the top 11 bits

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

// The key of 0-based rank (n - 1) / 2 among the n keys of q that stand for a residual (the bits of the lower median of
// its absolute values), for every thread of a block of GS_PS_THREADS; n (block-uniform) is handed out, and with n == 0
// the result is 0.  A radix selection over the 32 key bits, 11 + 11 + 10: the first digit comes from the counters the
// residual pass left in q.hist (n is their total; the block clears them for the next use), each of the other two is one
// pass over the key table (a histogram in LDS of the pass's digit over the keys that share the digits found so far, an
// exclusive scan, the bin that holds the rank).  Counts and ranks are uint32: they are bounded by nslots < 2^31.
GS_DEV uint32_t ps_select_median(const PiScaleRes& q, const int nslots, uint32_t& n) {
  __shared__ uint32_t hist[GS_PS_BINS];
  __shared__ uint32_t wsum[GS_PS_THREADS / GS_WAVE];
  __shared__ uint32_t sel[2];
  const int tid = threadIdx.x;
  if (tid == 0) { sel[0] = 0u; sel[1] = 0u; }
  // the first digit: the counters of the residual pass, cleared for the next iteration
  uint32_t h0 = q.hist[2 * tid], h1 = q.hist[2 * tid + 1];
  q.hist[2 * tid] = 0u;
  q.hist[2 * tid + 1] = 0u;
  uint32_t bin, rank;
  ps_pick(h0, h1, 0u, false, wsum, sel, bin, rank, n);
  uint32_t prefix = 0u;
  if (n > 0u) {   // (block-uniform)
    prefix = bin << GS_PS_TOP_SHIFT;
    uint32_t known = (uint32_t)(GS_PS_BINS - 1) << GS_PS_TOP_SHIFT;
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
  }
  return prefix;
}
