// gs_voxel.hip — voxel thinning of the surfel map: which rows of a map are the one surfel their voxel keeps?
//
// The map update only merges and appends, gs_prune.hip drops rows of low confidence and gs_carve.hip rows that later
// frames see through: nothing removes a surfel merely because others already sit in the same cubic centimetre.  This
// pass finds, per voxel of a regular grid, the most confident row (the oldest among equals) and writes a keep mask; the
// removal is the stable compaction of gs_prune.hip (its keep mask), exactly as for the carve.  No float is moved and
// nothing is averaged.
//
// The rule, per sequence, with n = min(*n_dev, n_bound) read on the device and voxel_size a finite float32 > 0:
//   Voxel of a row.   For each component c, q_c = floorf(p_c / voxel_size): the correctly rounded float32 division (the
//                     build's default, as in gs_picp_color.hip; not a multiplication by a reciprocal), then floorf.
//   Griddable rows.   A row is griddable iff all three p_c are finite and -2^20 <= q_c < 2^20 for all c.  The test is
//                     made on the float, before any conversion to an integer.
//   Key.              key = ((q_x + 2^20) << 42) | ((q_y + 2^20) << 21) | (q_z + 2^20).  It has 63 bits, so an all-ones
//                     word can mean "empty".
//   Score of a row.   The uint32 bit pattern of its confidence (feature channel 0, F == 1) when confidence >= +0.0f
//                     holds in float32; otherwise 0.  So NaN and negative values score 0, and -0.0 scores as +0.0.  Bit
//                     patterns of non-negative floats order like the floats, and +inf is the largest.  Without a
//                     confidence pointer every score is 0.
//   Winner.           Among the griddable rows r < n of one voxel the winner has the largest score.  Ties go to the
//                     lowest row: the oldest surfel, which is also "the first point of the voxel" for a plain cloud.
//   Keep mask.        keep[r] = 1 iff r < n and the row is not griddable or is its voxel's winner.  A non-griddable row
//                     is always kept and never competes.  Rows in [n, n_bound) get 0 and never compete, as in
//                     gs_free_space_dc_f32.
//   Winner output.    winner[r] (int64, optional) is the winner of r's voxel.  It is r itself for a non-griddable row
//                     and -1 for r >= n.
// The result is a pure function of the inputs: bitwise reproducible, no float arithmetic beyond the three divisions,
// and idempotent (a second pass over the compacted map removes nothing).
//
// Two launches per group of GS_MAX_BATCH sequences, the sequence index in the grid (as gs_prune.hip), one thread per
// row, nothing read back.  Each sequence has an open-addressing table in scratch: capacity = the power of two >=
// max(2 n_bound, 1024), two uint64 arrays, key (cleared to all-ones) and best (cleared to 0), 16 B per slot = 32 - 64 B
// per row of the bound.
//   elect     a griddable row r < n probes linearly from a 64-bit mix of its key: prev = atomicCAS(&key[s], EMPTY, k);
//             on prev == EMPTY || prev == k it does atomicMax(&best[s], (score << 32) | (0xFFFFFFFF - r)) and stops.
//             n_bound < 2^31, so the packed word is never 0; the larger word is the larger score, then the lower row.
//             Keys are never removed, so every row of a voxel ends at the same slot whatever the arrival order.
//   resolve   finds the row's slot again with a read-only probe (the table is static by now: a launch of its own),
//             reads best, derives the winner and writes keep / winner; non-griddable rows and rows >= n are written
//             here too.  Every element of both outputs is written by exactly one thread.
// Both probe loops run at most `capacity` times, never while (true).  At a load of at most one half the loop cannot run
// out; if it does, the row is kept (keep = 1, winner = r) and the sequence's int32 `unplaced` counter is bumped: the pass
// fails safe and never hangs.  Integer atomics only.  The worst case, every row of a map in one voxel, is pure
// contention on one atomicMax: merely correct, not fast.
//
// Block of 256: no LDS, no barrier, a handful of registers per thread, so the block size only sets the tail; 256 is
// what the other per-row map passes use.
//
// Bytes per row: 12 B of the point (+ 4 B of the confidence) read in each of the two kernels, one 8-byte CAS and one
// 8-byte max on a random slot in the first, one or a few 8-byte gathers of key and one of best in the second, 1 + 8 B
// written; clearing the table writes 32 - 64 B per row of the bound.
#include "gs_common.h"

#include <math.h>

constexpr uint64_t GS_VX_EMPTY = ~0ull;
constexpr int64_t GS_VX_MIN_CAPACITY = 1024;
constexpr int GS_VX_BLOCK = 256;

struct VxSeq {
  const float* points;
  const float* confidence;   // (n.host) or NULL
  GsCount n;
  uint8_t* keep;             // (n.host) or NULL
  int64_t* winner;           // (n.host) or NULL
  int32_t* unplaced;         // int32[1] or NULL
  uint64_t* key;             // scratch: capacity slots
  uint64_t* best;            // scratch: capacity slots
  uint64_t mask;             // capacity - 1
};
struct VxBatch {
  VxSeq s[GS_MAX_BATCH];
  int B;
  float voxel_size;
};

// slots of one sequence's table: the power of two >= max(2 n_bound, 1024)
static int64_t voxel_capacity(int64_t n_bound) {
  int64_t cap = GS_VX_MIN_CAPACITY;
  while (cap < 2 * n_bound) cap <<= 1;
  return cap;
}

// the key of row r, or false for a row that is not griddable
GS_DEV bool vx_key(const float* __restrict__ points, int64_t r, float voxel_size, uint64_t& key) {
  uint64_t k = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p = points[3 * r + c];
    const float q = floorf(p / voxel_size);
    // (p finite: an infinite p / voxel_size fails the range anyway, a NaN fails every compare; said as the rule says it)
    const bool in = (fabsf(p) < INFINITY) && q >= -1048576.0f && q < 1048576.0f;
    ok = ok && in;
    const int64_t qi = in ? (int64_t)q + (1ll << 20) : 0;   // 0 .. 2^21 - 1
    k = (k << 21) | (uint64_t)qi;
  }
  key = k;
  return ok;
}

GS_DEV uint32_t vx_score(const float* __restrict__ confidence, int64_t r) {
  if (!confidence) return 0u;
  const float c = confidence[r];
  return c >= 0.0f ? (__float_as_uint(c) & 0x7FFFFFFFu) : 0u;   // (the mask only changes -0.0, to +0.0)
}

// splitmix64's finaliser: neighbouring voxels differ in a few low bits of one 21-bit field
GS_DEV uint64_t vx_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__global__ void __launch_bounds__(GS_VX_BLOCK) gs_voxel_elect_kernel(const VxBatch vb) {
  const VxSeq& q = vb.s[blockIdx.x % vb.B];
  const int64_t r = (int64_t)(blockIdx.x / vb.B) * GS_VX_BLOCK + threadIdx.x;
  if (r >= q.n.host) return;
  const int64_t n = gs_count(q.n);
  if (r >= n) return;
  uint64_t k;
  if (!vx_key(q.points, r, vb.voxel_size, k)) return;
  const unsigned long long word =
      ((unsigned long long)vx_score(q.confidence, r) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)r);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(q.key);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(q.best);
  uint64_t s = vx_mix(k) & q.mask;
  for (uint64_t i = 0; i <= q.mask; ++i) {
    const unsigned long long prev = atomicCAS(&keys[s], (unsigned long long)GS_VX_EMPTY, (unsigned long long)k);
    if (prev == GS_VX_EMPTY || prev == k) {
      atomicMax(&best[s], word);
      return;
    }
    s = (s + 1) & q.mask;
  }
  if (q.unplaced) atomicAdd(q.unplaced, 1);   // (a full table: the resolve pass does not find the row and keeps it)
}

__global__ void __launch_bounds__(GS_VX_BLOCK) gs_voxel_resolve_kernel(const VxBatch vb) {
  const VxSeq& q = vb.s[blockIdx.x % vb.B];
  const int64_t r = (int64_t)(blockIdx.x / vb.B) * GS_VX_BLOCK + threadIdx.x;
  if (r >= q.n.host) return;
  const int64_t n = gs_count(q.n);
  int64_t win = -1;
  if (r < n) {
    win = r;   // not griddable, or not in the table: kept
    uint64_t k;
    if (vx_key(q.points, r, vb.voxel_size, k)) {
      uint64_t s = vx_mix(k) & q.mask;
      for (uint64_t i = 0; i <= q.mask; ++i) {
        const uint64_t have = q.key[s];
        if (have == k) {
          win = (int64_t)(0xFFFFFFFFu - (uint32_t)q.best[s]);
          break;
        }
        if (have == GS_VX_EMPTY) break;
        s = (s + 1) & q.mask;
      }
    }
  }
  if (q.keep) q.keep[r] = win == r ? 1 : 0;
  if (q.winner) q.winner[r] = win;
}

extern "C" int64_t gs_voxel_keep_scratch_bytes(int64_t n_bound) {
  return voxel_capacity(n_bound > 0 ? n_bound : 0) * 2 * (int64_t)sizeof(uint64_t);
}

extern "C" int gs_voxel_keep_dc_f32(const gs_voxel_keep_seq* seqs_host, int B, float voxel_size, void* stream) {
  GS_REQUIRE(seqs_host && B > 0, "bad arguments (NULL descriptors or B <= 0)");
  GS_REQUIRE(voxel_size > 0.0f && voxel_size < INFINITY, "voxel_size must be finite and > 0");
  for (int b = 0; b < B; ++b) {
    const gs_voxel_keep_seq& u = seqs_host[b];
    GS_REQUIRE(u.n_bound >= 0, "negative n_bound");
    GS_REQUIRE(u.n_bound < (1ll << 31), "n_bound too large (maps of 2^31 rows or more are not supported: a row index is packed into 32 bits)");
    if (u.n_bound == 0) continue;   // (an empty map may come without buffers: nothing of it is read or written)
    GS_REQUIRE(u.points, "NULL pointer (points)");
    GS_REQUIRE(u.keep || u.winner, "NULL pointer (keep and winner: at least one output is needed)");
    GS_REQUIRE(u.scratch, "NULL pointer (scratch)");
    GS_REQUIRE(u.scratch_bytes >= gs_voxel_keep_scratch_bytes(u.n_bound), "scratch too small (gs_voxel_keep_scratch_bytes(n_bound))");
    GS_REQUIRE((reinterpret_cast<uintptr_t>(u.scratch) & 15) == 0, "scratch must be 16-byte aligned");
    GS_REQUIRE(!u.winner || (reinterpret_cast<uintptr_t>(u.winner) & 7) == 0, "winner must be 8-byte aligned");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    VxBatch vb = {};
    vb.B = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    vb.voxel_size = voxel_size;
    int64_t n_max = 0;
    for (int b = 0; b < vb.B; ++b) {
      const gs_voxel_keep_seq& u = seqs_host[c0 + b];
      VxSeq& s = vb.s[b];
      s.points = u.points;
      s.confidence = u.confidence;
      s.n = GsCount{u.n_bound, u.n_dev};
      s.keep = u.keep;
      s.winner = u.winner;
      s.unplaced = u.unplaced;
      if (u.unplaced) GS_HIP(hipMemsetAsync(u.unplaced, 0, sizeof(int32_t), st));
      if (u.n_bound == 0) continue;
      const int64_t cap = voxel_capacity(u.n_bound);
      s.key = static_cast<uint64_t*>(u.scratch);
      s.best = s.key + cap;
      s.mask = (uint64_t)cap - 1;
      GS_HIP(hipMemsetAsync(s.key, 0xFF, sizeof(uint64_t) * (size_t)cap, st));
      GS_HIP(hipMemsetAsync(s.best, 0, sizeof(uint64_t) * (size_t)cap, st));
      n_max = u.n_bound > n_max ? u.n_bound : n_max;
    }
    if (n_max == 0) continue;
    const unsigned blocks = (unsigned)vb.B * (unsigned)gs_ceil_div(n_max, GS_VX_BLOCK);   // < 8 * 2^23
    hipLaunchKernelGGL(gs_voxel_elect_kernel, dim3(blocks), dim3(GS_VX_BLOCK), 0, st, vb);
    hipLaunchKernelGGL(gs_voxel_resolve_kernel, dim3(blocks), dim3(GS_VX_BLOCK), 0, st, vb);
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}
