// gs_prune.hip — pruning the surfel map: a stable, batched, out-of-place compaction of all four attributes of B maps.
//
// Row r of a map of n rows survives iff
//     (keep == NULL || keep[r] != 0)  &&  (!use_confidence || r >= young_from || features[r] >= min_confidence)
// (float32 compare: a NaN confidence fails it, a confidence bit-equal to the threshold passes).  Survivor k of the
// input becomes row k of the output in every attribute, moved bit for bit (the rows are copied as 32-bit words, never
// as floats); rows at or beyond the new count are not written.  n = min(*n_dev, n_bound): rows beyond the device count
// never survive, whatever they hold.
//
// Age without a per-surfel channel: rows are appended after all older rows and this compaction keeps input order, so a
// row's index is monotone in its birth step and "appended since epoch e" is "row >= the count at e".  The caller keeps
// up to GS_PRUNE_MAX_MARKS such counts per map ("epoch marks", ascending); young_from is one of them, and after the
// prune every mark m becomes the number of survivors among the rows < min(m, n), so the rule stays right over
// repeated prunes.
//
// The tile scheme of gs_compact.h (restated here with the sequence index in the grid; that header is untouched):
//   count    one block per tile of 1024 consecutive rows: survivors of the tile
//   scan     one block of 1024 threads per sequence: exclusive scan of the tile counts; writes the new count, the
//            removed count, and a copy of young_from for the marks pass
//   scatter  one block per tile: recomputes the predicate, lists the tile's survivors in LDS, then copies the
//            attributes so that consecutive lanes write consecutive 32-bit words of the output (the survivors of a
//            tile land on one contiguous range of every attribute: each wave stores whole 256-byte runs)
//   marks    one block per (sequence, mark): survivors in front of the mark = offset of its tile + survivors of that
//            tile in front of it.  A launch of its own: the marks are rewritten in place, and the passes before it read
//            young_from from them
// Four launches per group of GS_MAX_BATCH sequences, whatever B is (three when no sequence has marks).
//
// Out of place only: a tile's output range lies at or below its input range and overlaps the input of lower tiles that
// other blocks may not have read yet, so an in-place scatter across blocks would be a race.
//
// Bytes per sequence (surfel layout, 40 B per row): the two predicate passes read 4 n each (confidence; + n each with
// keep), the scatter reads 40 B of every surviving row (whole 64-byte lines of the tile: up to 40 n) and writes 40 kept.
#include "gs_compact.h"

constexpr int GS_PRUNE_MAX_MARKS = 64;

struct PrSeq {
  const uint32_t* src[4];   // points, normals, colors, features (as words); any but points may be NULL
  uint32_t* dst[4];
  const uint8_t* keep;
  GsCount n;
  int F;
  int n_marks, young_mark;
  int64_t* marks;
  int64_t* n_out;
  int64_t* removed_out;
  int64_t* young_from;      // scratch: young_from as the count / scatter passes saw it
  int32_t* tile_counts;     // scratch
  int64_t* tile_offsets;    // scratch
  int64_t ntiles;
};
struct PrBatch {
  PrSeq s[GS_MAX_BATCH];
  int B, use_conf;
  float min_conf;
};

// scratch of one sequence: int64 young_from | int32 tile_counts[ntiles] | int64 tile_offsets[ntiles]
static size_t prune_scratch_bytes(int64_t n_bound) {
  const int64_t t = gs_cp_tiles(n_bound);
  return gs_align(sizeof(int64_t)) + gs_align(sizeof(int32_t) * t) + gs_align(sizeof(int64_t) * t);
}

GS_DEV int64_t pr_young_from(const PrSeq& q) {
  // (every row is old enough without a mark: no row index reaches INT64_MAX)
  return q.young_mark >= 0 ? q.marks[q.young_mark] : INT64_MAX;
}

GS_DEV bool pr_survives(const PrSeq& q, int use_conf, float min_conf, int64_t young_from, int64_t e) {
  if (q.keep && q.keep[e] == 0) return false;
  if (!use_conf || e >= young_from) return true;
  return __uint_as_float(q.src[3][e]) >= min_conf;   // F == 1 with use_conf; false for NaN
}

__global__ void __launch_bounds__(GS_CP_BLOCK) gs_prune_count_kernel(const PrBatch pb) {
  __shared__ int smem[GS_CP_BLOCK / GS_WAVE + 1];
  const PrSeq& q = pb.s[blockIdx.x % pb.B];
  const int64_t tile = blockIdx.x / pb.B;
  if (tile >= q.ntiles) return;
  const int64_t n = gs_count(q.n);
  const int64_t young_from = pb.use_conf ? pr_young_from(q) : 0;
  const int64_t base = tile * GS_CP_TILE + (int64_t)threadIdx.x * GS_CP_ITEMS;
  int c = 0;
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    if (e < n && pr_survives(q, pb.use_conf, pb.min_conf, young_from, e)) ++c;
  }
  int total;
  (void)gs_block_excl_scan<GS_CP_BLOCK>(c, smem, &total);
  if (threadIdx.x == 0) q.tile_counts[tile] = total;
}

__global__ void __launch_bounds__(1024) gs_prune_scan_kernel(const PrBatch pb) {
  __shared__ int smem[1024 / GS_WAVE + 1];
  __shared__ int64_t carry;
  const PrSeq& q = pb.s[blockIdx.x];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t t0 = 0; t0 < q.ntiles; t0 += 1024) {
    const int64_t t = t0 + threadIdx.x;
    const int c = (t < q.ntiles) ? q.tile_counts[t] : 0;
    int total;
    const int excl = gs_block_excl_scan<1024>(c, smem, &total);
    if (t < q.ntiles) q.tile_offsets[t] = carry + excl;
    __syncthreads();
    if (threadIdx.x == 0) carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int64_t n = gs_count(q.n);
    q.n_out[0] = carry;
    if (q.removed_out) q.removed_out[0] = n - carry;
    q.young_from[0] = pb.use_conf ? pr_young_from(q) : 0;
  }
}

// words [0, total * C) of the tile's output range, one word per lane and step: word d belongs to survivor d / C
template <int C>
GS_DEV void pr_copy_rows(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const unsigned short* loc,
                         int64_t tile_base, int64_t off, int total, int c_runtime) {
  const int cw = C > 0 ? C : c_runtime;
  const int words = total * cw;
  const uint32_t* s = src + tile_base * cw;
  uint32_t* o = dst + off * cw;
  for (int d = threadIdx.x; d < words; d += GS_CP_BLOCK) {
    const int r = d / cw;
    const int c = d - r * cw;
    o[d] = s[(int)loc[r] * cw + c];
  }
}

__global__ void __launch_bounds__(GS_CP_BLOCK) gs_prune_scatter_kernel(const PrBatch pb) {
  __shared__ int smem[GS_CP_BLOCK / GS_WAVE + 1];
  __shared__ unsigned short loc_s[GS_CP_TILE];
  const PrSeq& q = pb.s[blockIdx.x % pb.B];
  const int64_t tile = blockIdx.x / pb.B;
  if (tile >= q.ntiles) return;
  const int64_t n = gs_count(q.n);
  const int64_t young_from = pb.use_conf ? pr_young_from(q) : 0;
  const int64_t tile_base = tile * GS_CP_TILE;
  if (tile_base >= n) return;   // (the same for the whole block)
  const int64_t base = tile_base + (int64_t)threadIdx.x * GS_CP_ITEMS;
  bool keep[GS_CP_ITEMS];
  int c = 0;
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    keep[i] = (e < n) && pr_survives(q, pb.use_conf, pb.min_conf, young_from, e);
    c += keep[i] ? 1 : 0;
  }
  int total;
  int w = gs_block_excl_scan<GS_CP_BLOCK>(c, smem, &total);
  // the survivors of the tile, in input order (gs_compact.h: writing from the thread that owns the input row scatters
  // the stores of a wave over the tile and multiplies the HBM write traffic)
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    if (keep[i]) loc_s[w++] = (unsigned short)(threadIdx.x * GS_CP_ITEMS + i);
  }
  __syncthreads();
  const int64_t off = q.tile_offsets[tile];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (q.src[a]) pr_copy_rows<3>(q.src[a], q.dst[a], loc_s, tile_base, off, total, 3);
  }
  if (q.src[3]) {
    if (q.F == 1) pr_copy_rows<1>(q.src[3], q.dst[3], loc_s, tile_base, off, total, 1);
    else pr_copy_rows<0>(q.src[3], q.dst[3], loc_s, tile_base, off, total, q.F);
  }
}

__global__ void __launch_bounds__(GS_CP_BLOCK) gs_prune_marks_kernel(const PrBatch pb) {
  __shared__ int smem[GS_CP_BLOCK / GS_WAVE + 1];
  __shared__ int64_t mark_s;
  const PrSeq& q = pb.s[blockIdx.x % pb.B];
  const int j = blockIdx.x / pb.B;
  if (j >= q.n_marks) return;
  const int64_t n = gs_count(q.n);
  // one read of the old mark for the whole block (thread 0 overwrites it below); the block of mark j is the only reader
  // and writer of marks[j], and young_from comes from the scan pass's copy: marks[young_mark] may already be rewritten
  if (threadIdx.x == 0) mark_s = q.marks[j];
  __syncthreads();
  int64_t m = mark_s;
  m = m < 0 ? 0 : m;
  if (m >= n) {
    if (threadIdx.x == 0) q.marks[j] = q.n_out[0];
    return;
  }
  const int64_t young_from = q.young_from[0];
  const int64_t tile = m / GS_CP_TILE;
  const int64_t base = tile * GS_CP_TILE + (int64_t)threadIdx.x * GS_CP_ITEMS;
  int c = 0;
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    if (e < m && pr_survives(q, pb.use_conf, pb.min_conf, young_from, e)) ++c;
  }
  int total;
  (void)gs_block_excl_scan<GS_CP_BLOCK>(c, smem, &total);
  if (threadIdx.x == 0) q.marks[j] = q.tile_offsets[tile] + total;
}

extern "C" int64_t gs_prune_scratch_bytes(int64_t n_bound) {
  return (int64_t)prune_scratch_bytes(n_bound > 0 ? n_bound : 0);
}

extern "C" int gs_prune_map_dc_f32(const gs_prune_seq* seqs_host, int B, float min_confidence, int use_confidence,
                                   void* stream) {
  GS_REQUIRE(seqs_host && B > 0, "bad arguments (NULL descriptors or B <= 0)");
  GS_REQUIRE(!(use_confidence && min_confidence != min_confidence), "min_confidence is NaN");
  for (int b = 0; b < B; ++b) {
    const gs_prune_seq& u = seqs_host[b];
    GS_REQUIRE(u.n_bound >= 0, "negative n_bound");
    GS_REQUIRE(u.n_bound < (1ll << 37), "n_bound too large (tiles of 8 sequences must fit one grid)");
    GS_REQUIRE(u.n_out && u.scratch, "NULL pointer (n_out, scratch)");
    GS_REQUIRE(u.features == nullptr || (u.F > 0 && u.F <= 4096), "F must be in 1..4096 with features");
    GS_REQUIRE(u.capacity_out >= u.n_bound, "destination capacity below n_bound");
    GS_REQUIRE(u.n_marks >= 0 && u.n_marks <= GS_PRUNE_MAX_MARKS, "n_marks must be in 0..64");
    GS_REQUIRE(u.n_marks == 0 || u.marks, "NULL pointer (marks)");
    GS_REQUIRE(u.young_mark >= -1 && u.young_mark < u.n_marks, "young_mark out of range");
    // (an empty map may come without buffers: nothing of it is read)
    if (use_confidence)
      GS_REQUIRE((u.features || u.n_bound == 0) && u.F == 1, "use_confidence needs features with F == 1 (the confidence count)");
    if (u.n_bound > 0) {
      GS_REQUIRE(u.points && u.points_out, "NULL pointer (points, points_out)");
      GS_REQUIRE((!u.normals || u.normals_out) && (!u.colors || u.colors_out) && (!u.features || u.features_out),
                 "NULL pointer (destination of an attribute the source has)");
    }
    GS_REQUIRE(!(u.points && u.points == u.points_out) && !(u.normals && u.normals == u.normals_out) &&
                   !(u.colors && u.colors == u.colors_out) && !(u.features && u.features == u.features_out),
               "source and destination alias: the prune is out of place");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    PrBatch pb = {};
    pb.B = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    pb.use_conf = use_confidence ? 1 : 0;
    pb.min_conf = min_confidence;
    int64_t tiles_max = 0;
    int marks_max = 0;
    for (int b = 0; b < pb.B; ++b) {
      const gs_prune_seq& u = seqs_host[c0 + b];
      PrSeq& s = pb.s[b];
      const float* src[4] = {u.points, u.normals, u.colors, u.features};
      float* dst[4] = {u.points_out, u.normals_out, u.colors_out, u.features_out};
      for (int a = 0; a < 4; ++a) {
        s.src[a] = u.n_bound > 0 ? reinterpret_cast<const uint32_t*>(src[a]) : nullptr;
        s.dst[a] = reinterpret_cast<uint32_t*>(dst[a]);
      }
      s.keep = u.keep;
      s.n = GsCount{u.n_bound, u.n_dev};
      s.F = u.F;
      s.n_marks = u.n_marks;
      s.young_mark = u.young_mark;
      s.marks = u.marks;
      s.n_out = u.n_out;
      s.removed_out = u.removed_out;
      s.ntiles = gs_cp_tiles(u.n_bound);
      char* p = static_cast<char*>(u.scratch);
      s.young_from = reinterpret_cast<int64_t*>(p);
      s.tile_counts = reinterpret_cast<int32_t*>(p + gs_align(sizeof(int64_t)));
      s.tile_offsets = reinterpret_cast<int64_t*>(p + gs_align(sizeof(int64_t)) + gs_align(sizeof(int32_t) * s.ntiles));
      tiles_max = s.ntiles > tiles_max ? s.ntiles : tiles_max;
      marks_max = u.n_marks > marks_max ? u.n_marks : marks_max;
    }
    const unsigned blocks = (unsigned)pb.B * (unsigned)tiles_max;   // < 8 * 2^27 (n_bound < 2^37)
    hipLaunchKernelGGL(gs_prune_count_kernel, dim3(blocks), dim3(GS_CP_BLOCK), 0, st, pb);
    hipLaunchKernelGGL(gs_prune_scan_kernel, dim3((unsigned)pb.B), dim3(1024), 0, st, pb);
    hipLaunchKernelGGL(gs_prune_scatter_kernel, dim3(blocks), dim3(GS_CP_BLOCK), 0, st, pb);
    if (marks_max > 0)
      hipLaunchKernelGGL(gs_prune_marks_kernel, dim3((unsigned)pb.B * (unsigned)marks_max), dim3(GS_CP_BLOCK), 0, st, pb);
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}
