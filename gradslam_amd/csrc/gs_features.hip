// gs_features.hip — a C-channel feature layer next to the surfel map: fused from per-pixel feature images with the
// weights and the correspondences of the colour fusion, and compacted with the map when rows are removed.
//
// A layer of one sequence is emb (capacity, C) float32 | float16 and weight (capacity) float32; row r belongs to map
// row r.  The rule (include/gradslam_hip.h; tests/feature_fuse_ref.py restates it in NumPy):
//   row(p) = best_pix[p]            if 0 <= best_pix[p] < n_old                          (matched)
//            n_old + rank(p)        if best_pix[p] < 0 and depth[p] > 0                   (appended; PredNewPixel's order)
//            none                   otherwise (a stale entry >= n_old, the tie marker)
//   matched, valid:    w2 = w + a; inv = 1 / (w2 == 0 ? 1 : w2); emb = ((w * emb) + (a * feat)) * inv; weight = w2
//                      (fuse_merge_row's operation sequence for colours: float32, one rounding per operation, no FMA)
//   matched, invalid:  untouched
//   appended, valid:   emb = feat (the bits), weight = a
//   appended, invalid: emb = +0, weight = +0
// A map row is matched by at most one pixel (best_pix comes from the unique-winner pass), so every layer row has one
// writer: no atomics, and the result is the same bits on every run.
//
// gs_fuse_features_batch, per group of GS_MAX_BATCH sequences (grid.y = sequence):
//   count   one block per tile of 1024 pixels: appended pixels of the tile
//   scan    one block per sequence: exclusive scan of the tile counts; *n_out = n_old + appended
//   rows    one block per tile: recomputes the predicate and writes row_of_pix
//   fuse    a group of G lanes (a power of two, at most a wave) owns one pixel and moves its row 16 bytes per lane and
//           step (C * sizeof(elem) a multiple of 16; else one element per lane and step: the same operations per
//           element, so the same bits).  With G < 64 several pixels share a wave.  The feature image is read once,
//           coalesced; the only scattered access is the one layer row of a matched pixel.
// gs_compact_features_batch: count / scan / scatter as gs_prune.hip; the survivors of a tile land on one contiguous
// range of emb_out, which the block writes 16 bytes per lane in output order.
//
// Bytes (fuse, per sequence): tables 4 (best_pix) + 4 (depth) + 4 + 4 (row_of_pix, written and read) + 4 (alpha)
// + 1 (valid) per pixel; C * sizeof(elem) per pixel with a row (the feature image, once); matched rows read and
// written, appended rows written.
#include "gs_compact.h"

constexpr int FF_BLOCK = 256;

struct FfSeq {
  char* emb;
  float* weight;
  GsCount n_old;
  const int32_t* best_pix;
  const float* depth;
  const float* alpha;
  const char* feat;
  const uint8_t* valid;
  int32_t* row_of_pix;
  int64_t* n_out;
  int32_t* tile_counts;    // scratch
  int64_t* tile_offsets;   // scratch
};
struct FfBatch {
  FfSeq s[GS_MAX_BATCH];
  int64_t P, ntiles;
  int C, lg;   // lg: log2 of the lanes that own one pixel
};

// the predicate and order of PredNewPixel (gs_fuse.hip)
GS_DEV bool ff_new_pixel(const FfSeq& q, int64_t p) {
  return q.depth[p] > 0.0f && (q.best_pix == nullptr || q.best_pix[p] < 0);
}

__global__ void __launch_bounds__(GS_CP_BLOCK) gs_ff_count_kernel(const FfBatch fb) {
  __shared__ int smem[GS_CP_BLOCK / GS_WAVE + 1];
  const FfSeq& q = fb.s[blockIdx.y];
  const int64_t base = (int64_t)blockIdx.x * GS_CP_TILE + (int64_t)threadIdx.x * GS_CP_ITEMS;
  int c = 0;
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    if (e < fb.P && ff_new_pixel(q, e)) ++c;
  }
  int total;
  (void)gs_block_excl_scan<GS_CP_BLOCK>(c, smem, &total);
  if (threadIdx.x == 0) q.tile_counts[blockIdx.x] = total;
}

// exclusive scan of ntiles tile counts by one block of 1024 threads; returns the grand total to thread 0
GS_DEV int64_t ft_scan_tiles(const int32_t* tile_counts, int64_t* tile_offsets, int64_t ntiles, int* smem,
                             int64_t* carry) {
  if (threadIdx.x == 0) *carry = 0;
  __syncthreads();
  for (int64_t t0 = 0; t0 < ntiles; t0 += 1024) {
    const int64_t t = t0 + threadIdx.x;
    const int c = (t < ntiles) ? tile_counts[t] : 0;
    int total;
    const int excl = gs_block_excl_scan<1024>(c, smem, &total);
    if (t < ntiles) tile_offsets[t] = *carry + excl;
    __syncthreads();
    if (threadIdx.x == 0) *carry += total;
    __syncthreads();
  }
  return *carry;
}

__global__ void __launch_bounds__(1024) gs_ff_scan_kernel(const FfBatch fb) {
  __shared__ int smem[1024 / GS_WAVE + 1];
  __shared__ int64_t carry;
  const FfSeq& q = fb.s[blockIdx.x];
  const int64_t total = ft_scan_tiles(q.tile_counts, q.tile_offsets, fb.ntiles, smem, &carry);
  if (threadIdx.x == 0) q.n_out[0] = gs_count(q.n_old) + total;
}

__global__ void __launch_bounds__(GS_CP_BLOCK) gs_ff_rows_kernel(const FfBatch fb) {
  __shared__ int smem[GS_CP_BLOCK / GS_WAVE + 1];
  const FfSeq& q = fb.s[blockIdx.y];
  const int64_t n_old = gs_count(q.n_old);
  const int64_t base = (int64_t)blockIdx.x * GS_CP_TILE + (int64_t)threadIdx.x * GS_CP_ITEMS;
  bool fresh[GS_CP_ITEMS];
  int c = 0;
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    fresh[i] = (e < fb.P) && ff_new_pixel(q, e);
    c += fresh[i] ? 1 : 0;
  }
  int total;
  int w = gs_block_excl_scan<GS_CP_BLOCK>(c, smem, &total);
  const int64_t first = n_old + q.tile_offsets[blockIdx.x];
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    if (e >= fb.P) continue;
    int32_t row = -1;
    if (fresh[i]) {
      row = (int32_t)(first + w++);
    } else if (q.best_pix) {
      const int32_t bp = q.best_pix[e];
      if (bp >= 0 && bp < n_old) row = bp;
    }
    q.row_of_pix[e] = row;
  }
}

// ---------------------------------------------------------------- one 16-byte unit or one element of a row
// The merged value is a float32 before anything else happens to it: the empty statement keeps the compiler from folding
// the last multiply into the conversion of a float16 layer (v_fma_mixlo_f16: one rounding from the exact product, where
// the rule rounds to float32 first and to float16 second -- other bits in about one element of 2^14).
GS_DEV float ff_merge(float w, float e, float a, float f, float inv) {
  float r = ((w * e) + (a * f)) * inv;
  asm("" : "+v"(r));
  return r;
}

GS_DEV float ff_h2f(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
GS_DEV uint32_t ff_f2h(float v) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v); }   // round to nearest even

GS_DEV uint32_t ff_merge_word(float, uint32_t e, uint32_t f, float w, float a, float inv) {
  return __float_as_uint(ff_merge(w, __uint_as_float(e), a, __uint_as_float(f), inv));
}
GS_DEV uint32_t ff_merge_word(_Float16, uint32_t e, uint32_t f, float w, float a, float inv) {
  const uint32_t lo = ff_f2h(ff_merge(w, ff_h2f(e & 0xffffu), a, ff_h2f(f & 0xffffu), inv));
  const uint32_t hi = ff_f2h(ff_merge(w, ff_h2f(e >> 16), a, ff_h2f(f >> 16), inv));
  return lo | (hi << 16);
}

template <class T>
GS_DEV T ff_merge_elem(T e, T f, float w, float a, float inv) {
  return (T)ff_merge(w, (float)e, a, (float)f, inv);
}

// T: float | _Float16.  VEC: rows move as uint4 units (C * sizeof(T) is a multiple of 16, emb and feat 16-byte aligned)
template <class T, bool VEC>
__global__ void __launch_bounds__(FF_BLOCK) gs_ff_fuse_kernel(const FfBatch fb) {
  const FfSeq& q = fb.s[blockIdx.y];
  const int G = 1 << fb.lg;
  const int lane = threadIdx.x & (G - 1);
  const int64_t p = (int64_t)blockIdx.x * (FF_BLOCK >> fb.lg) + (threadIdx.x >> fb.lg);
  if (p >= fb.P) return;
  const int64_t row = q.row_of_pix[p];
  if (row < 0) return;
  const bool matched = row < gs_count(q.n_old);
  const bool val = q.feat != nullptr && (q.valid == nullptr || q.valid[p] != 0);
  if (matched && !val) return;
  const float a = q.alpha[p];
  float w = 0.0f, w2 = val ? a : 0.0f, inv = 1.0f;
  if (matched) {
    w = q.weight[row];
    w2 = w + a;
    inv = 1.0f / (w2 == 0.0f ? 1.0f : w2);
  }
  if (VEC) {
    const int units = fb.C * (int)sizeof(T) / 16;
    uint4* er = reinterpret_cast<uint4*>(q.emb) + row * units;
    const uint4* fr = reinterpret_cast<const uint4*>(q.feat) + p * units;
    for (int u = lane; u < units; u += G) {
      uint4 o = make_uint4(0u, 0u, 0u, 0u);
      if (val) o = fr[u];
      if (matched) {
        const uint4 e = er[u];
        o.x = ff_merge_word(T(), e.x, o.x, w, a, inv);
        o.y = ff_merge_word(T(), e.y, o.y, w, a, inv);
        o.z = ff_merge_word(T(), e.z, o.z, w, a, inv);
        o.w = ff_merge_word(T(), e.w, o.w, w, a, inv);
      }
      er[u] = o;
    }
  } else {
    T* er = reinterpret_cast<T*>(q.emb) + row * fb.C;
    const T* fr = reinterpret_cast<const T*>(q.feat) + p * fb.C;
    for (int c = lane; c < fb.C; c += G) {
      T o = (T)0.0f;
      if (val) o = fr[c];
      if (matched) o = ff_merge_elem<T>(er[c], o, w, a, inv);
      er[c] = o;
    }
  }
  // (w2 hangs on the load of weight[row] above: the wave has that load back before this store is issued)
  if (lane == 0) q.weight[row] = w2;
}

static int ff_log2_lanes(int units) {
  int lg = 0;
  while (lg < 6 && (1 << lg) < units) ++lg;
  return lg;
}

static bool ff_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" int gs_fuse_features_batch(const gs_feature_fuse_seq* seqs_host, int B, int H, int W, int C, int dtype,
                                      void* stream) {
  GS_REQUIRE(seqs_host && B > 0, "bad arguments (NULL descriptors or B <= 0)");
  GS_REQUIRE(H > 0 && W > 0, "bad sizes (H, W)");
  GS_REQUIRE((int64_t)H * W < (1ll << 31), "H * W must be below 2^31");
  GS_REQUIRE(C >= 1 && C <= 4096, "C must be in 1..4096");
  GS_REQUIRE(dtype == GS_FEATURE_F32 || dtype == GS_FEATURE_F16, "unknown dtype");
  const int64_t P = (int64_t)H * W;
  const int es = dtype == GS_FEATURE_F32 ? 4 : 2;
  const bool vec = ((int64_t)C * es) % 16 == 0;
  for (int b = 0; b < B; ++b) {
    const gs_feature_fuse_seq& u = seqs_host[b];
    GS_REQUIRE(u.emb && u.weight && u.depth && u.alpha && u.row_of_pix && u.n_out && u.scratch,
               "NULL pointer (emb, weight, depth, alpha, row_of_pix, n_out, scratch)");
    GS_REQUIRE(u.n_old_bound >= 0, "negative n_old_bound");
    GS_REQUIRE(u.capacity >= u.n_old_bound + P, "capacity below n_old_bound + H * W");
    GS_REQUIRE(u.n_old_bound + P < (1ll << 31), "n_old_bound + H * W must be below 2^31 (row_of_pix is int32)");
    GS_REQUIRE(ff_aligned16(u.emb), "emb must be 16-byte aligned");
    GS_REQUIRE(!vec || ff_aligned16(u.feat), "feat must be 16-byte aligned when C * sizeof(elem) is a multiple of 16");
    GS_REQUIRE(u.feat != u.emb, "feat and emb alias: a destination equal to its source");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    FfBatch fb = {};
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    fb.P = P;
    fb.ntiles = gs_cp_tiles(P);
    fb.C = C;
    fb.lg = ff_log2_lanes(vec ? C * es / 16 : C);
    for (int b = 0; b < nb; ++b) {
      const gs_feature_fuse_seq& u = seqs_host[c0 + b];
      FfSeq& s = fb.s[b];
      s.emb = static_cast<char*>(u.emb);
      s.weight = u.weight;
      s.n_old = GsCount{u.n_old_bound, u.n_old_dev};
      s.best_pix = u.best_pix;
      s.depth = u.depth;
      s.alpha = u.alpha;
      s.feat = static_cast<const char*>(u.feat);
      s.valid = u.valid;
      s.row_of_pix = u.row_of_pix;
      s.n_out = u.n_out;
      char* p = static_cast<char*>(u.scratch);
      s.tile_counts = reinterpret_cast<int32_t*>(p);
      s.tile_offsets = reinterpret_cast<int64_t*>(p + gs_align(sizeof(int32_t) * fb.ntiles));
    }
    const dim3 tiles((unsigned)fb.ntiles, (unsigned)nb);
    const dim3 wide((unsigned)gs_ceil_div(P, FF_BLOCK >> fb.lg), (unsigned)nb);
    hipLaunchKernelGGL(gs_ff_count_kernel, tiles, dim3(GS_CP_BLOCK), 0, st, fb);
    hipLaunchKernelGGL(gs_ff_scan_kernel, dim3((unsigned)nb), dim3(1024), 0, st, fb);
    hipLaunchKernelGGL(gs_ff_rows_kernel, tiles, dim3(GS_CP_BLOCK), 0, st, fb);
    if (dtype == GS_FEATURE_F32) {
      if (vec) hipLaunchKernelGGL((gs_ff_fuse_kernel<float, true>), wide, dim3(FF_BLOCK), 0, st, fb);
      else hipLaunchKernelGGL((gs_ff_fuse_kernel<float, false>), wide, dim3(FF_BLOCK), 0, st, fb);
    } else {
      if (vec) hipLaunchKernelGGL((gs_ff_fuse_kernel<_Float16, true>), wide, dim3(FF_BLOCK), 0, st, fb);
      else hipLaunchKernelGGL((gs_ff_fuse_kernel<_Float16, false>), wide, dim3(FF_BLOCK), 0, st, fb);
    }
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}

// ---------------------------------------------------------------- compaction of a layer
struct FcSeq {
  const char* emb;
  const uint32_t* weight;
  char* emb_out;
  uint32_t* weight_out;
  const uint8_t* keep;
  GsCount n;
  int64_t* n_out;
  int32_t* tile_counts;    // scratch
  int64_t* tile_offsets;   // scratch
  int64_t ntiles;
};
struct FcBatch {
  FcSeq s[GS_MAX_BATCH];
  int units;   // 16-byte units (vector path) or elements (scalar path) per row
};

__global__ void __launch_bounds__(GS_CP_BLOCK) gs_fc_count_kernel(const FcBatch cb) {
  __shared__ int smem[GS_CP_BLOCK / GS_WAVE + 1];
  const FcSeq& q = cb.s[blockIdx.y];
  if ((int64_t)blockIdx.x >= q.ntiles) return;
  const int64_t n = gs_count(q.n);
  const int64_t base = (int64_t)blockIdx.x * GS_CP_TILE + (int64_t)threadIdx.x * GS_CP_ITEMS;
  int c = 0;
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    if (e < n && q.keep[e] != 0) ++c;
  }
  int total;
  (void)gs_block_excl_scan<GS_CP_BLOCK>(c, smem, &total);
  if (threadIdx.x == 0) q.tile_counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) gs_fc_scan_kernel(const FcBatch cb) {
  __shared__ int smem[1024 / GS_WAVE + 1];
  __shared__ int64_t carry;
  const FcSeq& q = cb.s[blockIdx.x];
  const int64_t total = ft_scan_tiles(q.tile_counts, q.tile_offsets, q.ntiles, smem, &carry);
  if (threadIdx.x == 0) q.n_out[0] = total;
}

// U: uint4 (16-byte units) | uint32_t | uint16_t (one element): the rows are moved as bits
template <class U>
__global__ void __launch_bounds__(GS_CP_BLOCK) gs_fc_scatter_kernel(const FcBatch cb) {
  __shared__ int smem[GS_CP_BLOCK / GS_WAVE + 1];
  __shared__ unsigned short loc_s[GS_CP_TILE];
  const FcSeq& q = cb.s[blockIdx.y];
  if ((int64_t)blockIdx.x >= q.ntiles) return;
  const int64_t n = gs_count(q.n);
  const int64_t tile_base = (int64_t)blockIdx.x * GS_CP_TILE;
  if (tile_base >= n) return;   // (the same for the whole block)
  const int64_t base = tile_base + (int64_t)threadIdx.x * GS_CP_ITEMS;
  bool keep[GS_CP_ITEMS];
  int c = 0;
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    const int64_t e = base + i;
    keep[i] = (e < n) && q.keep[e] != 0;
    c += keep[i] ? 1 : 0;
  }
  int total;
  int w = gs_block_excl_scan<GS_CP_BLOCK>(c, smem, &total);
#pragma unroll
  for (int i = 0; i < GS_CP_ITEMS; ++i) {
    if (keep[i]) loc_s[w++] = (unsigned short)(threadIdx.x * GS_CP_ITEMS + i);
  }
  __syncthreads();
  const int64_t off = q.tile_offsets[blockIdx.x];
  for (int r = threadIdx.x; r < total; r += GS_CP_BLOCK) q.weight_out[off + r] = q.weight[tile_base + loc_s[r]];
  // units [0, total * units) of the tile's output range, one per lane and step: consecutive lanes write consecutive
  // units (unit d belongs to survivor d / units)
  const int units = cb.units;
  const U* s = reinterpret_cast<const U*>(q.emb) + tile_base * units;
  U* o = reinterpret_cast<U*>(q.emb_out) + off * units;
  const int all = total * units;   // <= 1024 * 4096
  for (int d = threadIdx.x; d < all; d += GS_CP_BLOCK) {
    const int r = d / units;
    const int u = d - r * units;
    o[d] = s[(int64_t)loc_s[r] * units + u];
  }
}

extern "C" int gs_compact_features_batch(const gs_feature_compact_seq* seqs_host, int B, int C, int dtype, void* stream) {
  GS_REQUIRE(seqs_host && B > 0, "bad arguments (NULL descriptors or B <= 0)");
  GS_REQUIRE(C >= 1 && C <= 4096, "C must be in 1..4096");
  GS_REQUIRE(dtype == GS_FEATURE_F32 || dtype == GS_FEATURE_F16, "unknown dtype");
  const int es = dtype == GS_FEATURE_F32 ? 4 : 2;
  const bool vec = ((int64_t)C * es) % 16 == 0;
  for (int b = 0; b < B; ++b) {
    const gs_feature_compact_seq& u = seqs_host[b];
    GS_REQUIRE(u.emb && u.weight && u.emb_out && u.weight_out && u.keep && u.n_out && u.scratch,
               "NULL pointer (emb, weight, emb_out, weight_out, keep, n_out, scratch)");
    GS_REQUIRE(u.n_bound >= 0, "negative n_bound");
    GS_REQUIRE(u.n_bound < (1ll << 40), "n_bound too large (the tiles of a sequence must fit one grid)");
    GS_REQUIRE(u.capacity_out >= u.n_bound, "destination capacity below n_bound");
    GS_REQUIRE(ff_aligned16(u.emb) && ff_aligned16(u.emb_out), "emb and emb_out must be 16-byte aligned");
    GS_REQUIRE(u.emb != u.emb_out && u.weight != u.weight_out,
               "source and destination alias: the compaction is out of place");
  }
  hipStream_t st = gs_stream(stream);
  for (int c0 = 0; c0 < B; c0 += GS_MAX_BATCH) {
    FcBatch cb = {};
    const int nb = B - c0 < GS_MAX_BATCH ? B - c0 : GS_MAX_BATCH;
    cb.units = vec ? C * es / 16 : C;
    int64_t tiles_max = 0;
    for (int b = 0; b < nb; ++b) {
      const gs_feature_compact_seq& u = seqs_host[c0 + b];
      FcSeq& s = cb.s[b];
      s.emb = static_cast<const char*>(u.emb);
      s.weight = reinterpret_cast<const uint32_t*>(u.weight);
      s.emb_out = static_cast<char*>(u.emb_out);
      s.weight_out = reinterpret_cast<uint32_t*>(u.weight_out);
      s.keep = u.keep;
      s.n = GsCount{u.n_bound, u.n_dev};
      s.n_out = u.n_out;
      s.ntiles = gs_cp_tiles(u.n_bound);
      char* p = static_cast<char*>(u.scratch);
      s.tile_counts = reinterpret_cast<int32_t*>(p);
      s.tile_offsets = reinterpret_cast<int64_t*>(p + gs_align(sizeof(int32_t) * s.ntiles));
      tiles_max = s.ntiles > tiles_max ? s.ntiles : tiles_max;
    }
    const dim3 tiles((unsigned)tiles_max, (unsigned)nb);
    hipLaunchKernelGGL(gs_fc_count_kernel, tiles, dim3(GS_CP_BLOCK), 0, st, cb);
    hipLaunchKernelGGL(gs_fc_scan_kernel, dim3((unsigned)nb), dim3(1024), 0, st, cb);
    if (vec) hipLaunchKernelGGL((gs_fc_scatter_kernel<uint4>), tiles, dim3(GS_CP_BLOCK), 0, st, cb);
    else if (es == 4) hipLaunchKernelGGL((gs_fc_scatter_kernel<uint32_t>), tiles, dim3(GS_CP_BLOCK), 0, st, cb);
    else hipLaunchKernelGGL((gs_fc_scatter_kernel<uint16_t>), tiles, dim3(GS_CP_BLOCK), 0, st, cb);
    GS_LAUNCH_CHECK();
  }
  return GS_OK;
}
