// gs_picp_dev.h — what the projective ICP (gs_picp.hip) and its backward pass (gs_picp_bwd.hip) share: the lattice
// geometry, the slot's association at a pose (ONE definition: the backward uses the forward's association exactly, at
// the taped float32 pose), the fixed-shape wave reduction and the layout of the forward tape.
#pragma once
#include "gs_assoc_dev.h"
#include "gs_icp_math.h"

constexpr int GS_PI_CHUNK = 256;
constexpr int GS_PI_TRACE = 8;   // floats per trace row: count, (float)S[27], xi(6)

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
