// gs_picp_color_dev.h — the colour row of a slot of the projective ICP, ONE definition for the joint linearise kernel
// (gs_picp_color.hip) and for the residual pass of the median rule (gs_picp_scale.hip), which needs the colour residual r
// with the linearise kernel's bits.  The arithmetic is spelled out in the header comment of gs_picp_color.hip
// (-ffp-contract=off; float32, one rounding per operation, no FMA in anything below).
#pragma once
#include "gs_picp_dev.h"

GS_DEV float pic_luma(const float r, const float g, const float b) {
  const float t = 0.299f * r + 0.587f * g;
  return t + 0.114f * b;
}

// the continuous pixel (u, v) of the camera-frame point q: the operations of gs_project_point_hw_q
GS_DEV void pic_project_uv(const GsCamera& c, const float* q, float& u, float& v) {
  float r[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float acc = c.K[4 * j] * q[0];
    acc = acc + c.K[4 * j + 1] * q[1];
    acc = acc + c.K[4 * j + 2] * q[2];
    acc = acc + c.K[4 * j + 3] * 1.0f;
    r[j] = acc;
  }
  const float zz = (r[2] != 0.0f) ? r[2] : 1.0f;
  u = r[0] / zz;
  v = r[1] / zz;
}

// The colour row of a slot with code 0 (s: the live vertex under the pose, as pi_associate left it; p: the slot's pixel):
// whether it has one (the model pixel it lands on has ok == 1), and then the residual r BEFORE the weight is applied and
// the row zc = (wgt Js, wgt c, wgt r).  A slot without a colour row leaves r and zc as they are.  A caller that reads r
// only (the residual pass) pays for r only: the Jacobian is dead code there.
GS_DEV bool pic_color_row(const GsCamera& cam, const PiGeom& g, const float* __restrict__ color,
                          const float4* __restrict__ model, const int64_t p, const float* s, const float wgt, float* zc,
                          float& r) {
  // the pixel the association read, again, with the camera-frame point (the same device function on the same
  // operands: the same (h2, w2), inside the view -- the slot would be code 2 otherwise)
  int h2 = 0, w2 = 0;
  float cq[3];
  gs_project_point_hw_q(cam, s[0], s[1], s[2], g.H, g.W, g.u_hi, g.v_hi, h2, w2, cq);
  const float4 M = model[(int64_t)h2 * g.W + w2];   // (I, gx, gy, ok)
  if (!(M.w == 1.0f)) return false;
  float u, v;
  pic_project_uv(cam, cq, u, v);
  const float Il = pic_luma(color[3 * p], color[3 * p + 1], color[3 * p + 2]);
  const float lin = M.x + M.y * (u - (float)w2);
  r = Il - (lin + M.z * (v - (float)h2));
  const float ax = M.y * cam.K[0], ay = M.z * cam.K[5];
  const float j0 = ax / cq[2], j1 = ay / cq[2];
  const float j2 = (-(ax * cq[0] + ay * cq[1])) / (cq[2] * cq[2]);
  // R_m[j][k] = cam.Ri[3 * k + j]
  const float J0 = gs_dot3_plain(cam.Ri[0], cam.Ri[3], cam.Ri[6], j0, j1, j2);
  const float J1 = gs_dot3_plain(cam.Ri[1], cam.Ri[4], cam.Ri[7], j0, j1, j2);
  const float J2 = gs_dot3_plain(cam.Ri[2], cam.Ri[5], cam.Ri[8], j0, j1, j2);
  zc[0] = wgt * J0; zc[1] = wgt * J1; zc[2] = wgt * J2;
  zc[3] = wgt * (J2 * s[1] - J1 * s[2]);
  zc[4] = wgt * (J0 * s[2] - J2 * s[0]);
  zc[5] = wgt * (J1 * s[0] - J0 * s[1]);
  zc[6] = wgt * r;
  return true;
}
