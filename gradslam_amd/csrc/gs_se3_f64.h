// gs_se3_f64.h — float64 device pieces shared by the backward passes (gs_icp_bwd.hip, gs_picp_bwd.hip): 4x4 / 3x3
// products, the SE(3) exponential and its adjoint, the un-pivoted 6x6 solve.  One lane runs them; all float64.
#pragma once
#include "gs_common.h"

GS_DEV void d_mm4(const double* A, const double* B, double* C) {
  double t[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc += A[4 * i + k] * B[4 * k + j];
      t[4 * i + j] = acc;
    }
  for (int i = 0; i < 16; ++i) C[i] = t[i];
}

GS_DEV void d_hat(const double* w, double* wh) {
  wh[0] = 0; wh[1] = -w[2]; wh[2] = w[1];
  wh[3] = w[2]; wh[4] = 0; wh[5] = -w[0];
  wh[6] = -w[1]; wh[7] = w[0]; wh[8] = 0;
}
GS_DEV void d_mm3(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// geometry/se3utils.py:77-115 in double
GS_DEV void d_se3_exp(const double* xi, double* T) {
  const double* v = xi;
  const double* w = xi + 3;
  double wh[9], wh2[9], R[9], V[9];
  d_hat(w, wh);
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if ((float)th < 1e-6f) {
    for (int i = 0; i < 9; ++i) { R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + wh[i]; V[i] = R[i]; }
  } else {
    d_mm3(wh, wh, wh2);
    const double s = sin(th), c = cos(th);
    const double A = s / th, B = (1 - c) / (th * th), Cc = (th - s) / (th * th * th);
    for (int i = 0; i < 9; ++i) {
      const double I = (i % 4 == 0) ? 1.0 : 0.0;
      R[i] = I + A * wh[i] + B * wh2[i];
      V[i] = I + B * wh[i] + Cc * wh2[i];
    }
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
    T[4 * i + 3] = V[3 * i] * v[0] + V[3 * i + 1] * v[1] + V[3 * i + 2] * v[2];
  }
  T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}

// d <Tbar, Exp(xi)> / d xi (Tbar: 4x4, only its top three rows matter)
GS_DEV void d_se3_exp_adjoint(const double* xi, const double* Tbar, double* out) {
  const double* v = xi;
  const double* w = xi + 3;
  double Rb[9], tb[3], wh[9], wh2[9], V[9], Vb[9], whb[9];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rb[3 * i + j] = Tbar[4 * i + j];
    tb[i] = Tbar[4 * i + 3];
  }
  d_hat(w, wh);
  d_mm3(wh, wh, wh2);
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const bool small = (float)th < 1e-6f;
  double s = 0, c = 1, A = 1, B = 0, Cc = 0;
  if (small) {
    for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + wh[i];
  } else {
    s = sin(th); c = cos(th);
    A = s / th; B = (1 - c) / (th * th); Cc = (th - s) / (th * th * th);
    for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + B * wh[i] + Cc * wh2[i];
  }
  for (int j = 0; j < 3; ++j) out[j] = V[j] * tb[0] + V[3 + j] * tb[1] + V[6 + j] * tb[2];  // V^T tb
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Vb[3 * i + j] = tb[i] * v[j];
  double thb = 0.0;
  if (small) {
    for (int i = 0; i < 9; ++i) whb[i] = Rb[i] + Vb[i];
  } else {
    double Ab = 0, Bb = 0, Cb = 0, W2b[9], whT[9], t1[9], t2[9];
    for (int i = 0; i < 9; ++i) {
      Ab += Rb[i] * wh[i];
      Bb += Rb[i] * wh2[i] + Vb[i] * wh[i];
      Cb += Vb[i] * wh2[i];
      W2b[i] = B * Rb[i] + Cc * Vb[i];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) whT[3 * i + j] = wh[3 * j + i];
    d_mm3(W2b, whT, t1);
    d_mm3(whT, W2b, t2);
    for (int i = 0; i < 9; ++i) whb[i] = A * Rb[i] + B * Vb[i] + t1[i] + t2[i];
    const double dA = (c * th - s) / (th * th);
    const double dB = (s * th - 2 * (1 - c)) / (th * th * th);
    const double dC = ((1 - c) * th - 3 * (th - s)) / (th * th * th * th);
    thb = Ab * dA + Bb * dB + Cb * dC;
  }
  out[3] = whb[7] - whb[5];
  out[4] = whb[2] - whb[6];
  out[5] = whb[3] - whb[1];
  if (!small)
    for (int j = 0; j < 3; ++j) out[3 + j] += thb * w[j] / th;
}

// 6x6 symmetric positive definite solve in double (un-pivoted Gauss-Jordan)
GS_DEV void d_solve6(const double* H, const double* rhs, double* x) {
  double a[6][7];
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) a[i][j] = H[6 * i + j];
    a[i][6] = rhs[i];
  }
  for (int c = 0; c < 6; ++c) {
    const double inv = 1.0 / a[c][c];
    for (int j = c; j <= 6; ++j) a[c][j] *= inv;
    for (int r = 0; r < 6; ++r) {
      if (r == c) continue;
      const double f = a[r][c];
      for (int j = c; j <= 6; ++j) a[r][j] -= f * a[c][j];
    }
  }
  for (int i = 0; i < 6; ++i) x[i] = a[i][6];
}
