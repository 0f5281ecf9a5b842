// new_points_geom.h -- the per-neighbour geometry of vo_kfstore_create_map_points: camera centres,
// baseline, F12 (LocalMapping::computeF12, localMapping.cpp:526-536, in closed form) and the epipole
// (matcher.cpp:887-891).  Every operation is an explicitly rounded double operation in the order DESIGN.md writes down, so
// that tests/new_points_ref.py reproduces F12, ex, ey and the baseline bit for bit.
#pragma once
#include "vo_common.h"

namespace vo {

// (a * b + c * d) + e * f, each product and sum rounded
__device__ __forceinline__ double np_dot3(double a, double b, double c, double d, double e, double f) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a, b), __dmul_rn(c, d)), __dmul_rn(e, f));
}

// Ow = -(R^T t): Ow[i] = -((R[0][i] t[0] + R[1][i] t[1]) + R[2][i] t[2])
__device__ __forceinline__ void np_center(const double *T, double Ow[3]) {
  for (int i = 0; i < 3; i++) Ow[i] = -np_dot3(T[i], T[9], T[3 + i], T[10], T[6 + i], T[11]);
}

// T: R row-major (9) then t (3).  cam: fx, fy, cx, cy as the floats Camera holds.  -> G.F, G.ex, G.ey, G.Ow1, G.Ow2, G.bl
__device__ inline void np_geometry(const double *T1, const double *T2, const float *cam, NpStep &G) {
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
  np_center(T1, G.Ow1);
  np_center(T2, G.Ow2);
  double d[3];
  for (int i = 0; i < 3; i++) d[i] = __dadd_rn(G.Ow2[i], -G.Ow1[i]);
  G.bl = (float)__dsqrt_rn(np_dot3(d[0], d[0], d[1], d[1], d[2], d[2]));  // float bl = baseline.norm()  :171-172
  double R12[9], t12[3], M[9], N[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R12[3 * i + j] = np_dot3(T1[3 * i], T2[3 * j], T1[3 * i + 1], T2[3 * j + 1], T1[3 * i + 2], T2[3 * j + 2]);
  for (int i = 0; i < 3; i++)
    t12[i] = __dadd_rn(T1[9 + i], -np_dot3(R12[3 * i], T2[9], R12[3 * i + 1], T2[10], R12[3 * i + 2], T2[11]));
  for (int j = 0; j < 3; j++) {  // M = [t12]x R12
    M[j] = __dadd_rn(__dmul_rn(-t12[2], R12[3 + j]), __dmul_rn(t12[1], R12[6 + j]));
    M[3 + j] = __dadd_rn(__dmul_rn(t12[2], R12[j]), __dmul_rn(-t12[0], R12[6 + j]));
    M[6 + j] = __dadd_rn(__dmul_rn(-t12[1], R12[j]), __dmul_rn(t12[0], R12[3 + j]));
  }
  // K^-1 = [ifx 0 mcx; 0 ify mcy; 0 0 1]
  const double ifx = __ddiv_rn(1.0, fx), ify = __ddiv_rn(1.0, fy), mcx = -__dmul_rn(cx, ifx), mcy = -__dmul_rn(cy, ify);
  for (int i = 0; i < 3; i++) {  // N = M K^-1
    N[3 * i] = __dmul_rn(M[3 * i], ifx);
    N[3 * i + 1] = __dmul_rn(M[3 * i + 1], ify);
    N[3 * i + 2] = __dadd_rn(__dadd_rn(__dmul_rn(M[3 * i], mcx), __dmul_rn(M[3 * i + 1], mcy)), M[3 * i + 2]);
  }
  for (int j = 0; j < 3; j++) {  // F12 = K^-T N
    G.F[j] = __dmul_rn(ifx, N[j]);
    G.F[3 + j] = __dmul_rn(ify, N[3 + j]);
    G.F[6 + j] = __dadd_rn(__dadd_rn(__dmul_rn(mcx, N[j]), __dmul_rn(mcy, N[3 + j])), N[6 + j]);
  }
  // the epipole: camera2pixel(R2 Ow1 + t2), fx * x / z + cx in double, rounded to float
  double C2[3];
  for (int i = 0; i < 3; i++) C2[i] = __dadd_rn(np_dot3(T2[3 * i], G.Ow1[0], T2[3 * i + 1], G.Ow1[1], T2[3 * i + 2], G.Ow1[2]), T2[9 + i]);
  G.ex = (float)__dadd_rn(__ddiv_rn(__dmul_rn(fx, C2[0]), C2[2]), cx);
  G.ey = (float)__dadd_rn(__ddiv_rn(__dmul_rn(fy, C2[1]), C2[2]), cy);
}

}  // namespace vo
