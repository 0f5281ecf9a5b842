// keyframe_geom.h -- the arithmetic of a map point created with its key-frame (keyframe_create.hip):
// Camera::pixel2camera (camera.cpp:87-95), T_c_w.inverse() * p (:82-85) and, for the point's one holder,
// MapPoint::updateNormalAndDepth (mappoint.cpp:66-116) in the operation order k_ba_refresh (local_ba_store.hip) runs it.  Every
// operation is an explicitly rounded float or double operation in the order written here, so that
// tests/keyframe_create_ref.py reproduces every byte and a later vo_kfstore_refresh_points changes none.
#pragma once
#include "new_points_geom.h"

namespace vo {

// x = ((u - cx) * d) / fx, y = ((v - cy) * d) / fy in float, every operation rounded; z = d; widened to double
__device__ __forceinline__ void kc_pixel2camera(const float *cam, float u, float v, float d, double pc[3]) {
  pc[0] = (double)__fdiv_rn(__fmul_rn(__fsub_rn(u, cam[2]), d), cam[0]);
  pc[1] = (double)__fdiv_rn(__fmul_rn(__fsub_rn(v, cam[3]), d), cam[1]);
  pc[2] = (double)d;
}

// p_w = R^T (p_c - t): q = p_c + (-t), p_w[i] = (R[0][i] q[0] + R[1][i] q[1]) + R[2][i] q[2].  T: R row-major (9) then t (3).
__device__ __forceinline__ void kc_camera2world(const double *T, const double pc[3], double pw[3]) {
  double q[3];
  for (int c = 0; c < 3; c++) q[c] = __dadd_rn(pc[c], -T[9 + c]);
  for (int i = 0; i < 3; i++) pw[i] = np_dot3(T[i], q[0], T[3 + i], q[1], T[6 + i], q[2]);
}

// updateNormalAndDepth with T's key-frame as the only holder and the reference: Ow = np_center(T), d = p + (-Ow),
// len = sqrt((d0 d0 + d1 d1) + d2 d2), normal = (0 + d / len) / 1 (the sum over one holder, then its mean),
// max = (float)len * sf_level, min = max / sf_last
__device__ __forceinline__ void kc_single_view(const double *T, const double p[3], float sf_level, float sf_last, double nrm[3], float &mind,
                                               float &maxd) {
  double Ow[3], d[3];
  np_center(T, Ow);
  for (int c = 0; c < 3; c++) d[c] = __dadd_rn(p[c], -Ow[c]);
  const double len = __dsqrt_rn(np_dot3(d[0], d[0], d[1], d[1], d[2], d[2]));
  for (int c = 0; c < 3; c++) nrm[c] = __ddiv_rn(__dadd_rn(0.0, __ddiv_rn(d[c], len)), 1.0);
  maxd = __fmul_rn((float)len, sf_level);
  mind = __fdiv_rn(maxd, sf_last);
}

}  // namespace vo
