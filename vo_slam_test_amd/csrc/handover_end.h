// handover_end.h -- the steps of frame_last_ = frame_curr_ that do not depend on where a slot's map point comes from
// (visualOdometry.cpp:87-128): the pose side -- the frame's pose, Tcl_ = Tcw * Tlw^-1, the verdict (:94-103, :115-118) -- and
// cullingOutliersOfFrame with the frame written as the last-frame list (:888-895, :128).  k_ho_end (handover.hip, the motion
// route) and k_hs_end (handover_store.hip, the relocalisation and reference-key-frame routes from the key-frame store) are these
// two functions around their own slot rule.
#pragma once
#include "handover_geom.h"

namespace vo {

// One thread per frame.  pose6: the frame's se3; ok: the route's verdict (status 0 and enough tracked points).  The pointers are
// the frame's own rows: frame_pose, velocity, last_pose [12], last_valid, motion_state [1].
__device__ __forceinline__ void ho_end_pose(const double *pose6, bool ok, double *frame_pose, double *velocity, double *last_pose,
                                            uint8_t *last_valid, int *motion_state) {
  double T[12], V[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  ho_pose12(ba::se3_exp(pose6), T);
  const bool moving = ok && *last_valid != 0;
  if (moving) {
    double Li[12];
    ho_inverse(last_pose, Li);
    ho_compose(T, Li, V);
  }
  for (int k = 0; k < 12; k++) frame_pose[k] = T[k], velocity[k] = V[k], last_pose[k] = T[k];
  *motion_state = moving ? 1 : 0;
  *last_valid = ok ? 1 : 0;
}

// Every thread of a workgroup of 256 calls it for the same frame, behind a barrier that follows the slot rule: a thread reads
// back the slots it wrote.  slot_*, octave, angle, fpoint: the frame's rows of max_features entries (n of them features); p0 ..
// last_ids: its rows of the last-frame list (n_last entries, n_last >= max_features).
__device__ __forceinline__ void ho_end_list(int n, int n_last, const uint8_t *slot_flags, const int *slot_ids, const uint8_t *slot_desc,
                                            const int *octave, const float *angle, const double *fpoint, double *p0, uint8_t *pf0,
                                            int *q0_level, float *q0_angle, uint8_t *q0_desc, int *last_ids) {
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (int i = threadIdx.x; i < n_last; i += 256) {
    uint8_t flags = 0;
    int id = -1, oct = 0;
    float ang = 0.f;
    double p[3] = {0, 0, 0};
    uint4 d0 = zero, d1 = zero;
    if (i < n) {
      flags = slot_flags[i], oct = octave[i], ang = angle[i];
      if (flags) {
        id = slot_ids[i];
        const uint4 *src = reinterpret_cast<const uint4 *>(slot_desc) + 2 * (size_t)i;
        d0 = src[0], d1 = src[1];
        for (int c = 0; c < 3; c++) p[c] = fpoint[3 * (size_t)i + c];
      }
    }
    pf0[i] = flags, last_ids[i] = id, q0_level[i] = oct, q0_angle[i] = ang;
    for (int c = 0; c < 3; c++) p0[3 * (size_t)i + c] = p[c];
    uint4 *dst = reinterpret_cast<uint4 *>(q0_desc) + 2 * (size_t)i;
    dst[0] = d0, dst[1] = d1;
  }
}

}  // namespace vo
