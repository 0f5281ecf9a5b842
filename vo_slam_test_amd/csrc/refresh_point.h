// refresh_point.h -- MapPoint::updateNormalAndDepth (mappoint.cpp:66-116) for one map point of the key-frame store, by one lane
// (DESIGN.md section 4k), shared by the local-BA write-back and refresh_points (k_ba_refresh, local_ba_store.hip) and the loop
// correction (k_lc_points, loop_correct.hip), so that the operation order stands in one place: holders ascending, bad ones
// included, `Ow = -(R^T t)`, every double operation rounded on its own, the ref_kf resolution, min / max in float.  The files
// that include it are compiled with -ffp-contract=off.
#pragma once
#include "kfstore.h"

#include "new_points_geom.h"
#include "obs_walk.h"

namespace vo {

// The point `id` at position p.  write_pos: p is the caller's new position and goes into every live feature that carries the
// id; else p is read from the store's row at the id's first live key.  A key is live iff its key-frame is not erased and its
// flags byte has bit 0 now (the index may be older than the flags).  The poses are the pose column's; a holder without one is
// left out of the sum and raises VO_KFSTORE_CONNECTIONS_INVALID.  -> the feature rows written (0: nobody holds the id).
__device__ __forceinline__ int refresh_point(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, int *ref_kf,
                                             double *normals, int *status, int id, double p[3], bool write_pos) {
  const int NK = S.NK, size = S.size;
  const int start = obs_lower_bound(O, id);
  auto live = [&](int kk, unsigned e) {
    return !X.erased[kk] && (kf_sec<uint8_t>(S, kk, S.o_flags)[e - (unsigned)kk * (unsigned)NK] & 1);
  };
  double sum[3] = {0, 0, 0};
  int r0 = -2, lowest = -1, cnt = 0;
  bool r0_holds = false, no_pose = false;
  double len_r0 = -1, len_low = -1;  // |p - Ow| of the two reference candidates (< 0: without a pose)
  int oct_r0 = 0, oct_low = 0;
  obs_run_holders(O, NK, size, start, id, live, [&](int kk, int f) {
    if (r0 == -2) {  // the first live key
      r0 = ref_kf[(size_t)kk * NK + f], lowest = kk;
      if (!write_pos) {
        const double *P = kf_sec<double>(S, kk, S.o_points) + 3 * (size_t)f;
        p[0] = P[0], p[1] = P[1], p[2] = P[2];
      }
    }
    double len = -1;
    if (*np_pose_set(M, kk)) {
      double Ow[3], d[3];
      np_center(np_pose(M, kk), Ow);
      for (int c = 0; c < 3; c++) d[c] = __dadd_rn(p[c], -Ow[c]);
      len = __dsqrt_rn(np_dot3(d[0], d[0], d[1], d[1], d[2], d[2]));
      for (int c = 0; c < 3; c++) sum[c] = __dadd_rn(sum[c], __ddiv_rn(d[c], len));
      cnt++;
    } else {
      no_pose = true;
    }
    const int oct = min(max(cull_octave(X, kk)[f], 0), 15);
    if (kk == lowest) len_low = len, oct_low = oct;
    if (kk == r0) r0_holds = true, len_r0 = len, oct_r0 = oct;
    return true;
  });
  if (no_pose) atomicOr(status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  if (lowest < 0) return 0;  // no holder: nothing to write
  const int ref = r0_holds ? r0 : lowest;  // (mappoint.cpp:350-351 under the ascending rule)
  const double len_ref = r0_holds ? len_r0 : len_low;
  const bool has_dist = len_ref >= 0, has_normal = cnt > 0;
  float maxd = 0.f, mind = 0.f;
  if (has_dist) {
    maxd = (float)len_ref * M.sf[r0_holds ? oct_r0 : oct_low];
    mind = maxd / M.sf[min(max(M.n_levels - 1, 0), 15)];
  }
  double nrm[3] = {0, 0, 0};
  if (has_normal)
    for (int c = 0; c < 3; c++) nrm[c] = __ddiv_rn(sum[c], (double)cnt);
  int rows = 0;
  obs_run_each(O, start, id, [&](unsigned e) {
    const int kk = (int)(e / (unsigned)NK);
    if (kk >= size || !live(kk, e)) return true;
    const int f = (int)(e - (unsigned)kk * (unsigned)NK);
    uint8_t *r = const_cast<uint8_t *>(S.base) + (size_t)kk * S.rec;
    if (write_pos) {
      double *pt = reinterpret_cast<double *>(r + S.o_points) + 3 * (size_t)f;
      pt[0] = p[0], pt[1] = p[1], pt[2] = p[2];
    }
    ref_kf[(size_t)kk * NK + f] = ref;
    if (has_normal) {
      double *nv = normals + ((size_t)kk * NK + f) * 3;
      nv[0] = nrm[0], nv[1] = nrm[1], nv[2] = nrm[2];
    }
    if (has_dist) reinterpret_cast<float *>(r + S.o_mind)[f] = mind, reinterpret_cast<float *>(r + S.o_maxd)[f] = maxd;
    rows++;
    return true;
  });
  return rows;
}

}  // namespace vo
