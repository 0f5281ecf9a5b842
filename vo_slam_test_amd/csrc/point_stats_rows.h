// point_stats_rows.h -- the local points' half of a frame's addVisible / addFound rows (visualOdometry.cpp:750-760, :295-297):
// segment B of vo_tracker_point_stats (k_ms_stats, motion_store.hip) and of vo_tracker_point_stats_store (k_hs_stats,
// handover_store.hip) is this one function.
#pragma once
#include "vo_common.h"

namespace vo {

// Every thread of a workgroup of 256 calls it for the same frame.  assigned, foutl: the frame's rows of the n feature slots
// (the local point a slot claimed, the second solve's outliers); ids1, q1_flags: its rows of the local map (nq_local entries,
// bit 0 of q1_flags: Frame::isInFrame accepted the point); ids, visible, found: the max_local entries of its three rows behind
// the slots' segment.  A local point is claimed by at most one slot: plain stores.  found is 1 iff the claiming slot is no
// outlier; a point neither visible nor found carries the id -1.
__device__ __forceinline__ void ps_local_rows(int n, int nq_local, int max_local, const int *assigned, const uint8_t *foutl, const int *ids1,
                                              const uint8_t *q1_flags, int *ids, int *visible, int *found) {
  const int tid = threadIdx.x;
  for (int j = tid; j < max_local; j += 256) found[j] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int a = assigned[i];
    if (a >= 0 && a < max_local && foutl[i] == 0) found[a] = 1;
  }
  __syncthreads();
  for (int j = tid; j < max_local; j += 256) {
    int id = j < nq_local ? ids1[j] : -1;
    int vis = 0, fnd = 0;
    if (id >= 0) vis = q1_flags[j] & 1, fnd = found[j];
    if (!vis && !fnd) id = -1;
    ids[j] = id, visible[j] = vis, found[j] = fnd;
  }
}

}  // namespace vo
