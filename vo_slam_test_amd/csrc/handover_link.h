// handover_link.h -- `link` by map-point id (visualOdometry.cpp:765 through the ids): for every local point the lowest
// last-frame index that carries its id with bit 0 set, or -1.  Step 3 of vo_tracker_begin_frame (handover.hip) and the last step
// of vo_tracker_build_local_map on the motion route (motion_store.hip) are this one function.
#pragma once
#include "block_sort.h"

namespace vo {

// Every thread of a workgroup of 256 calls it for the same frame.  keys: pow2_ceil(n_entries) words in LDS or in device memory
// that only this workgroup touches.  pf0, last_ids: the frame's rows of the last-frame list, n_entries = the list's n (behind
// vo_tracker_end_frame that is max_features; a list the host set may hold up to max_last); ids1, link1: its rows of the local map
// (nq_local entries).  The last entries' (id << 32 | index) are sorted, each local point takes a lower bound: the id's lowest
// index.  The caller puts a barrier between its own writes of pf0 / last_ids and this call.
__device__ __forceinline__ void ho_link_by_id(unsigned long long *keys, int n_entries, const uint8_t *pf0, const int *last_ids,
                                              const int *ids1, int *link1, int nq_local) {
  const int tid = threadIdx.x;
  const int P = pow2_ceil(max(n_entries, 1));
  for (int i = tid; i < P; i += 256) {
    unsigned long long key = ~0ull;
    if (i < n_entries && (pf0[i] & 1)) {
      const int id = last_ids[i];
      if (id >= 0) key = ((unsigned long long)(unsigned)id << 32) | (unsigned)i;
    }
    keys[i] = key;
  }
  block_bitonic_sort(keys, P);
  for (int j = tid; j < nq_local; j += 256) {
    const int id = ids1[j];
    int lk = -1;
    if (id >= 0) {
      const unsigned long long want = (unsigned long long)(unsigned)id << 32;
      int lo_ = 0, hi = P;  // the first key >= want: the id's lowest index
      while (lo_ < hi) {
        const int mid = (lo_ + hi) >> 1;
        if (keys[mid] < want) lo_ = mid + 1;
        else hi = mid;
      }
      if (lo_ < P && keys[lo_] != ~0ull && (int)(keys[lo_] >> 32) == id) lk = (int)(keys[lo_] & 0xffffffffu);
    }
    link1[j] = lk;
  }
}

}  // namespace vo
