// obs_walk.h -- the walk over one id's run of the observation index (vo_common.h: KfObsView), shared
// by the kernels that read "who holds this id": k_conn_count (connections.hip), the culling kernels (cull.hip), the local-BA
// window and write-back (local_ba_store.hip) and the map-point upkeep (point_upkeep.hip).
#pragma once
#include "vo_common.h"

namespace vo {

// first key position whose id is >= `id` (id >= 0)
__device__ __forceinline__ int obs_lower_bound(const KfObsView &O, int id) {
  const unsigned long long first = (unsigned long long)(unsigned)id << 32;
  int lo = 0, hi = O.n_keys;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (O.keys[mid] < first) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// every key of id's run from position `start` (run[entry] of one of the id's entries) in ascending entry;
// f(entry) -> false ends the walk
template <class F>
__device__ __forceinline__ void obs_run_each(const KfObsView &O, int start, int id, F f) {
  for (int s = max(start, 0); s < O.n_keys; s++) {
    const unsigned long long key = O.keys[s];
    if ((int)(key >> 32) != id) break;
    if (!f((unsigned)(key & 0xffffffffu))) break;
  }
}

// the key-frames that hold id, ascending, each once at its OBSERVATION: its lowest-numbered entry that live(key-frame,
// entry) accepts (two features of one key-frame are one observation); f(key-frame, feature) -> false ends the walk
template <class Live, class F>
__device__ __forceinline__ void obs_run_holders(const KfObsView &O, int NK, int size, int start, int id, Live live, F f) {
  int prev = -1;
  obs_run_each(O, start, id, [&](unsigned e) {
    const int kk = (int)(e / (unsigned)NK);
    if (kk == prev || kk >= size || !live(kk, e)) return true;
    prev = kk;
    return f(kk, (int)(e - (unsigned)kk * (unsigned)NK));
  });
}

}  // namespace vo
