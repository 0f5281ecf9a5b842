// obs_walk.h -- the walk over one id's run of the observation index (kfstore.h: KfObsView), shared
// by the kernels that read "who holds this id": k_conn_count (connections.hip), the culling kernels (cull.hip), the local-BA
// window and write-back (local_ba_store.hip), the map-point upkeep (point_upkeep.hip) and the fusion (fuse.hip), which
// walks it through an overlay.
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

// ---- the walk through the overlay (kfstore.h: KfOverlay), by one WAVEFRONT: every entry that may
// carry the id whose run starts at slot p -- the frozen run of p, the frozen runs of the slots chained behind p, and the
// entries added to any of them in this call.  f(valid, entry) is called by all 64 lanes together (it may ballot); the
// caller validates an entry against the live feature word.  Every index read from memory is checked against its array, and
// both chains are cut after as many links as the arrays have entries.
template <class F>
__device__ __forceinline__ void obs_overlay_wave(const KfObsView &O, const KfOverlay &V, int p, F f) {
  const int lane = threadIdx.x & 63;
  int q = p;
  for (int links = 0; q >= 0 && q < O.n_keys && q < V.n_slots && links <= V.n_nodes; links++) {
    const unsigned rid = (unsigned)(O.keys[q] >> 32);
    for (int pos = q; pos < O.n_keys; pos += 64) {
      const int s = pos + lane;
      const unsigned long long key = s < O.n_keys ? O.keys[s] : ~0ull;
      const bool in = key != ~0ull && (unsigned)(key >> 32) == rid;
      f(in, (unsigned)(key & 0xffffffffu));
      if (__ballot(in) != ~0ull) break;
    }
    int node = V.a_head[q] - 1;
    for (int hops = 0; node >= 0 && node < V.n_nodes && hops < V.n_nodes; hops++) {
      f(lane == 0, (unsigned)V.node_entry[node]);
      node = V.node_next[node] - 1;
    }
    q = V.m_next[q] - 1;
  }
}

}  // namespace vo
