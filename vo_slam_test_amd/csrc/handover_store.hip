// handover_store.hip -- frame_last_ = frame_curr_ and the addVisible / addFound rows behind the two routes of
// VisualOdometry::run that keep their slot ids in the key-frame store: a relocalisation from the store
// (vo_tracker_relocalize_store / _db) and trackRefKeyFrame from the store (first stage only), each followed by
// vo_tracker_build_local_map and vo_tracker_track_local_map.
//   k_hs_end    one workgroup per frame: the slot's map-point id from the route's source, its descriptor from the store at the
//               id's first key of the observation index, cullingTempMapPoints, then -- behind a barrier -- the steps k_ho_end
//               shares (handover_end.h: the pose side, cullingOutliersOfFrame, the frame written as the last-frame list)
//   k_hs_stats  one workgroup per frame: segment A from the same source, segment B as on the motion route (point_stats_rows.h)
// They write the hand-over block (handover.hip) and the counter rows of motion_store.hip's block; the file has no state of its
// own.  No atomic decides an order; no kernel waits on another workgroup; every loop is bounded by a count read once.
#include "tracker_state.h"

#include "handover_end.h"
#include "obs_walk.h"
#include "point_stats_rows.h"

#include <algorithm>

namespace {

using namespace vo;

// where a slot's map point comes from.  route 1 (relocalisation): the frame's id array, which the walk filled from the winner
// key-frame and k_reloc_local_gather from the local map; winner < 0: the relocalisation failed.  route 2 (reference key-frame):
// the store's ids of key-frame ref_kf[f] at the first search's match.
struct SlotSource {
  int route, cap, n_local;
  KfStoreView S;
  KfObsView O;
  const int *fn;              // the frame store's counts [B]
  const uint8_t *fhas;        // [B][cap]
  const int *assigned;        // [B][cap] the local search's claims
  const int *assigned_first;  // [B][cap] route 2
  const int *ref_kf;          // [B] route 2
  const int *fid, *winner;    // [B][cap], [B] route 1
  const int *ids1;            // the local map [B][n_local]
};

__device__ __forceinline__ bool hs_failed(const SlotSource &Q, int f) { return Q.route == 1 && Q.winner[f] < 0; }

// the features of route 2's reference key-frame (0: a number outside the store)
__device__ __forceinline__ int hs_ref_count(const SlotSource &Q, int f, int *rk) {
  if (Q.route != 2) return *rk = -1, 0;
  const int k = Q.ref_kf[f];
  *rk = k;
  return k >= 0 && k < Q.S.size ? min(max(kf_head(Q.S, k)[0], 0), Q.S.NK) : 0;
}

// the id of non-null slot i as the route left it before the local search, -1: null or without an id
__device__ __forceinline__ int hs_kept_id(const SlotSource &Q, size_t o, int i, int rk, int rn) {
  if (!Q.fhas[o + i]) return -1;
  int id = -1;
  if (Q.route == 1) {
    id = Q.fid[o + i];
  } else {
    const int a0 = Q.assigned_first[o + i];
    if (a0 >= 0 && a0 < rn) id = kf_sec<int>(Q.S, rk, Q.S.o_ids)[a0];
  }
  return id < 0 ? -1 : id;
}

// mp->descriptor_: the store's point descriptor at the id's first key, the lowest (key-frame, feature) that holds it below size;
// false: nobody holds the id
__device__ __forceinline__ bool hs_point_desc(const SlotSource &Q, int id, uint4 *d0, uint4 *d1) {
  const int s = obs_lower_bound(Q.O, id);
  if (s >= Q.O.n_keys) return false;
  const unsigned long long key = Q.O.keys[s];
  if (key == ~0ull || (int)(key >> 32) != id) return false;
  const unsigned e = (unsigned)(key & 0xffffffffu);
  const int k = (int)(e / (unsigned)Q.S.NK);
  if (k >= Q.S.size) return false;  // (ascending entries: every later holder lies beyond size too)
  const uint4 *src = kf_sec<uint4>(Q.S, k, Q.S.o_pdesc) + 2 * (size_t)(e - (unsigned)k * (unsigned)Q.S.NK);
  *d0 = src[0], *d1 = src[1];
  return true;
}

struct EndArgs {
  SlotSource Q;
  int n_last, min_tracked;
  const uint8_t *fobs, *foutl;  // [B][cap]
  const double *fpoint;
  const int *octave;            // the frame store's columns [B][cap]
  const float *angle;
  const uint8_t *resblk;        // the result block: 72 bytes per frame -- pose (6 doubles), n_tracked, ..., status (5th int)
  double *p0;                   // the last-frame list [B][n_last]: rewritten
  uint8_t *pf0;
  int *q0_level;
  float *q0_angle;
  uint8_t *q0_desc;
  int *last_ids;
  int *slot_ids;                // [B][cap]
  uint8_t *slot_desc, *slot_flags;
  double *frame_pose, *velocity, *last_pose;
  uint8_t *last_valid;
  int *motion_state;
};

__global__ __launch_bounds__(256) void k_hs_end(EndArgs A) {
  const SlotSource &Q = A.Q;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(Q.fn[f], 0), Q.cap);
  const size_t o = (size_t)f * Q.cap, lo = (size_t)f * A.n_last, mo = (size_t)f * Q.n_local;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  const bool failed = hs_failed(Q, f);
  // ---- the pose side (:87-118); the verdict is what vo_tracker_results reports
  if (tid == 0) {
    const uint8_t *rec = A.resblk + (size_t)f * 72;
    const int *pi = reinterpret_cast<const int *>(rec + 48);
    const bool ok = !failed && pi[4] == 0 && pi[0] >= A.min_tracked;
    ho_end_pose(reinterpret_cast<const double *>(rec), ok, A.frame_pose + 12 * (size_t)f, A.velocity + 12 * (size_t)f,
                A.last_pose + 12 * (size_t)f, A.last_valid + f, A.motion_state + f);
  }
  // ---- the slots as createNewKeyFrame sees them
  int rk;
  const int rn = hs_ref_count(Q, f, &rk);
  for (int i = tid; i < Q.cap; i += 256) {
    int id = -1;
    uint4 d0 = zero, d1 = zero;
    uint8_t flags = 0;
    if (i < n && !failed) {
      const int a1 = Q.assigned[o + i];
      if (Q.route == 2 && a1 >= 0) id = a1 < Q.n_local ? Q.ids1[mo + a1] : -1;  // (route 1: k_reloc_local_gather wrote it into fid)
      else id = hs_kept_id(Q, o, i, rk, rn);
      // (:848: an unobserved point is a temporary one; an id nobody holds is a bad point: both slots are handed over null)
      if (id >= 0 && A.fobs[o + i] && hs_point_desc(Q, id, &d0, &d1)) flags = A.foutl[o + i] ? 2 : 3;
      else id = -1, d0 = zero, d1 = zero;
    }
    A.slot_ids[o + i] = id, A.slot_flags[o + i] = flags;
    uint4 *dst = reinterpret_cast<uint4 *>(A.slot_desc) + 2 * (o + i);
    dst[0] = d0, dst[1] = d1;
  }
  __syncthreads();  // (the pose side has read the old last pose; a thread reads back the slots it wrote)
  ho_end_list(n, A.n_last, A.slot_flags + o, A.slot_ids + o, A.slot_desc + 32 * o, A.octave + o, A.angle + o, A.fpoint + 3 * o, A.p0 + 3 * lo,
              A.pf0 + lo, A.q0_level + lo, A.q0_angle + lo, A.q0_desc + 32 * lo, A.last_ids + lo);
}

struct StatArgs {
  SlotSource Q;
  int nq_local, max_local, row;
  const uint8_t *foutl;         // [B][cap]
  const uint8_t *q1_flags;      // [B][n_local] the flags Frame::isInFrame ran with and wrote
  int *ids, *visible, *found;   // [B][row]
};

__global__ __launch_bounds__(256) void k_hs_stats(StatArgs A) {
  const SlotSource &Q = A.Q;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(Q.fn[f], 0), Q.cap);
  const size_t o = (size_t)f * Q.cap, mo = (size_t)f * Q.n_local, r = (size_t)f * A.row, rb = r + Q.cap;
  if (hs_failed(Q, f)) {  // (uniform: the frame took no part in the local stage)
    for (int j = tid; j < A.row; j += 256) A.ids[r + j] = -1, A.visible[r + j] = 0, A.found[r + j] = 0;
    return;
  }
  // ---- segment A: the slots searchLocalMapPoints found occupied (:738), found where the slot is an inlier (:295-297)
  int rk;
  const int rn = hs_ref_count(Q, f, &rk);
  for (int i = tid; i < Q.cap; i += 256) {
    int p = -1;
    if (i < n && Q.assigned[o + i] < 0) p = hs_kept_id(Q, o, i, rk, rn);
    A.ids[r + i] = p, A.visible[r + i] = p >= 0 ? 1 : 0;
    A.found[r + i] = (p >= 0 && A.foutl[o + i] == 0) ? 1 : 0;
  }
  // ---- segment B: the local points (:750-760)
  ps_local_rows(n, A.nq_local, A.max_local, Q.assigned + o, A.foutl + o, Q.ids1 + mo, A.q1_flags + mo, A.ids + rb, A.visible + rb, A.found + rb);
}

// what both calls ask: the route, this frame's map built from the store, the local stage behind it
int store_call_ready(vo_tracker *t, const vo_kfstore *store, const char *W) {
  if (!t || !store) return VO_ERR_INVALID;
  const unsigned r = t->last_run;
  const bool reloc = t->ids_route == 1 && r == (kRunFront | kRunReloc);
  const bool ref = t->ids_route == 2 && r == (kRunFront | kRunRefStore | kRunLocal);
  if (!t->have_result || !(reloc || ref) || t->lm_route != t->ids_route || !t->local_ran || !t->have_local || !t->have_ids ||
      t->cfg.max_local < 1) {
    set_error("%s: valid after vo_tracker_relocalize_store / _db or vo_tracker_track_ref_keyframe_store (first_stage_only = 1), each "
              "followed by vo_tracker_build_local_map and vo_tracker_track_local_map",
              W);
    return VO_ERR_INVALID;
  }
  return VO_OK;
}

// the views and the ordering against the store's stream, as vo_tracker_build_local_map takes them; everything that can be
// refused has been checked before
int slot_source(vo_tracker *t, vo_kfstore *store, SlotSource *Q) {
  const vo_tracker::Arrays &d = t->d;
  Q->route = t->ids_route, Q->cap = t->cap, Q->n_local = t->n_local;
  Q->fn = frame_store_view(t->frames).n;
  Q->fhas = d.fhas, Q->assigned = d.assigned, Q->assigned_first = d.assigned_first, Q->ref_kf = d.ref_kf, Q->ids1 = d.ids1;
  if (Q->route == 1) {
    int *fid = nullptr;
    VO_CHECK(reloc_frame_ids(t->reloc, &fid, &Q->winner));
    Q->fid = fid;
  }
  VO_CHECK(kfstore_obs_view(store, &Q->O));  // (rebuilds the observation index on the store's stream when it is stale)
  Q->S = kfstore_view(store);
  return kfstore_order_before(store, t->st);
}

}  // namespace

extern "C" {

int vo_tracker_end_frame_store(vo_tracker *t, vo_kfstore *store, const vo_tracker_handover_params *p) {
  if (!p) return VO_ERR_INVALID;
  // everything is checked before anything is enqueued
  VO_CHECK(store_call_ready(t, store, "vo_tracker_end_frame_store"));
  if (t->cap > t->n_last) {
    set_error("vo_tracker_end_frame_store: %d feature slots per frame, the last-frame list holds %d (max_last)", t->cap, t->n_last);
    return VO_ERR_CAPACITY;
  }
  VO_CHECK(handover_ensure(t));
  const vo_tracker::Arrays &d = t->d;
  const Handover &h = *t->ho;
  const FrameStoreView F = frame_store_view(t->frames);
  EndArgs A{};
  VO_CHECK(slot_source(t, store, &A.Q));
  A.n_last = t->n_last, A.min_tracked = p->min_tracked > 0 ? p->min_tracked : 30;
  A.fobs = d.fobs, A.foutl = d.foutl, A.fpoint = d.fpoint, A.octave = F.octave, A.angle = F.angle, A.resblk = d.resblk;
  A.p0 = d.p0, A.pf0 = d.pf0, A.q0_level = d.q0_level, A.q0_angle = d.q0_angle, A.q0_desc = d.q0_desc, A.last_ids = h.last_ids;
  A.slot_ids = h.slot_ids, A.slot_desc = h.slot_desc, A.slot_flags = h.slot_flags;
  A.frame_pose = h.frame_pose, A.velocity = h.velocity, A.last_pose = h.last_pose, A.last_valid = h.last_valid;
  A.motion_state = h.motion_state;
  hipLaunchKernelGGL(k_hs_end, dim3(t->B), dim3(256), 0, t->st, A);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(kfstore_order_after(store, t->st));
  t->nq_last = t->cap;  // entry i is slot i
  t->have_last_ids = true, t->handed_over = true, t->begun = false;
  return VO_OK;
}

int vo_tracker_point_stats_store(vo_tracker *t, vo_kfstore *store) {
  VO_CHECK(store_call_ready(t, store, "vo_tracker_point_stats_store"));
  VO_CHECK(motion_store_ensure(t));
  StatArgs A{};
  VO_CHECK(slot_source(t, store, &A.Q));
  A.nq_local = std::min(t->nq_local, t->cfg.max_local), A.max_local = t->cfg.max_local;
  A.foutl = t->d.foutl, A.q1_flags = t->d.q1_flags;
  motion_store_stat_rows(t, &A.ids, &A.visible, &A.found, &A.row);
  hipLaunchKernelGGL(k_hs_stats, dim3(t->B), dim3(256), 0, t->st, A);
  VO_HIP_CHECK(hipGetLastError());
  return kfstore_order_after(store, t->st);
}

}  // extern "C"
