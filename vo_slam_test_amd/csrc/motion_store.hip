// motion_store.hip -- what a motion-tracked frame needs of the key-frame store between its two stages and behind them, on the
// device:
//   k_ms_gather   the slot ids of the frame from the last-frame list's ids (mappoints_[i] after cullingOutliersBeforeLocalMap),
//                 and the vote mask vo_tracker_build_local_map's kernels run on -- a temporary point of updateLastFrame holds a
//                 point and no id: it neither votes nor is nulled (visualOdometry.cpp:598-614)
//   k_ms_link     behind k_lm_points: the builder's nulling taken over into the tracker's slots, and `link` by id
//                 (handover_link.h, the rule of vo_tracker_begin_frame)
//   k_ms_stats    addVisible / addFound of trackLocalMap (:295-297, :738, :750-760) as three rows per frame
//   k_ms_record   Tcr = Tcw * ref^-1 with the reference key-frame's pose in the store (:130-140)
//   k_ms_refresh  last pose = Tcr * ref pose (updateLastFrame, :547-549)
// One workgroup per frame (the pose kernels: one thread).  The file's state is one block of its own; the tracker's arena, the
// hand-over block and every array the timed step touches stay where they are.  No atomic decides an order; no kernel waits on
// another workgroup; every loop is bounded by a count read once.
#include "tracker_state.h"

#include "handover_geom.h"
#include "handover_link.h"
#include "point_stats_rows.h"

#include <algorithm>
#include <new>

namespace vo {

struct MotionStore {
  Arena mem;
  int row = 0;  // max_features + max_local: a frame's row of the three counter arrays
  int P = 0;    // the power of two >= max(max_features, max_last): the link's keys of a frame (a host-set list holds max_last entries)
  unsigned long long *keys = nullptr;  // [B][P] where P > kHoLdsKeys, else unused (the keys live in LDS)
  int *first_ids = nullptr, *stat_ids = nullptr, *stat_visible = nullptr, *stat_found = nullptr, *ref_kf = nullptr;
  uint8_t *vote = nullptr;    // [B][cap] the builder's has-point column on the motion route: the slot holds an id
  double *ref_tcr = nullptr;  // [B][12]
};

void motion_store_destroy(MotionStore *m) { delete m; }

}  // namespace vo

namespace {

using namespace vo;

// the id of frame slot i when the local-map stage starts: the last entry the first search assigned, where the slot still holds
// its point after cullingOutliersBeforeLocalMap; -1: null, a temporary point, or beyond n.  Row pointers of one frame.
__device__ __forceinline__ int ms_slot_id(int i, int n, int n_last, const uint8_t *fhas, const int *assigned_first, const int *last_ids) {
  if (i >= n || !fhas[i]) return -1;
  const int a = assigned_first[i];
  if (a < 0 || a >= n_last) return -1;
  const int id = last_ids[a];
  return id < 0 ? -1 : id;
}

struct SlotArgs {
  int cap, n_last, nq_last, n_local, max_local, P;  // nq_last: the list's n -- its entries may lie beyond cap; P >= nq_last
  const int *fn;               // the frame store's counts [B]
  const int *assigned_first;   // [B][cap]
  uint8_t *fhas, *fobs;        // [B][cap]
  const int *last_ids;         // [B][n_last]
  const uint8_t *pf0;
  int *first_ids;              // [B][cap]
  uint8_t *vote;
  const int *ids1;             // the local map [B][n_local]
  int *link1;
  unsigned long long *gkeys;   // [B][P] where P > kHoLdsKeys
};

__global__ __launch_bounds__(256) void k_ms_gather(SlotArgs A) {
  const int f = blockIdx.x;
  const int n = min(max(A.fn[f], 0), A.cap);
  const size_t o = (size_t)f * A.cap, lo = (size_t)f * A.n_last;
  for (int i = threadIdx.x; i < A.cap; i += 256) {
    const int id = ms_slot_id(i, n, A.n_last, A.fhas + o, A.assigned_first + o, A.last_ids + lo);
    A.first_ids[o + i] = id, A.vote[o + i] = id >= 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_ms_link(SlotArgs A) {
  __shared__ unsigned long long s_keys[kHoLdsKeys];
  const int f = blockIdx.x;
  const int n = min(max(A.fn[f], 0), A.cap);
  const size_t o = (size_t)f * A.cap, lo = (size_t)f * A.n_last, mo = (size_t)f * A.n_local;
  // a slot that held an id and holds none now was nulled by the builder (:612): the tracker's slot follows (a thread reads the
  // byte it may write; nothing below reads it)
  for (int i = threadIdx.x; i < n; i += 256)
    if (A.first_ids[o + i] < 0 && ms_slot_id(i, n, A.n_last, A.fhas + o, A.assigned_first + o, A.last_ids + lo) >= 0)
      A.fhas[o + i] = 0, A.fobs[o + i] = 0;
  unsigned long long *keys = A.P <= kHoLdsKeys ? s_keys : A.gkeys + (size_t)f * A.P;
  ho_link_by_id(keys, A.nq_last, A.pf0 + lo, A.last_ids + lo, A.ids1 + mo, A.link1 + mo, A.max_local);  // every entry of the list
}

struct StatArgs {
  int cap, n_last, n_local, nq_local, max_local, row;
  const int *fn;
  const int *first_ids;        // or NULL: the local map was set by the host, the ids are gathered here
  const uint8_t *fhas, *foutl;
  const int *assigned_first, *assigned;
  const int *last_ids;
  const int *ids1;
  const uint8_t *q1_flags;
  int *ids, *visible, *found;  // [B][row]
};

__global__ __launch_bounds__(256) void k_ms_stats(StatArgs A) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(A.fn[f], 0), A.cap);
  const size_t o = (size_t)f * A.cap, lo = (size_t)f * A.n_last, mo = (size_t)f * A.n_local, r = (size_t)f * A.row, rb = r + A.cap;
  // ---- segment A: the slots as searchLocalMapPoints found them (:738), found where the slot kept its point as an inlier (:295-297)
  for (int i = tid; i < A.cap; i += 256) {
    int p = -1;
    if (i < n) p = A.first_ids ? A.first_ids[o + i] : ms_slot_id(i, n, A.n_last, A.fhas + o, A.assigned_first + o, A.last_ids + lo);
    if (p < 0) p = -1;
    A.ids[r + i] = p, A.visible[r + i] = p >= 0 ? 1 : 0;
    A.found[r + i] = (p >= 0 && A.assigned[o + i] < 0 && A.foutl[o + i] == 0) ? 1 : 0;
  }
  // ---- segment B: the local points (:750-760)
  ps_local_rows(n, A.nq_local, A.max_local, A.assigned + o, A.foutl + o, A.ids1 + mo, A.q1_flags + mo, A.ids + rb, A.visible + rb, A.found + rb);
}

struct PoseArgs {
  int B, size;
  KfMapView M;
  const int *src_ref;  // record: [B] the caller's key-frame numbers, or the builder's best key-frames
  const double *frame_pose;
  double *last_pose;
  const uint8_t *last_valid;
  double *ref_tcr;
  int *ref_kf;
};

__device__ __forceinline__ bool ms_ref_ok(const PoseArgs &A, int k) { return k >= 0 && k < A.size && *np_pose_set(A.M, k) != 0; }

__global__ __launch_bounds__(64) void k_ms_record(PoseArgs A) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= A.B) return;
  int ref = A.src_ref[f];
  if (!ms_ref_ok(A, ref)) ref = A.ref_kf[f];  // (:692-696: no voter keeps keyframe_trackRef_)
  if (!ms_ref_ok(A, ref) || !A.last_valid[f]) return;  // (:138-139: the previous pair stands)
  double Ri[12], T[12];
  ho_inverse(np_pose(A.M, ref), Ri);
  ho_compose(A.frame_pose + 12 * (size_t)f, Ri, T);
  for (int k = 0; k < 12; k++) A.ref_tcr[12 * (size_t)f + k] = T[k];
  A.ref_kf[f] = ref;
}

__global__ __launch_bounds__(64) void k_ms_refresh(PoseArgs A) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= A.B) return;
  const int ref = A.ref_kf[f];
  if (!ms_ref_ok(A, ref)) return;
  double T[12];
  ho_compose(A.ref_tcr + 12 * (size_t)f, np_pose(A.M, ref), T);
  for (int k = 0; k < 12; k++) A.last_pose[12 * (size_t)f + k] = T[k];
}

SlotArgs slot_args(vo_tracker *t) {
  const vo_tracker::Arrays &d = t->d;
  SlotArgs S{};
  S.cap = t->cap, S.n_last = t->n_last, S.nq_last = std::min(std::max(t->nq_last, 0), t->n_last), S.n_local = t->n_local;
  S.max_local = t->cfg.max_local, S.P = t->ms->P;
  S.fn = frame_store_view(t->frames).n, S.assigned_first = d.assigned_first, S.fhas = d.fhas, S.fobs = d.fobs;
  S.last_ids = t->ho->last_ids, S.pf0 = d.pf0, S.first_ids = t->ms->first_ids, S.vote = t->ms->vote;
  S.ids1 = d.ids1, S.link1 = d.link1, S.gkeys = t->ms->keys;
  return S;
}

// the mapping layer, the window, the block; everything is checked before anything is enqueued
int pose_call_ready(vo_tracker *t, const vo_kfstore *store, const char *W, bool before_begin) {
  if (!t || !store) return VO_ERR_INVALID;
  VO_CHECK(need(store, W, kLayerMapping));
  if (!t->ho || !t->handed_over || (before_begin && t->begun)) {
    set_error("%s: valid after vo_tracker_end_frame%s", W, before_begin ? ", before vo_tracker_begin_frame" : ", before the next track call or last-frame setter");
    return VO_ERR_INVALID;
  }
  return VO_OK;
}

PoseArgs pose_args(vo_tracker *t, const vo_kfstore *store) {
  PoseArgs A{};
  A.B = t->B, A.size = store->size, A.M = store->M;
  A.frame_pose = t->ho->frame_pose, A.last_pose = t->ho->last_pose, A.last_valid = t->ho->last_valid;
  A.ref_tcr = t->ms->ref_tcr, A.ref_kf = t->ms->ref_kf;
  return A;
}

}  // namespace

// the block, allocated by the first call that needs it
int vo::motion_store_ensure(vo_tracker *t) {
  if (t->ms) return VO_OK;
  MotionStore *m = new (std::nothrow) MotionStore();
  if (!m) {
    set_error("vo_tracker: out of host memory");
    return VO_ERR_HIP;
  }
  const size_t B = t->B, cap = t->cap;
  m->row = t->cap + std::max(t->cfg.max_local, 0);
  m->P = pow2_ceil(std::max(std::max(t->cap, t->n_last), 1));
  const size_t row = m->row;
  const int rc = m->mem.build(
      [&](Arena &a) {
        a.take(m->first_ids, B * cap * 4);
        a.take(m->vote, B * cap);
        a.take(m->stat_ids, B * row * 4);
        a.take(m->stat_visible, B * row * 4);
        a.take(m->stat_found, B * row * 4);
        a.take(m->ref_tcr, B * 96);
        a.take(m->ref_kf, B * 4);
        a.take(m->keys, m->P > kHoLdsKeys ? B * (size_t)m->P * 8 : 0);
      },
      "vo_tracker (motion route from the store)");
  if (rc != VO_OK) {
    delete m;
    return rc;
  }
  // no ids, no counts, no remembered key-frame: zeros, and -1 in the id arrays
  if (hipMemsetAsync(m->mem.block, 0, m->mem.bytes, t->st) != hipSuccess ||
      hipMemsetAsync(m->first_ids, 0xff, B * cap * 4, t->st) != hipSuccess ||
      hipMemsetAsync(m->stat_ids, 0xff, B * row * 4, t->st) != hipSuccess ||
      hipMemsetAsync(m->ref_kf, 0xff, B * 4, t->st) != hipSuccess || hipStreamSynchronize(t->st) != hipSuccess) {
    delete m;
    set_error("vo_tracker (motion route from the store): clearing the block failed");
    return VO_ERR_HIP;
  }
  t->ms = m;
  return VO_OK;
}

int vo::motion_store_slot_ids(vo_tracker *t, LocalMapArgs *A, hipStream_t st) {
  hipLaunchKernelGGL(k_ms_gather, dim3(t->B), dim3(256), 0, st, slot_args(t));
  VO_HIP_CHECK(hipGetLastError());
  A->sid = t->ms->first_ids, A->fhas = t->ms->vote, A->fobs = t->ms->vote;
  return VO_OK;
}

int vo::motion_store_link(vo_tracker *t, hipStream_t st) {
  hipLaunchKernelGGL(k_ms_link, dim3(t->B), dim3(256), 0, st, slot_args(t));
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

void vo::motion_store_stat_rows(const vo_tracker *t, int **ids, int **visible, int **found, int *row) {
  *ids = t->ms->stat_ids, *visible = t->ms->stat_visible, *found = t->ms->stat_found, *row = t->ms->row;
}

const void *vo::motion_store_selector(const vo_tracker *t, int what, size_t *bytes) {
  const MotionStore *m = t->ms;
  if (!m) return nullptr;
  const size_t B = t->B;
  switch (what) {
    case VO_TRACKER_FIRST_SLOT_IDS: *bytes = B * (size_t)t->cap * 4; return m->first_ids;
    case VO_TRACKER_STAT_IDS: *bytes = B * (size_t)m->row * 4; return m->stat_ids;
    case VO_TRACKER_STAT_VISIBLE: *bytes = B * (size_t)m->row * 4; return m->stat_visible;
    case VO_TRACKER_STAT_FOUND: *bytes = B * (size_t)m->row * 4; return m->stat_found;
    case VO_TRACKER_REF_TCR: *bytes = B * 96; return m->ref_tcr;
    case VO_TRACKER_REF_KF: *bytes = B * 4; return m->ref_kf;
    default: return nullptr;
  }
}

extern "C" {

int vo_tracker_point_stats(vo_tracker *t) {
  if (!t) return VO_ERR_INVALID;
  // everything is checked before anything is enqueued
  if (!t->have_result || t->last_run != (kRunFront | kRunMotion | kRunLocal) || !t->local_split) {
    set_error("vo_tracker_point_stats: valid after vo_tracker_track_first[_dev] + vo_tracker_track_local_map");
    return VO_ERR_INVALID;
  }
  if (!t->have_local || !t->have_ids || !t->have_last_ids || !t->ho || t->cfg.max_local < 1) {
    set_error("vo_tracker_point_stats: the local map and the last-frame list must both carry map-point ids");
    return VO_ERR_INVALID;
  }
  VO_CHECK(motion_store_ensure(t));
  const vo_tracker::Arrays &d = t->d;
  const MotionStore &m = *t->ms;
  StatArgs A{};
  A.cap = t->cap, A.n_last = t->n_last, A.n_local = t->n_local, A.nq_local = std::min(t->nq_local, t->cfg.max_local);
  A.max_local = t->cfg.max_local, A.row = m.row;
  A.fn = frame_store_view(t->frames).n;
  A.first_ids = t->lm_motion ? m.first_ids : nullptr;
  A.fhas = d.fhas, A.foutl = d.foutl, A.assigned_first = d.assigned_first, A.assigned = d.assigned;
  A.last_ids = t->ho->last_ids, A.ids1 = d.ids1, A.q1_flags = d.q1_flags;
  A.ids = m.stat_ids, A.visible = m.stat_visible, A.found = m.stat_found;
  hipLaunchKernelGGL(k_ms_stats, dim3(t->B), dim3(256), 0, t->st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_tracker_point_stats_arrays(vo_tracker *t, const int32_t **dev_ids, const int32_t **dev_visible, const int32_t **dev_found, int32_t *row_len) {
  if (!t) return VO_ERR_INVALID;
  VO_CHECK(motion_store_ensure(t));
  if (dev_ids) *dev_ids = t->ms->stat_ids;
  if (dev_visible) *dev_visible = t->ms->stat_visible;
  if (dev_found) *dev_found = t->ms->stat_found;
  if (row_len) *row_len = t->ms->row;
  return VO_OK;
}

int vo_tracker_record_ref_pose(vo_tracker *t, const vo_kfstore *store, const int32_t *dev_ref_kf) {
  VO_CHECK(pose_call_ready(t, store, "vo_tracker_record_ref_pose", false));
  if (!dev_ref_kf && !t->lm.best) {
    set_error("vo_tracker_record_ref_pose: no dev_ref_kf, and vo_tracker_build_local_map has left no VO_TRACKER_LOCAL_REF_KF");
    return VO_ERR_INVALID;
  }
  VO_CHECK(motion_store_ensure(t));
  PoseArgs A = pose_args(t, store);
  A.src_ref = dev_ref_kf ? dev_ref_kf : t->lm.best;
  VO_CHECK(kfstore_order_before(store, t->st));
  hipLaunchKernelGGL(k_ms_record, dim3((t->B + 63) / 64), dim3(64), 0, t->st, A);
  VO_HIP_CHECK(hipGetLastError());
  return kfstore_order_after(store, t->st);
}

int vo_tracker_refresh_last_pose(vo_tracker *t, const vo_kfstore *store) {
  VO_CHECK(pose_call_ready(t, store, "vo_tracker_refresh_last_pose", true));
  VO_CHECK(motion_store_ensure(t));
  const PoseArgs A = pose_args(t, store);
  VO_CHECK(kfstore_order_before(store, t->st));
  hipLaunchKernelGGL(k_ms_refresh, dim3((t->B + 63) / 64), dim3(64), 0, t->st, A);
  VO_HIP_CHECK(hipGetLastError());
  return kfstore_order_after(store, t->st);
}

}  // extern "C"
