// handover.hip -- frame_last_ = frame_curr_ on the device: what VisualOdometry::run does between two
// frames (visualOdometry.cpp:80-128) and the preamble of trackWithMotion (:233-236), for every frame of a tracker's batch.
//   k_ho_end    one workgroup per frame: the slot rule of examples/vo_run_hip.cpp:279-281 (local over last), cullingTempMapPoints
//               (:844-853), the verdict, Tcl_ = Tcw * Tlw^-1 (:94-103, :115-118), then -- behind a barrier, the reads of the old
//               list being done -- cullingOutliersOfFrame (:888-895) and the frame written as the last-frame list (:128).  The pose
//               side and the list rewrite are handover_end.h's, shared with handover_store.hip.
//   k_ho_begin  one workgroup per frame: updateLastFrame's temporary points (:555-592) as k_kc_walk's walk -- the pairs
//               (depth bits << 32 | feature) sorted by block_bitonic_sort in LDS (up to kHoLdsKeys keys, else in the block), the
//               inclusive count C_j by wave ballots, the first j with d_j > th_depth && C_j > 100 --, the start pose
//               Tcl_ * Tlw (:236) with its logarithm, and `link` by id: the last entries' (id << 32 | index) sorted, a lower
//               bound per local point (handover_link.h, shared with motion_store.hip).
// They write the arrays vo_tracker_set_last_frame fills from the host; the tracker's arena and every array the timed step
// touches stay where they are, and the state of this file is one block of its own.  No atomic decides an order; no kernel waits
// on another workgroup; every loop is bounded by a count read once.
#include "tracker_state.h"

#include "block_sort.h"
#include "handover_end.h"
#include "handover_geom.h"
#include "handover_link.h"

#include <algorithm>
#include <new>

namespace vo {

void handover_destroy(Handover *h) { delete h; }

}  // namespace vo

namespace {

using namespace vo;

struct EndArgs {
  int cap, n_last, n_local;
  const int *fn;                          // the frame store's counts [B]
  const int *assigned_first, *assigned;   // [B][cap]
  const uint8_t *fhas, *fobs, *foutl;     // foutl NULL: the local-map stage did not run
  const double *fpoint;
  const uint8_t *q1_desc;                 // the local map [B][n_local]
  const int *ids1;                        // or NULL: no ids
  int have_last_ids;
  const int *octave;                      // the frame store's columns [B][cap]
  const float *angle;
  const double *pose6;
  const int *status, *ntracked;
  int min_tracked;
  double *p0;                             // the last-frame list [B][n_last]: read (descriptors, ids), then rewritten
  uint8_t *pf0;
  int *q0_level;
  float *q0_angle;
  uint8_t *q0_desc;
  int *last_ids;
  int *slot_ids;                          // [B][cap]
  uint8_t *slot_desc, *slot_flags;
  double *frame_pose, *velocity, *last_pose;
  uint8_t *last_valid;
  int *motion_state;
};

__global__ __launch_bounds__(256) void k_ho_end(EndArgs A) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(A.fn[f], 0), A.cap);
  const size_t o = (size_t)f * A.cap, lo = (size_t)f * A.n_last, mo = (size_t)f * A.n_local;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  // ---- the pose side (:87-118)
  if (tid == 0) {
    const bool ok = A.status[f] == 0 && A.ntracked[f] >= A.min_tracked;
    ho_end_pose(A.pose6 + 6 * (size_t)f, ok, A.frame_pose + 12 * (size_t)f, A.velocity + 12 * (size_t)f, A.last_pose + 12 * (size_t)f,
                A.last_valid + f, A.motion_state + f);
  }
  // ---- the slots as createNewKeyFrame sees them (steps 1 and 2)
  for (int i = tid; i < A.cap; i += 256) {
    int id = -1;
    uint4 d0 = zero, d1 = zero;
    uint8_t flags = 0;
    if (i < n) {
      const int a1 = A.assigned[o + i], a0 = A.assigned_first[o + i];
      const uint4 *src = nullptr;
      if (a1 >= 0) {
        src = reinterpret_cast<const uint4 *>(A.q1_desc) + 2 * (mo + a1);
        if (A.ids1) id = A.ids1[mo + a1];
      } else if (a0 >= 0 && A.fhas[o + i]) {
        src = reinterpret_cast<const uint4 *>(A.q0_desc) + 2 * (lo + a0);
        if (A.have_last_ids) id = A.last_ids[lo + a0];
      }
      if (src && A.fobs[o + i]) {  // (:848: an unobserved point is a temporary one)
        d0 = src[0], d1 = src[1];
        flags = (A.foutl && A.foutl[o + i]) ? 2 : 3;
        if (id < 0) id = -1;
      } else {
        id = -1;
      }
    }
    A.slot_ids[o + i] = id, A.slot_flags[o + i] = flags;
    uint4 *dst = reinterpret_cast<uint4 *>(A.slot_desc) + 2 * (o + i);
    dst[0] = d0, dst[1] = d1;
  }
  __syncthreads();  // every read of the old list is done
  // ---- cullingOutliersOfFrame (:888-895) and frame_last_ = frame_curr_ (:128); a thread reads back the slots it wrote
  ho_end_list(n, A.n_last, A.slot_flags + o, A.slot_ids + o, A.slot_desc + 32 * o, A.octave + o, A.angle + o, A.fpoint + 3 * o, A.p0 + 3 * lo,
              A.pf0 + lo, A.q0_level + lo, A.q0_angle + lo, A.q0_desc + 32 * lo, A.last_ids + lo);
}

struct BeginArgs {
  int cap, n_last, n_local, nq_local, P;
  const int *fn;
  const float *x, *y, *depth;  // the frame store's columns [B][cap]
  const uint8_t *desc;
  const uint8_t *is_keyframe;  // [B] or NULL
  float th_depth;
  float cam[4];
  const double *velocity, *last_pose;
  double *p0;
  uint8_t *pf0, *q0_desc;
  int *last_ids, *temp_count;
  double *Tcw, *pose0;
  const int *ids1;  // or NULL: the link is left alone
  int *link1;
  unsigned long long *gkeys;
};

__global__ __launch_bounds__(256) void k_ho_begin(BeginArgs A) {
  __shared__ unsigned long long s_keys[kHoLdsKeys];
  __shared__ int s_w[4];
  __shared__ int s_stop[2];  // J and C_J of the pair that ends the walk
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(A.fn[f], 0), A.cap);
  const size_t o = (size_t)f * A.cap, lo = (size_t)f * A.n_last, mo = (size_t)f * A.n_local;
  unsigned long long *keys = A.P <= kHoLdsKeys ? s_keys : A.gkeys + (size_t)f * A.P;
  const double *L = A.last_pose + 12 * (size_t)f;
  // ---- the start pose (:236)
  if (tid == 0) {
    double T[12], xi[6];
    ho_compose(A.velocity + 12 * (size_t)f, L, T);
    ba::se3_log_from_R(T, T + 9, xi);
    for (int k = 0; k < 12; k++) A.Tcw[12 * (size_t)f + k] = T[k];
    for (int k = 0; k < 6; k++) A.pose0[6 * (size_t)f + k] = xi[k];
  }
  // ---- updateLastFrame's temporary points (:555-592)
  int C = 0;
  if (!(A.is_keyframe && A.is_keyframe[f])) {  // (:552)
    const int P = pow2_ceil(max(n, 1));         // (<= A.P: n <= cap)
    for (int i = tid; i < P; i += 256) {
      const float d = i < n ? A.depth[o + i] : 0.f;
      keys[i] = d > 0.f ? ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i : ~0ull;  // (:562)
    }
    block_bitonic_sort(keys, P);  // sort(depthPairs) (:569): distinct keys, THE order of pair<float, int>
    for (int j0 = 0; j0 < P; j0 += 256) {
      const int j = j0 + tid;
      const unsigned long long key = j < P ? keys[j] : ~0ull;
      const bool valid = key != ~0ull;
      const int idx = (int)(key & 0xffffffffu);
      const float d = __uint_as_float((unsigned)(key >> 32));
      const bool c = valid && (A.pf0[lo + idx] & 3) != 3;  // `!mp || mp->getObsCnt() < 1` (:579)
      int total, ts;
      const int Cj = C + block_rank(c, s_w, &total) + (c ? 1 : 0);
      const bool stop = valid && d > A.th_depth && Cj > 100;  // (:590)
      const int sr = block_rank(stop, s_w, &ts);
      if (stop && sr == 0) s_stop[0] = j, s_stop[1] = Cj;
      __syncthreads();
      const int J = ts > 0 ? s_stop[0] : j0 + 256;
      if (c && j <= J) {  // the check follows the creation: pair J itself is created when its slot is null
        double pc[3], pw[3];
        kc_pixel2camera(A.cam, A.x[o + idx], A.y[o + idx], d, pc);
        kc_camera2world(L, pc, pw);
        for (int k = 0; k < 3; k++) A.p0[3 * (lo + idx) + k] = pw[k];
        A.pf0[lo + idx] = 1, A.last_ids[lo + idx] = -1;  // exists, observe_cnt_ 0 (mappoint.cpp:11-34)
        const uint4 *src = reinterpret_cast<const uint4 *>(A.desc) + 2 * (o + idx);
        uint4 *dst = reinterpret_cast<uint4 *>(A.q0_desc) + 2 * (lo + idx);
        dst[0] = src[0], dst[1] = src[1];  // descriptor_ = the feature's (mappoint.cpp:30)
      }
      if (ts > 0) {
        C = s_stop[1];
        break;  // (uniform)
      }
      C += total;
      __syncthreads();  // (s_stop is the next chunk's)
    }
  }
  if (tid == 0) A.temp_count[f] = C;
  // ---- link by id (:765)
  if (!A.ids1) return;
  __syncthreads();  // the temporary points' flags and ids are written (id -1: they link to nothing)
  ho_link_by_id(keys, A.cap, A.pf0 + lo, A.last_ids + lo, A.ids1 + mo, A.link1 + mo, A.nq_local);
}

// the block, allocated by the first call of this file's API
int ho_ensure(vo_tracker *t) {
  if (t->ho) return VO_OK;
  Handover *h = new (std::nothrow) Handover();
  if (!h) {
    set_error("vo_tracker: out of host memory");
    return VO_ERR_HIP;
  }
  const size_t B = t->B, cap = t->cap, nl = (size_t)t->n_last;
  h->P = pow2_ceil(std::max(t->cap, 1));
  const int rc = h->mem.build(
      [&](Arena &a) {
        a.take(h->slot_ids, B * cap * 4);
        a.take(h->slot_desc, B * cap * 32);
        a.take(h->slot_flags, B * cap);
        a.take(h->last_ids, B * nl * 4);
        a.take(h->frame_pose, B * 96);
        a.take(h->velocity, B * 96);
        a.take(h->last_pose, B * 96 + B);
        a.take(h->motion_state, B * 4);
        a.take(h->temp_count, B * 4);
        a.take(h->keys, h->P > kHoLdsKeys ? B * (size_t)h->P * 8 : 0);
      },
      "vo_tracker (hand-over)");
  if (rc != VO_OK) {
    delete h;
    return rc;
  }
  h->last_valid = reinterpret_cast<uint8_t *>(h->last_pose + B * 12);
  // no last pose, no motion, no ids: zeros, and -1 in the id arrays
  if (hipMemsetAsync(h->mem.block, 0, h->mem.bytes, t->st) != hipSuccess ||
      hipMemsetAsync(h->slot_ids, 0xff, B * cap * 4, t->st) != hipSuccess ||
      hipMemsetAsync(h->last_ids, 0xff, B * nl * 4, t->st) != hipSuccess || hipStreamSynchronize(t->st) != hipSuccess) {
    delete h;
    set_error("vo_tracker (hand-over): clearing the block failed");
    return VO_ERR_HIP;
  }
  t->ho = h;
  return VO_OK;
}

}  // namespace

int vo::handover_ensure(vo_tracker *t) { return ho_ensure(t); }

const void *vo::handover_selector(const vo_tracker *t, int what, size_t *bytes) {
  const Handover *h = t->ho;
  if (!h) return nullptr;
  const size_t B = t->B, cap = t->cap;
  switch (what) {
    case VO_TRACKER_SLOT_IDS: *bytes = B * cap * 4; return h->slot_ids;
    case VO_TRACKER_SLOT_DESC: *bytes = B * cap * 32; return h->slot_desc;
    case VO_TRACKER_FRAME_POSE: *bytes = B * 96; return h->frame_pose;
    case VO_TRACKER_VELOCITY: *bytes = B * 96; return h->velocity;
    case VO_TRACKER_MOTION_STATE: *bytes = B * 4; return h->motion_state;
    case VO_TRACKER_TEMP_COUNT: *bytes = B * 4; return h->temp_count;
    case VO_TRACKER_LAST_IDS: *bytes = B * (size_t)t->n_last * 4; return h->last_ids;
    default: return nullptr;
  }
}

extern "C" {

int vo_tracker_set_last_frame_ids(vo_tracker *t, int n, const int32_t *ids) {
  if (!t) return VO_ERR_INVALID;
  if (n != t->nq_last || (n > 0 && !ids)) {
    set_error("vo_tracker_set_last_frame_ids: %d ids for a last-frame list of %d entries", n, t->nq_last);
    return VO_ERR_INVALID;
  }
  VO_CHECK(ho_ensure(t));
  // rows of max_last entries, -1 behind n: one copy
  const size_t B = t->B, nl = (size_t)t->n_last;
  VO_CHECK(t->stage.reserve(B * nl * 4));
  int32_t *h = reinterpret_cast<int32_t *>(t->stage.data());
  for (size_t f = 0; f < B; f++)
    for (size_t i = 0; i < nl; i++) h[f * nl + i] = i < (size_t)n ? ids[f * (size_t)n + i] : -1;
  VO_HIP_CHECK(hipMemcpyAsync(t->ho->last_ids, h, B * nl * 4, hipMemcpyHostToDevice, t->st));
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  t->have_last_ids = true;
  return VO_OK;
}

int vo_tracker_set_last_pose(vo_tracker *t, const double *Tcw12, const uint8_t *valid) {
  if (!t || !Tcw12 || !valid) return VO_ERR_INVALID;
  VO_CHECK(ho_ensure(t));
  const size_t B = t->B;
  VO_CHECK(t->stage.reserve(B * 97));
  memcpy(t->stage.data(), Tcw12, B * 96);
  for (size_t f = 0; f < B; f++) t->stage.data()[B * 96 + f] = valid[f] ? 1 : 0;
  VO_HIP_CHECK(hipMemcpyAsync(t->ho->last_pose, t->stage.data(), B * 97, hipMemcpyHostToDevice, t->st));
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  return VO_OK;
}

int vo_tracker_end_frame(vo_tracker *t, const vo_tracker_handover_params *p) {
  if (!t || !p) return VO_ERR_INVALID;
  // everything is checked before anything is enqueued
  const unsigned r = t->last_run;
  if (!t->have_result || !(r & kRunMotion) || (r & (kRunReloc | kRunRefKeyFrame | kRunRefStore))) {
    set_error("vo_tracker_end_frame: valid after vo_tracker_track[_dev] and vo_tracker_track_first[_dev] (+ vo_tracker_track_local_map)");
    return VO_ERR_INVALID;
  }
  if (t->cap > t->n_last) {
    set_error("vo_tracker_end_frame: %d feature slots per frame, the last-frame list holds %d (max_last)", t->cap, t->n_last);
    return VO_ERR_CAPACITY;
  }
  VO_CHECK(ho_ensure(t));
  const vo_tracker::Arrays &d = t->d;
  const Handover &h = *t->ho;
  const FrameStoreView F = frame_store_view(t->frames);
  EndArgs A{};
  A.cap = t->cap, A.n_last = t->n_last, A.n_local = t->n_local, A.fn = F.n;
  A.assigned_first = d.assigned_first, A.assigned = d.assigned, A.fhas = d.fhas, A.fobs = d.fobs;
  A.foutl = (r & kRunLocal) ? d.foutl : nullptr, A.fpoint = d.fpoint;
  A.q1_desc = d.q1_desc, A.ids1 = t->have_ids ? d.ids1 : nullptr, A.have_last_ids = t->have_last_ids ? 1 : 0;
  A.octave = F.octave, A.angle = F.angle, A.pose6 = d.pose, A.status = d.status, A.ntracked = d.ntracked;
  A.min_tracked = p->min_tracked > 0 ? p->min_tracked : 30;
  A.p0 = d.p0, A.pf0 = d.pf0, A.q0_level = d.q0_level, A.q0_angle = d.q0_angle, A.q0_desc = d.q0_desc, A.last_ids = h.last_ids;
  A.slot_ids = h.slot_ids, A.slot_desc = h.slot_desc, A.slot_flags = h.slot_flags;
  A.frame_pose = h.frame_pose, A.velocity = h.velocity, A.last_pose = h.last_pose, A.last_valid = h.last_valid;
  A.motion_state = h.motion_state;
  hipLaunchKernelGGL(k_ho_end, dim3(t->B), dim3(256), 0, t->st, A);
  VO_HIP_CHECK(hipGetLastError());
  t->nq_last = t->cap;  // entry i is slot i
  t->have_last_ids = true, t->handed_over = true, t->begun = false;
  return VO_OK;
}

int vo_tracker_begin_frame(vo_tracker *t, const vo_tracker_handover_params *p, const uint8_t *dev_is_keyframe) {
  if (!t || !p) return VO_ERR_INVALID;
  if (!t->ho || !t->handed_over) {
    set_error("vo_tracker_begin_frame: valid after vo_tracker_end_frame, before the next track call or last-frame setter");
    return VO_ERR_INVALID;
  }
  const vo_tracker::Arrays &d = t->d;
  const Handover &h = *t->ho;
  const FrameStoreView F = frame_store_view(t->frames);
  const bool link = t->have_local && t->have_ids && t->have_last_ids;
  BeginArgs A{};
  A.cap = t->cap, A.n_last = t->n_last, A.n_local = t->n_local, A.nq_local = t->nq_local, A.P = h.P;
  A.fn = F.n, A.x = F.x, A.y = F.y, A.depth = frame_store_source(t->frames).depth, A.desc = F.desc;
  A.is_keyframe = dev_is_keyframe, A.th_depth = p->th_depth;
  for (int i = 0; i < 4; i++) A.cam[i] = t->cfg.intrinsics[i];
  A.velocity = h.velocity, A.last_pose = h.last_pose;
  A.p0 = d.p0, A.pf0 = d.pf0, A.q0_desc = d.q0_desc, A.last_ids = h.last_ids, A.temp_count = h.temp_count;
  A.Tcw = d.Tcw, A.pose0 = d.pose0;
  A.ids1 = link ? d.ids1 : nullptr, A.link1 = d.link1, A.gkeys = h.keys;
  hipLaunchKernelGGL(k_ho_begin, dim3(t->B), dim3(256), 0, t->st, A);
  VO_HIP_CHECK(hipGetLastError());
  if (link) t->have_link = true;
  t->begun = true;  // (vo_tracker_refresh_last_pose's window is closed)
  return VO_OK;
}

int vo_tracker_handover_arrays(vo_tracker *t, const int32_t **dev_slot_ids, const double **dev_Tcw12, const int32_t **dev_state) {
  if (!t) return VO_ERR_INVALID;
  VO_CHECK(ho_ensure(t));
  if (dev_slot_ids) *dev_slot_ids = t->ho->slot_ids;
  if (dev_Tcw12) *dev_Tcw12 = t->ho->frame_pose;
  if (dev_state) *dev_state = t->ho->motion_state;
  return VO_OK;
}

}  // extern "C"
