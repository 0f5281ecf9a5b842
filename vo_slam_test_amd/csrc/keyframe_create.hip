// keyframe_create.hip -- a tracked frame written into the key-frame store as a key-frame:
// VisualOdometry::createNewKeyFrame (visualOdometry.cpp:463-517) with cullingTempMapPoints' slot rule (:844-853), the first
// key-frame of initVisualOdometry (:170-198), Camera::pixel2world (camera.cpp:82-94) and the MapPoint(KeyFrame*) constructor
// with addObservation, computeDescriptor and updateNormalAndDepth for one holder (mappoint.cpp:36-179); and the three counts of
// needNewKeyFrame (visualOdometry.cpp:406-428).
//   k_kc_walk   ONE workgroup: the temp cull (a thread per slot: is the id held by a key-frame of the index?), the pairs
//               (depth bits << 32 | feature) sorted by block_bitonic_sort -- in LDS up to kKcLdsKeys keys, else in the layer's
//               block --, then the walk as a scan: the inclusive count C_j of null slots by wave ballots, the first j with
//               d_j > th_depth && C_j > 100, the created rows (feature, counter + C_j - 1) for j <= J, the counter, the record.
//               initial: the keys are the features with !(d < 0) in feature order, nothing stops the walk.
//   k_kc_fill   a thread per feature: the feature columns, the created point (keyframe_geom.h), the tracked slot's map
//               columns from the id's first observation, or the null slot's zeros; the head words and the pose.
//   k_kc_stats  ONE workgroup: trackedMapPoints(min_obs) of a key-frame and map_cnt / total_cnt of a frame, counted by ballots.
// Then k_bow_transform and k_featvec (match.hip) as vo_kfstore_insert_dev's caller runs them.  No atomic decides an id or an
// order; no kernel waits on another workgroup; every loop is bounded by a count read once.
#include "kfstore.h"

#include "block_sort.h"
#include "keyframe_geom.h"
#include "obs_walk.h"

#include <algorithm>

namespace {

using namespace vo;

constexpr int kSeq = 1024;  // threads of the one-workgroup kernels

// (block_rank, the workgroup-wide exclusive prefix of a flag: block_sort.h)

// the entry of id's first observation in a fresh index (its lowest key: the lowest non-erased key-frame that holds it, at
// its lowest flagged feature), or -1 when no key-frame of the store holds it
__device__ __forceinline__ int first_observation(const KfStoreView &S, const KfObsView &O, int id) {
  if (id < 0) return -1;
  const int pos = obs_lower_bound(O, id);
  if (pos >= O.n_keys) return -1;
  const unsigned long long key = O.keys[pos];
  if (key == ~0ull || (int)(key >> 32) != id) return -1;
  const unsigned e = (unsigned)(key & 0xffffffffu);
  return (int)(e / (unsigned)S.NK) < S.size ? (int)e : -1;
}

struct KcArgs {
  KfStoreView S;  // size: the store's before the call = the new key-frame's number
  KfObsView O;
  KfCullView X;
  KfMapView M;
  KfBaView B;
  KfCreateView K;
  double *normals;
  int n, initial;
  float th_depth;
  const double *Tcw;
  const float *x, *y, *angle, *depth, *u_right;
  const int *octave, *slot_ids;
  const uint8_t *desc;
  const int *n_expected;  // NULL, or the device count n must equal (the frames form): else nothing beyond the head is written
  int *status;
};

enum { kKcOk = 0, kKcCountMismatch = 1 };  // rec[kKcStatus]

__global__ __launch_bounds__(kSeq) void k_kc_walk(KcArgs A) {
  __shared__ unsigned long long s_keys[kKcLdsKeys];
  __shared__ int s_w[kSeq / 64];
  __shared__ int s_stop[2];  // J and C_J of the pair that ends the walk
  const KfCreateView &K = A.K;
  const int tid = threadIdx.x, kf = A.S.size;
  const bool mismatch = A.n_expected && *A.n_expected != A.n;
  const int n = mismatch ? 0 : A.n, counter0 = *A.M.counter;
  const int P = pow2_ceil(max(n, 1));  // (<= K.P: n <= NK)
  unsigned long long *keys = P <= kKcLdsKeys ? s_keys : K.keys;
  // ---- the temp cull (:844-853) and the keys
  int n_tracked = 0;
  for (int i0 = 0; i0 < P; i0 += kSeq) {
    const int i = i0 + tid;
    int id = -1, first = -1;
    unsigned long long key = ~0ull;
    if (i < n) {
      const float d = A.depth[i];
      if (A.initial) {
        if (!(d < 0.f)) key = (unsigned long long)(unsigned)i;  // (:183: d == 0 and NaN are created)
      } else {
        first = first_observation(A.S, A.O, A.slot_ids[i]);
        if (first >= 0) id = A.slot_ids[i];
        if (d > 0.f) key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;  // (:475)
      }
      K.slot[i] = id, K.first[i] = first, K.newid[i] = -1;
    }
    if (i < P) keys[i] = key;
    int total;
    block_rank(id >= 0, s_w, &total);
    n_tracked += total;
  }
  block_bitonic_sort(keys, P);  // sort(depthPairs) (:481): distinct keys, THE order of pair<float, int>
  // ---- the walk (:485-512) as a scan
  int C = 0, m = 0, J = -1, CJ = 0;
  bool found = false;
  for (int j0 = 0; j0 < P; j0 += kSeq) {
    const int j = j0 + tid;
    const unsigned long long key = j < P ? keys[j] : ~0ull;
    const bool valid = key != ~0ull;
    const int idx = (int)(key & 0xffffffffu);
    const bool c = valid && K.slot[idx] < 0;  // "the slot is null" (:493)
    int total, tv, ts;
    const int Cj = C + block_rank(c, s_w, &total) + (c ? 1 : 0);
    block_rank(valid, s_w, &tv);
    m += tv;
    if (found) continue;  // (uniform: the remaining pairs are only counted)
    const bool stop = !A.initial && valid && __uint_as_float((unsigned)(key >> 32)) > A.th_depth && Cj > 100;  // (:510)
    const int sr = block_rank(stop, s_w, &ts);
    if (stop && sr == 0) s_stop[0] = j, s_stop[1] = Cj;
    __syncthreads();
    if (ts > 0) found = true, J = s_stop[0], CJ = s_stop[1];
    if (c && (!found || j <= J)) {  // the check follows the creation: pair J itself is created when its slot is null
      const int id = counter0 + Cj - 1;  // factory_id_++ in walk order (mappoint.cpp:49)
      K.created[Cj - 1] = make_int2(idx, id);
      K.newid[idx] = id;
    }
    C += total;
    __syncthreads();  // (s_stop is the next chunk's)
  }
  if (!found) J = m - 1, CJ = C;
  if (tid < kKcRecInts) {
    int v = 0;
    if (tid == kKcKeyframe) v = kf;
    if (tid == kKcN) v = A.n;
    if (tid == kKcNPairs) v = m;
    if (tid == kKcNWalked) v = J + 1;
    if (tid == kKcNCreated) v = CJ;
    if (tid == kKcNTracked) v = n_tracked;
    if (tid == kKcFirstId) v = counter0;
    if (tid == kKcNextId) v = counter0 + CJ;
    if (tid == kKcEarly) v = found && J < m - 1;
    if (tid == kKcStatus) v = mismatch ? kKcCountMismatch : kKcOk;
    K.rec[tid] = v;
  }
  if (tid == 0) {
    *A.M.counter = counter0 + CJ;
    *K.n_eff = n;  // k_kc_fill's and k_featvec's count
    if (mismatch) atomicOr(A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  }
}

__global__ __launch_bounds__(256) void k_kc_fill(KcArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x, kf = A.S.size, NK = A.S.NK;
  const int n = min(max(*A.K.n_eff, 0), A.n);
  uint8_t *r = const_cast<uint8_t *>(A.S.base) + (size_t)kf * A.S.rec;
  if (i == 0) {
    int *head = reinterpret_cast<int *>(r);
    head[0] = n, head[1] = 0, head[3] = 0;  // bad = 0; head[2], the node count, is k_featvec's
  }
  if (i < 12) np_pose(A.M, kf)[i] = A.Tcw[i];
  if (i == 12) np_pose_set(A.M, kf)[0] = 1, np_pose_set(A.M, kf)[1] = 0;
  if (i >= n) {
    if (i < A.n) {  // the frames form with a wrong count: the rows the host's getters span hold "no feature, no point"
      reinterpret_cast<float *>(r + A.S.o_angle)[i] = 0.f;
      uint4 *z = reinterpret_cast<uint4 *>(r + A.S.o_desc) + 2 * (size_t)i, *zp = reinterpret_cast<uint4 *>(r + A.S.o_pdesc) + 2 * (size_t)i;
      z[0] = z[1] = zp[0] = zp[1] = make_uint4(0, 0, 0, 0);
      cull_octave(A.X, kf)[i] = 0, cull_depth(A.X, kf)[i] = -1.f, cull_uright(A.X, kf)[i] = -1.f;
      np_x(A.M, kf)[i] = 0.f, np_y(A.M, kf)[i] = 0.f;
      r[A.S.o_flags + i] = 0;
      reinterpret_cast<int *>(r + A.S.o_ids)[i] = -1;
      double *pt = reinterpret_cast<double *>(r + A.S.o_points) + 3 * (size_t)i, *nv = A.normals + ((size_t)kf * NK + i) * 3;
      for (int c = 0; c < 3; c++) pt[c] = 0.0, nv[c] = 0.0;
      reinterpret_cast<float *>(r + A.S.o_mind)[i] = 0.f, reinterpret_cast<float *>(r + A.S.o_maxd)[i] = 0.f;
      A.B.ref_kf[(size_t)kf * NK + i] = -1;
    }
    return;
  }
  // ---- the feature side
  const float u = A.x[i], v = A.y[i], d = A.depth[i];
  const int oct = A.octave[i];
  reinterpret_cast<float *>(r + A.S.o_angle)[i] = A.angle[i];
  const uint4 *dsrc = reinterpret_cast<const uint4 *>(A.desc) + 2 * (size_t)i;
  const uint4 d0 = dsrc[0], d1 = dsrc[1];
  uint4 *ddst = reinterpret_cast<uint4 *>(r + A.S.o_desc) + 2 * (size_t)i;
  ddst[0] = d0, ddst[1] = d1;
  cull_octave(A.X, kf)[i] = oct, cull_depth(A.X, kf)[i] = d, cull_uright(A.X, kf)[i] = A.u_right[i];
  np_x(A.M, kf)[i] = u, np_y(A.M, kf)[i] = v;
  // ---- the map side
  const int newid = A.K.newid[i], slot = A.K.slot[i];
  uint8_t flags = 0;
  int id = -1, ref = -1;
  double p[3] = {0, 0, 0}, nrm[3] = {0, 0, 0};
  float mind = 0.f, maxd = 0.f;
  uint4 p0 = make_uint4(0, 0, 0, 0), p1 = p0;
  if (newid >= 0) {  // a created point (camera.cpp:82-94, mappoint.cpp:36-50, 52-64, 66-116, 118-179)
    double pc[3];
    kc_pixel2camera(A.M.cam, u, v, d, pc);
    kc_camera2world(A.Tcw, pc, p);
    kc_single_view(A.Tcw, p, A.M.sf[min(max(oct, 0), 15)], A.M.sf[min(max(A.M.n_levels - 1, 0), 15)], nrm, mind, maxd);
    flags = 3, id = newid, ref = kf, p0 = d0, p1 = d1;
  } else if (slot >= 0) {  // a tracked slot: the map columns of the id's first observation
    const unsigned e = (unsigned)A.K.first[i];
    const int kk = (int)(e / (unsigned)NK), f = (int)(e - (unsigned)kk * (unsigned)NK);
    const double *P = kf_sec<double>(A.S, kk, A.S.o_points) + 3 * (size_t)f;
    const double *N = A.normals + ((size_t)kk * NK + f) * 3;
    for (int c = 0; c < 3; c++) p[c] = P[c], nrm[c] = N[c];
    const uint4 *ps = kf_sec<uint4>(A.S, kk, A.S.o_pdesc) + 2 * (size_t)f;
    p0 = ps[0], p1 = ps[1];
    mind = kf_sec<float>(A.S, kk, A.S.o_mind)[f], maxd = kf_sec<float>(A.S, kk, A.S.o_maxd)[f];
    ref = A.B.ref_kf[(size_t)kk * NK + f];
    flags = 3, id = slot;
  }
  r[A.S.o_flags + i] = flags;
  reinterpret_cast<int *>(r + A.S.o_ids)[i] = id;
  double *pt = reinterpret_cast<double *>(r + A.S.o_points) + 3 * (size_t)i;
  double *nv = A.normals + ((size_t)kf * NK + i) * 3;
  for (int c = 0; c < 3; c++) pt[c] = p[c], nv[c] = nrm[c];
  uint4 *pd = reinterpret_cast<uint4 *>(r + A.S.o_pdesc) + 2 * (size_t)i;
  pd[0] = p0, pd[1] = p1;
  reinterpret_cast<float *>(r + A.S.o_mind)[i] = mind, reinterpret_cast<float *>(r + A.S.o_maxd)[i] = maxd;
  A.B.ref_kf[(size_t)kf * NK + i] = ref;
}

// ---- needNewKeyFrame's counts (visualOdometry.cpp:406-428, keyframe.cpp:210-226)
__global__ __launch_bounds__(kSeq) void k_kc_stats(KfStoreView S, KfObsView O, KfCullView X, int *status, int ref_kf, int min_obs, int n,
                                                   const float *depth, const int *slot_ids, float th_depth, int *out) {
  __shared__ int s_w[kSeq / 64];
  const int tid = threadIdx.x;
  const bool gone = ref_kf < 0 || ref_kf >= S.size || X.erased[ref_kf] != 0;
  int tracked = 0, map_cnt = 0, total_cnt = 0, total;
  const int nf = gone ? 0 : min(max(kf_head(S, ref_kf)[0], 0), S.NK);
  for (int i0 = 0; i0 < nf; i0 += kSeq) {
    const int i = i0 + tid;
    bool ok = false;
    if (i < nf && (kf_sec<uint8_t>(S, ref_kf, S.o_flags)[i] & 1)) {
      const int id = kf_sec<int>(S, ref_kf, S.o_ids)[i];
      if (id >= 0) {
        int obs = 0;  // (the index is fresh: every key is live)
        obs_run_holders(
            O, S.NK, S.size, obs_lower_bound(O, id), id, [](int, unsigned) { return true; },
            [&](int kk, int f) {
              obs += cull_uright(X, kk)[f] >= 0.f ? 2 : 1;
              return true;
            });
        ok = obs >= min_obs;
      }
    }
    block_rank(ok, s_w, &total);
    tracked += total;
  }
  if (!gone)
    for (int i0 = 0; i0 < n; i0 += kSeq) {
      const int i = i0 + tid;
      const float d = i < n ? depth[i] : 0.f;
      const bool near = i < n && d > 0.f && d < th_depth;  // (:418)
      const bool held = near && first_observation(S, O, slot_ids[i]) >= 0;  // mp && mp->getObsCnt() > 0 (:425)
      block_rank(near, s_w, &total);
      total_cnt += total;
      block_rank(held, s_w, &total);
      map_cnt += total;
    }
  if (tid == 0) {
    out[0] = tracked, out[1] = map_cnt, out[2] = total_cnt, out[3] = 0;
    if (gone) atomicOr(status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  }
}

__global__ void k_kc_init(KfCreateView K) {
  if (threadIdx.x < kKcRecInts) K.rec[threadIdx.x] = 0;
  if (threadIdx.x < 4) K.stats[threadIdx.x] = 0;
}

struct KcLayout {
  uint8_t *block;
  size_t at = 0;
  template <class T>
  void take(T *&field, size_t bytes) {
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += up16(bytes);
  }
};

void kc_layout(KcLayout &L, KfCreateView &K, int NK) {
  const size_t n = (size_t)NK, P = (size_t)pow2_ceil(NK);
  L.take(K.keys, P * 8);
  L.take(K.created, n * 8);
  L.take(K.rec, kKcRecInts * 4);
  L.take(K.stats, 16);
  L.take(K.n_eff, 16);
  L.take(K.slot, n * 4), L.take(K.first, n * 4), L.take(K.newid, n * 4), L.take(K.word, n * 4), L.take(K.node, n * 4);
  L.take(K.weight, n * 8);
  K.in_bytes = 96 + 7 * up16(n * 4) + n * 32;
  L.take(K.in, K.in_bytes);
  K.NK = NK, K.P = (int)P;
}

size_t kc_bytes(int NK) {
  KcLayout L{nullptr};
  KfCreateView K{};
  kc_layout(L, K, NK);
  return L.at;
}

// the call's launches: walk, fill, k_bow_transform, k_featvec
int kc_enqueue(vo_kfstore *s, const vo_vocab *vocab, const KfObsView &O, int n, const double *Tcw, const float *x, const float *y,
               const int32_t *octave, const float *angle, const float *depth, const float *u_right, const uint8_t *desc,
               const int32_t *slot_ids, float th_depth, int initial, const int *n_expected) {
  const KfStoreView V = kfstore_view(s);
  KcArgs A{V, O, s->X, s->M, s->B, s->K, s->normals.as<double>(), n, initial ? 1 : 0, th_depth, Tcw,
           x, y, angle, depth, u_right, octave, slot_ids, desc, n_expected, connections_view(s->conn).status};
  hipStream_t st = s->st;
  hipLaunchKernelGGL(k_kc_walk, dim3(1), dim3(kSeq), 0, st, A);
  hipLaunchKernelGGL(k_kc_fill, dim3((unsigned)((std::max(n, 13) + 255) / 256)), dim3(256), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  // KeyFrame::computeBow's FeatureVector, as vo_kfstore_insert_dev builds it from node ids
  uint8_t *r = s->record(s->size);
  VO_CHECK(vocab_transform_resident(vocab, n, reinterpret_cast<const uint32_t *>(desc), 3, s->K.word, s->K.weight, s->K.node, st));
  return featvec_dev(n, s->K.node, reinterpret_cast<int *>(r) + 2, reinterpret_cast<int *>(r + V.o_node), reinterpret_cast<int *>(r + V.o_start),
                     reinterpret_cast<int *>(r + V.o_feat), st, s->K.n_eff);
}

// what both forms validate before anything is enqueued
int kc_check(const vo_kfstore *s, const char *W, const vo_vocab *vocab, int n) {
  VO_CHECK(need(s, W, kLayerKeyframeCreate));
  if (!vocab || n < 0) return VO_ERR_INVALID;
  if (n > s->NK || n > 16384) {  // (vo_kfstore_enable_mapping refuses a store wider than 16384: the second bound restates it)
    set_error("%s: %d features, the store holds %d per key-frame (max_features) and the FeatureVector kernel sorts 16384", W, n, s->NK);
    return VO_ERR_CAPACITY;
  }
  if (s->size >= s->max_kf) {
    set_error("%s: the store holds %d key-frames (max_keyframes)", W, s->max_kf);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_keyframe_create(vo_kfstore *s) {
  const char *W = "vo_kfstore_enable_keyframe_create";
  if (const int rc = enable_begin(s, W, kLayerLocalBa, kLayerKeyframeCreate)) return rc < 0 ? rc : VO_OK;
  VO_CHECK(s->kc.reserve(kc_bytes(s->NK)));
  KcLayout L{s->kc.as<uint8_t>()};
  kc_layout(L, s->K, s->NK);
  VO_CHECK(s->kc_stage.reserve(s->K.in_bytes));
  hipLaunchKernelGGL(k_kc_init, dim3(1), dim3(64), 0, s->st, s->K);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerKeyframeCreate;
  return VO_OK;
}

int vo_kfstore_create_keyframe_dev(vo_kfstore *s, const vo_vocab *vocab, int n, const double *dev_Tcw12, const float *dev_x,
                                   const float *dev_y, const int32_t *dev_octave, const float *dev_angle, const float *dev_depth,
                                   const float *dev_u_right, const uint8_t *dev_desc, const int32_t *dev_slot_ids, float th_depth,
                                   int initial, int32_t *index) {
  const char *W = "vo_kfstore_create_keyframe_dev";
  VO_CHECK(kc_check(s, W, vocab, n));
  if (!dev_Tcw12 || (n > 0 && (!dev_x || !dev_y || !dev_octave || !dev_angle || !dev_depth || !dev_u_right || !dev_desc ||
                               (!initial && !dev_slot_ids)))) {
    set_error("%s: the frame lacks an array", W);
    return VO_ERR_INVALID;
  }
  if (reinterpret_cast<uintptr_t>(dev_desc) & 15) {
    set_error("%s: the descriptor rows must start on a 16-byte boundary", W);
    return VO_ERR_INVALID;
  }
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // the key-frame being created is not in it
  VO_CHECK(kc_enqueue(s, vocab, O, n, dev_Tcw12, dev_x, dev_y, dev_octave, dev_angle, dev_depth, dev_u_right, dev_desc, dev_slot_ids,
                      th_depth, initial, nullptr));
  if (index) *index = s->size;
  s->n.push_back(n);
  s->size++;
  s->obs_dirty = true, s->gen++;
  return VO_OK;
}

int vo_kfstore_create_keyframe(vo_kfstore *s, const vo_vocab *vocab, int n, const double *Tcw12, const float *x, const float *y,
                               const int32_t *octave, const float *angle, const float *depth, const float *u_right, const uint8_t *desc,
                               const int32_t *slot_ids, float th_depth, int initial, int32_t *index) {
  const char *W = "vo_kfstore_create_keyframe";
  VO_CHECK(kc_check(s, W, vocab, n));
  if (!Tcw12 || (n > 0 && (!x || !y || !octave || !angle || !depth || !u_right || !desc || (!initial && !slot_ids)))) {
    set_error("%s: the frame lacks an array", W);
    return VO_ERR_INVALID;
  }
  for (int i = 0; i < n; i++)
    if (octave[i] < 0 || octave[i] >= s->M.n_levels) {
      set_error("%s: feature %d: octave %d outside the store's %d levels", W, i, octave[i], s->M.n_levels);
      return VO_ERR_INVALID;
    }
  // staged as the block's `in` holds them; one copy
  const size_t N = (size_t)n;
  const KcInputs H = kc_inputs(s->kc_stage.data(), s->NK), D = kc_inputs(s->K.in, s->NK);
  memcpy(H.T, Tcw12, 96);
  if (n > 0) {
    memcpy(H.x, x, N * 4), memcpy(H.y, y, N * 4), memcpy(H.octave, octave, N * 4), memcpy(H.angle, angle, N * 4);
    memcpy(H.depth, depth, N * 4), memcpy(H.u_right, u_right, N * 4), memcpy(H.desc, desc, N * 32);
    if (initial) memset(H.slot, 0xff, N * 4);
    else memcpy(H.slot, slot_ids, N * 4);
  }
  const size_t bytes = (size_t)(H.desc - s->kc_stage.data()) + N * 32;
  VO_CHECK(copy_h2d(s->K.in, s->kc_stage.data(), bytes, s->st, W));
  const int rc = vo_kfstore_create_keyframe_dev(s, vocab, n, D.T, D.x, D.y, D.octave, D.angle, D.depth, D.u_right, D.desc, D.slot, th_depth,
                                                initial, index);
  const int rs = stream_sync(s->st, W);  // (the staging block is free again, whatever the call answered)
  return rc != VO_OK ? rc : rs;
}

int vo_kfstore_create_keyframe_from_frames(vo_kfstore *s, const vo_vocab *vocab, vo_frames *frames, int slot, int n, const double *dev_Tcw12,
                                           const int32_t *dev_slot_ids, float th_depth, int initial, int32_t *index) {
  const char *W = "vo_kfstore_create_keyframe_from_frames";
  VO_CHECK(kc_check(s, W, vocab, n));
  if (!frames || !dev_Tcw12 || (n > 0 && !initial && !dev_slot_ids)) return VO_ERR_INVALID;
  const FrameStoreView F = frame_store_view(frames);
  const FrameStoreSource src = frame_store_source(frames);
  if (slot < 0 || slot >= src.slots) {
    set_error("%s: slot %d outside [0, %d)", W, slot, src.slots);
    return VO_ERR_INVALID;
  }
  if (n > F.cap) {
    set_error("%s: %d features, the frames hold %d per slot", W, n, F.cap);
    return VO_ERR_CAPACITY;
  }
  VO_CHECK(kfstore_order_after(s, src.producer));  // the store's stream waits for what the frames' producer holds now
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  const size_t o = (size_t)slot * F.cap;
  VO_CHECK(kc_enqueue(s, vocab, O, n, dev_Tcw12, F.x + o, F.y + o, F.octave + o, F.angle + o, src.depth + o, F.uright + o, F.desc + o * 32,
                      dev_slot_ids, th_depth, initial, F.n + slot));
  if (index) *index = s->size;
  s->n.push_back(n);
  s->size++;
  s->obs_dirty = true, s->gen++;
  return VO_OK;
}

int vo_kfstore_get_features(vo_kfstore *s, int keyframe, float *angle, uint8_t *desc, int32_t *octave, float *depth, float *u_right,
                            float *xy, int32_t *n_nodes, int32_t *node, int32_t *start, int32_t *feat) {
  const char *W = "vo_kfstore_get_features";
  VO_CHECK(need(s, W, kLayerMapping));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  const KfStoreView &V = s->V;
  const uint8_t *r = s->record(keyframe);
  int32_t head[4] = {0, 0, 0, 0};
  VO_CHECK(copy_d2h(head, r, 16, s->st, W));
  std::vector<float> cols(xy ? 2 * n : 0);
  if (n > 0) {
    if (angle) VO_CHECK(copy_d2h(angle, r + V.o_angle, n * 4, s->st, W));
    if (desc) VO_CHECK(copy_d2h(desc, r + V.o_desc, n * 32, s->st, W));
    if (octave) VO_CHECK(copy_d2h(octave, cull_octave(s->X, keyframe), n * 4, s->st, W));
    if (depth) VO_CHECK(copy_d2h(depth, cull_depth(s->X, keyframe), n * 4, s->st, W));
    if (u_right) VO_CHECK(copy_d2h(u_right, cull_uright(s->X, keyframe), n * 4, s->st, W));
    if (xy) {
      VO_CHECK(copy_d2h(cols.data(), np_x(s->M, keyframe), n * 4, s->st, W));
      VO_CHECK(copy_d2h(cols.data() + n, np_y(s->M, keyframe), n * 4, s->st, W));
    }
    if (node) VO_CHECK(copy_d2h(node, r + V.o_node, n * 4, s->st, W));
    if (feat) VO_CHECK(copy_d2h(feat, r + V.o_feat, n * 4, s->st, W));
  }
  if (start) VO_CHECK(copy_d2h(start, r + V.o_start, (n + 1) * 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  for (size_t i = 0; xy && i < n; i++) xy[2 * i] = cols[i], xy[2 * i + 1] = cols[n + i];
  if (n_nodes) *n_nodes = head[2];
  return VO_OK;
}

int vo_kfstore_keyframe_result(vo_kfstore *s, int32_t *record, int32_t *created_feature, int32_t *created_id) {
  const char *W = "vo_kfstore_keyframe_result";
  VO_CHECK(need(s, W, kLayerKeyframeCreate));
  int32_t rec[kKcRecInts];
  VO_CHECK(copy_d2h(rec, s->K.rec, sizeof(rec), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  if (record) memcpy(record, rec, sizeof(rec));
  const int nc = std::min(std::max(rec[kKcNCreated], 0), s->NK);
  if (nc > 0 && (created_feature || created_id)) {
    std::vector<int32_t> rows((size_t)nc * 2);
    VO_CHECK(copy_d2h(rows.data(), s->K.created, rows.size() * 4, s->st, W));
    VO_CHECK(stream_sync(s->st, W));
    for (int i = 0; i < nc; i++) {
      if (created_feature) created_feature[i] = rows[2 * (size_t)i];
      if (created_id) created_id[i] = rows[2 * (size_t)i + 1];
    }
  }
  return VO_OK;
}

int vo_kfstore_keyframe_need_stats_dev(vo_kfstore *s, int ref_kf, int min_obs, int n, const float *dev_depth, const int32_t *dev_slot_ids,
                                       float th_depth, int32_t *dev_out) {
  const char *W = "vo_kfstore_keyframe_need_stats_dev";
  VO_CHECK(need(s, W, kLayerKeyframeCreate));
  if (n < 0 || !dev_out || (n > 0 && (!dev_depth || !dev_slot_ids))) return VO_ERR_INVALID;
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  // (that ref_kf is erased only the device knows; a number outside the store is answered there too: zeros and the sticky bit)
  hipLaunchKernelGGL(k_kc_stats, dim3(1), dim3(kSeq), 0, s->st, kfstore_view(s), O, s->X, connections_view(s->conn).status, ref_kf, min_obs, n,
                     dev_depth, dev_slot_ids, th_depth, dev_out);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_kfstore_keyframe_need_stats(vo_kfstore *s, int ref_kf, int min_obs, int n, const float *depth, const int32_t *slot_ids,
                                   float th_depth, int32_t *out) {
  const char *W = "vo_kfstore_keyframe_need_stats";
  VO_CHECK(need(s, W, kLayerKeyframeCreate));
  if (n < 0 || !out || (n > 0 && (!depth || !slot_ids))) return VO_ERR_INVALID;
  if (n > s->NK) {
    set_error("%s: %d features, the store holds %d per key-frame (max_features)", W, n, s->NK);
    return VO_ERR_CAPACITY;
  }
  const KcInputs H = kc_inputs(s->kc_stage.data(), s->NK), D = kc_inputs(s->K.in, s->NK);
  if (n > 0) {  // one copy spans the depth column, the one between and the slot ids
    memcpy(H.depth, depth, (size_t)n * 4), memcpy(H.slot, slot_ids, (size_t)n * 4);
    const size_t bytes = (size_t)(reinterpret_cast<uint8_t *>(H.slot) - reinterpret_cast<uint8_t *>(H.depth)) + (size_t)n * 4;
    VO_CHECK(copy_h2d(D.depth, H.depth, bytes, s->st, W));
  }
  VO_CHECK(vo_kfstore_keyframe_need_stats_dev(s, ref_kf, min_obs, n, D.depth, D.slot, th_depth, s->K.stats));
  VO_CHECK(copy_d2h(out, s->K.stats, 16, s->st, W));
  return stream_sync(s->st, W);
}

}  // extern "C"
