// kfstore.hip -- the key-frame feature store: everything the relocalisation route reads of a
// key-frame, resident on the device, addressed by the insertion number the key-frame database (kfdb.hip) uses.  One
// fixed-size record per key-frame (vo_common.h: KfStoreView), so that the host insert is one staging copy and the route's
// kernels reach a key-frame's arrays from its number alone.
#include "vo_common.h"

#include <new>
#include <vector>

namespace {

__global__ void k_kfstore_head(int *head, int n, int bad) {
  if (threadIdx.x == 0) head[0] = n, head[1] = bad, head[3] = 0;  // head[2], the node count, is k_featvec's
}
__global__ void k_kfstore_bad(int *head, int bad) {
  if (threadIdx.x == 0) head[1] = bad;
}

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

struct vo_kfstore {
  int max_kf = 0, NK = 0, size = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  vo::KfStoreView V{};
  vo::OwnedDevBuf rec;
  vo::OwnedPinnedBuf stage;
  std::vector<int> n;  // features per key-frame (host copy: update_points' lengths)
  uint8_t *record(int k) const { return rec.as<uint8_t>() + (size_t)k * V.rec; }
};

namespace vo {

KfStoreView kfstore_view(const vo_kfstore *s) {
  KfStoreView v = s->V;
  v.size = s->size;
  return v;
}

int kfstore_order_before(const vo_kfstore *s, hipStream_t st) {
  if (s->st == st) return VO_OK;
  VO_HIP_CHECK(hipEventRecord(s->ev_in, s->st));
  VO_HIP_CHECK(hipStreamWaitEvent(st, s->ev_in, 0));
  return VO_OK;
}

int kfstore_order_after(const vo_kfstore *s, hipStream_t st) {
  if (s->st == st) return VO_OK;
  VO_HIP_CHECK(hipEventRecord(s->ev_out, st));
  VO_HIP_CHECK(hipStreamWaitEvent(s->st, s->ev_out, 0));
  return VO_OK;
}

}  // namespace vo

extern "C" {

int vo_kfstore_create(vo_kfstore **out, int max_keyframes, int max_features) {
  if (!out || max_keyframes < 1 || max_features < 1) return VO_ERR_INVALID;
  if (max_features > 65534) {
    vo::set_error("vo_kfstore_create: %d features per key-frame exceed 65534", max_features);
    return VO_ERR_CAPACITY;
  }
  VO_CHECK(vo::ensure_device());
  vo_kfstore *s = new (std::nothrow) vo_kfstore();
  if (!s) return VO_ERR_HIP;
  s->max_kf = max_keyframes, s->NK = max_features;
  const size_t NK = (size_t)max_features;
  vo::KfStoreView &V = s->V;
  V.max_kf = max_keyframes, V.NK = max_features;
  size_t o = 16;
  V.o_angle = o, o = up16(o + NK * 4);
  V.o_mind = o, o = up16(o + NK * 4);
  V.o_maxd = o, o = up16(o + NK * 4);
  V.o_ids = o, o = up16(o + NK * 4);
  V.o_node = o, o = up16(o + NK * 4);
  V.o_start = o, o = up16(o + (NK + 1) * 4);
  V.o_feat = o, o = up16(o + NK * 4);
  V.o_points = o, o = up16(o + NK * 24);
  V.o_desc = o, o = up16(o + NK * 32);
  V.o_pdesc = o, o = up16(o + NK * 32);
  V.o_flags = o, o = up16(o + NK);
  V.rec = o;
  auto fail = [&](int rc) {
    vo_kfstore_destroy(s);
    return rc;
  };
  if (s->rec.reserve(V.rec * (size_t)max_keyframes) != VO_OK) return fail(VO_ERR_HIP);
  V.base = s->rec.as<uint8_t>();
  if (s->stage.reserve(V.rec) != VO_OK) return fail(VO_ERR_HIP);
  if (hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming) != hipSuccess) {
    vo::set_error("vo_kfstore_create: hipEventCreate failed");
    return fail(VO_ERR_HIP);
  }
  s->n.reserve((size_t)max_keyframes);
  *out = s;
  return VO_OK;
}

void vo_kfstore_destroy(vo_kfstore *s) {
  if (!s) return;
  if (s->ev_in) (void)hipEventDestroy(s->ev_in);
  if (s->ev_out) (void)hipEventDestroy(s->ev_out);
  delete s;
}

int vo_kfstore_set_stream(vo_kfstore *s, void *hip_stream) {
  if (!s) return VO_ERR_INVALID;
  s->st = (hipStream_t)hip_stream;
  return VO_OK;
}

int vo_kfstore_size(const vo_kfstore *s) { return s ? s->size : VO_ERR_INVALID; }

int vo_kfstore_insert(vo_kfstore *s, const vo_reloc_candidate *kf, int32_t *index) {
  if (!s || !kf || kf->n < 0) return VO_ERR_INVALID;
  const vo_reloc_candidate &K = *kf;
  const int NK = s->NK;
  // everything is validated BEFORE anything is enqueued or any state changes
  if (s->size >= s->max_kf) {
    vo::set_error("vo_kfstore_insert: the store holds %d key-frames (max_keyframes)", s->max_kf);
    return VO_ERR_CAPACITY;
  }
  if (K.n > NK) {
    vo::set_error("vo_kfstore_insert: %d features, the store holds %d per key-frame (max_features)", K.n, NK);
    return VO_ERR_CAPACITY;
  }
  const vo_bow_view *v = K.nodes;
  int n_nodes = 0, n_feat = 0;
  if (K.n > 0) {
    if (!K.angle || !K.desc || !v || !K.flags || !K.points || !K.ids || !K.point_desc || !K.min_distance || !K.max_distance ||
        v->n_nodes < 0 || (v->n_nodes > 0 && (!v->node_id || !v->start || !v->feat || v->start[0] != 0))) {
      vo::set_error("vo_kfstore_insert: the key-frame lacks an array");
      return VO_ERR_INVALID;
    }
    n_nodes = v->n_nodes;
    for (int j = 0; j < n_nodes; j++)
      if (v->start[j + 1] < v->start[j]) return VO_ERR_INVALID;
    n_feat = n_nodes > 0 ? v->start[n_nodes] : 0;
    if (n_nodes > NK || n_feat > NK) {
      vo::set_error("vo_kfstore_insert: a FeatureVector of %d nodes and %d entries, the store holds %d (max_features)", n_nodes,
                    n_feat, NK);
      return VO_ERR_CAPACITY;
    }
    for (int i = 0; i < n_feat; i++)
      if ((int)v->feat[i] < 0 || (int)v->feat[i] >= K.n) return VO_ERR_INVALID;
    for (int i = 0; i < K.n; i++)
      if ((K.flags[i] & 1) && K.ids[i] < 0) {
        vo::set_error("vo_kfstore_insert: feature %d: id %d is negative", i, K.ids[i]);
        return VO_ERR_INVALID;
      }
  }
  const vo::KfStoreView &V = s->V;
  uint8_t *h = s->stage.data();
  memset(h, 0, V.rec);
  int *head = reinterpret_cast<int *>(h);
  head[0] = K.n, head[1] = K.bad ? 1 : 0, head[2] = n_nodes;
  if (K.n > 0) {
    const size_t n = (size_t)K.n;
    memcpy(h + V.o_angle, K.angle, n * 4);
    memcpy(h + V.o_mind, K.min_distance, n * 4);
    memcpy(h + V.o_maxd, K.max_distance, n * 4);
    memcpy(h + V.o_ids, K.ids, n * 4);
    if (n_nodes > 0) {
      memcpy(h + V.o_node, v->node_id, (size_t)n_nodes * 4);
      memcpy(h + V.o_start, v->start, ((size_t)n_nodes + 1) * 4);
      memcpy(h + V.o_feat, v->feat, (size_t)n_feat * 4);
    }
    memcpy(h + V.o_points, K.points, n * 24);
    memcpy(h + V.o_desc, K.desc, n * 32);
    memcpy(h + V.o_pdesc, K.point_desc, n * 32);
    memcpy(h + V.o_flags, K.flags, n);
  }
  VO_HIP_CHECK(hipMemcpyAsync(s->record(s->size), h, V.rec, hipMemcpyHostToDevice, s->st));  // the one staging copy
  VO_HIP_CHECK(hipStreamSynchronize(s->st));  // the staging block is free again
  if (index) *index = s->size;
  s->n.push_back(K.n);
  s->size++;
  return VO_OK;
}

int vo_kfstore_insert_dev(vo_kfstore *s, int n, int bad, const float *dev_angle, const uint8_t *dev_desc,
                          const int32_t *dev_node_of_feature, const uint8_t *dev_flags, const double *dev_points,
                          const int32_t *dev_ids, const uint8_t *dev_point_desc, const float *dev_min_distance,
                          const float *dev_max_distance, int32_t *index) {
  if (!s || n < 0) return VO_ERR_INVALID;
  if (n > 0 && (!dev_angle || !dev_desc || !dev_node_of_feature || !dev_flags || !dev_points || !dev_ids || !dev_point_desc ||
                !dev_min_distance || !dev_max_distance)) {
    vo::set_error("vo_kfstore_insert_dev: the key-frame lacks an array");
    return VO_ERR_INVALID;
  }
  if (s->size >= s->max_kf) {
    vo::set_error("vo_kfstore_insert_dev: the store holds %d key-frames (max_keyframes)", s->max_kf);
    return VO_ERR_CAPACITY;
  }
  if (n > s->NK || n > 16384) {
    vo::set_error("vo_kfstore_insert_dev: %d features, the store holds %d per key-frame (max_features) and the FeatureVector "
                  "kernel sorts 16384", n, s->NK);
    return VO_ERR_CAPACITY;
  }
  const vo::KfStoreView &V = s->V;
  uint8_t *r = s->record(s->size);
  hipStream_t st = s->st;
  auto d2d = [&](size_t off, const void *src, size_t bytes) -> int {
    if (bytes) VO_HIP_CHECK(hipMemcpyAsync(r + off, src, bytes, hipMemcpyDeviceToDevice, st));
    return VO_OK;
  };
  const size_t N = (size_t)n;
  VO_CHECK(d2d(V.o_angle, dev_angle, N * 4));
  VO_CHECK(d2d(V.o_mind, dev_min_distance, N * 4));
  VO_CHECK(d2d(V.o_maxd, dev_max_distance, N * 4));
  VO_CHECK(d2d(V.o_ids, dev_ids, N * 4));
  VO_CHECK(d2d(V.o_points, dev_points, N * 24));
  VO_CHECK(d2d(V.o_desc, dev_desc, N * 32));
  VO_CHECK(d2d(V.o_pdesc, dev_point_desc, N * 32));
  VO_CHECK(d2d(V.o_flags, dev_flags, N));
  int *head = reinterpret_cast<int *>(r);
  hipLaunchKernelGGL(k_kfstore_head, dim3(1), dim3(64), 0, st, head, n, bad ? 1 : 0);
  VO_HIP_CHECK(hipGetLastError());
  // KeyFrame::computeBow's FeatureVector: node ascending, the features of a node in index order
  VO_CHECK(vo::featvec_dev(n, dev_node_of_feature, head + 2, reinterpret_cast<int *>(r + V.o_node), reinterpret_cast<int *>(r + V.o_start),
                           reinterpret_cast<int *>(r + V.o_feat), st));
  if (index) *index = s->size;
  s->n.push_back(n);
  s->size++;
  return VO_OK;
}

int vo_kfstore_set_bad(vo_kfstore *s, int keyframe, int bad) {
  if (!s || keyframe < 0 || keyframe >= s->size) return VO_ERR_INVALID;
  hipLaunchKernelGGL(k_kfstore_bad, dim3(1), dim3(64), 0, s->st, reinterpret_cast<int *>(s->record(keyframe)), bad ? 1 : 0);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_kfstore_update_points(vo_kfstore *s, int keyframe, const uint8_t *flags, const double *points, const int32_t *ids,
                             const uint8_t *point_desc, const float *min_distance, const float *max_distance) {
  if (!s || keyframe < 0 || keyframe >= s->size) return VO_ERR_INVALID;
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!flags || !points || !ids || !point_desc || !min_distance || !max_distance) return VO_ERR_INVALID;
  for (size_t i = 0; i < n; i++)
    if ((flags[i] & 1) && ids[i] < 0) {
      vo::set_error("vo_kfstore_update_points: feature %zu: id %d is negative", i, ids[i]);
      return VO_ERR_INVALID;
    }
  const vo::KfStoreView &V = s->V;
  // staged at the record's own offsets (the staging block is one record long)
  uint8_t *h = s->stage.data(), *r = s->record(keyframe);
  memcpy(h + V.o_flags, flags, n);
  memcpy(h + V.o_points, points, n * 24);
  memcpy(h + V.o_ids, ids, n * 4);
  memcpy(h + V.o_pdesc, point_desc, n * 32);
  memcpy(h + V.o_mind, min_distance, n * 4);
  memcpy(h + V.o_maxd, max_distance, n * 4);
  auto up = [&](size_t off, size_t bytes) -> int {
    VO_HIP_CHECK(hipMemcpyAsync(r + off, h + off, bytes, hipMemcpyHostToDevice, s->st));
    return VO_OK;
  };
  VO_CHECK(up(V.o_flags, n));
  VO_CHECK(up(V.o_points, n * 24));
  VO_CHECK(up(V.o_ids, n * 4));
  VO_CHECK(up(V.o_pdesc, n * 32));
  VO_CHECK(up(V.o_mind, n * 4));
  VO_CHECK(up(V.o_maxd, n * 4));
  VO_HIP_CHECK(hipStreamSynchronize(s->st));
  return VO_OK;
}

}  // extern "C"
