// kfstore.hip -- the key-frame feature store: everything the relocalisation route reads of a
// key-frame, resident on the device, addressed by the insertion number the key-frame database (kfdb.hip) uses.  One
// fixed-size record per key-frame (kfstore.h: KfStoreView), so that the host insert is one staging copy and the route's
// kernels reach a key-frame's arrays from its number alone.  The opt-in layers (sections 4h-4o) have a file each, kernels
// and entry points; this one holds the store itself, the observation index and the guards the layers share.
#include "kfstore.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {

__global__ void k_kfstore_head(int *head, int n, int bad) {
  if (threadIdx.x == 0) head[0] = n, head[1] = bad, head[3] = 0;  // head[2], the node count, is k_featvec's
}
__global__ void k_kfstore_bad(int *head, int bad) {
  if (threadIdx.x == 0) head[1] = bad;
}

// ---- the observation index: one 64-bit key per flagged feature of the store, id << 32 | entry,
// sorted by a device-wide bitonic network (fixed: the result is a function of the keys alone, and the keys are distinct).
constexpr int kObsChunk = 2048;  // keys a workgroup of 256 sorts in LDS

// (erased: the column of a store with culling, else NULL -- an erased key-frame holds nothing)
__global__ __launch_bounds__(256) void k_obs_fill(vo::KfStoreView V, const int *erased, unsigned long long *keys, int n_keys) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_keys) return;
  const int k = e / V.NK, i = e - k * V.NK;
  unsigned long long key = ~0ull;
  if (k < V.size && !(erased && erased[k]) && i < min(max(vo::kf_head(V, k)[0], 0), V.NK) &&
      (vo::kf_sec<uint8_t>(V, k, V.o_flags)[i] & 1)) {
    const int id = vo::kf_sec<int>(V, k, V.o_ids)[i];
    if (id >= 0) key = ((unsigned long long)(unsigned)id << 32) | (unsigned)e;
  }
  keys[e] = key;
}

// the steps j = min(k / 2, kObsChunk / 2) .. 1 of the stages k = k_lo .. k_hi on one chunk of kObsChunk keys, in LDS; the
// direction of a compare-exchange comes from the key's GLOBAL position
__global__ __launch_bounds__(256) void k_obs_sort_local(unsigned long long *keys, int k_lo, int k_hi) {
  __shared__ unsigned long long sk[kObsChunk];
  const int base = blockIdx.x * kObsChunk, tid = threadIdx.x;
  for (int i = tid; i < kObsChunk; i += 256) sk[i] = keys[base + i];
  for (int k = k_lo; k <= k_hi && k > 0; k <<= 1)
    for (int j = min(k >> 1, kObsChunk >> 1); j > 0; j >>= 1) {
      __syncthreads();
      for (int t = tid; t < kObsChunk / 2; t += 256) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const unsigned long long a = sk[i], b = sk[l];
        if ((a > b) == (((base + i) & k) == 0)) sk[i] = b, sk[l] = a;
      }
    }
  __syncthreads();
  for (int i = tid; i < kObsChunk; i += 256) keys[base + i] = sk[i];
}

// one step (k, j) with j >= kObsChunk: partners lie in different chunks
__global__ __launch_bounds__(256) void k_obs_sort_global(unsigned long long *keys, int n_keys, int k, int j) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_keys / 2) return;
  const int i = 2 * t - (t & (j - 1)), l = i + j;
  const unsigned long long a = keys[i], b = keys[l];
  if ((a > b) == ((i & k) == 0)) keys[i] = b, keys[l] = a;
}

// run[entry] = position of the first key that carries the entry's id (binary search below the key's own position)
__global__ __launch_bounds__(256) void k_obs_runs(const unsigned long long *keys, int n_keys, int *run) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_keys) return;
  const unsigned long long key = keys[s];
  if (key == ~0ull) return;
  const unsigned long long first = key & 0xffffffff00000000ull;
  int lo = 0, hi = s;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < first) lo = mid + 1;
    else hi = mid;
  }
  run[(unsigned)(key & 0xffffffffu)] = lo;
}

}  // namespace

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

int kfstore_obs_view(vo_kfstore *s, KfObsView *out) {
  if (!s || !out) return VO_ERR_INVALID;
  if (s->obs_dirty) {
    int n = kObsChunk;
    while ((long long)n < (long long)s->size * s->NK) n <<= 1;  // (<= okeys_cap: size <= max_kf)
    unsigned long long *keys = s->okeys.as<unsigned long long>();
    hipStream_t st = s->st;
    KfStoreView V = kfstore_view(s);
    hipLaunchKernelGGL(k_obs_fill, dim3(n / 256), dim3(256), 0, st, V, (const int *)((s->layers & kLayerCulling) ? s->X.erased : nullptr), keys, n);
    hipLaunchKernelGGL(k_obs_sort_local, dim3(n / kObsChunk), dim3(256), 0, st, keys, 2, kObsChunk);
    for (int k = 2 * kObsChunk; k <= n && k > 0; k <<= 1) {
      for (int j = k >> 1; j >= kObsChunk; j >>= 1)
        hipLaunchKernelGGL(k_obs_sort_global, dim3(n / 512), dim3(256), 0, st, keys, n, k, j);
      hipLaunchKernelGGL(k_obs_sort_local, dim3(n / kObsChunk), dim3(256), 0, st, keys, k, k);
    }
    hipLaunchKernelGGL(k_obs_runs, dim3(n / 256), dim3(256), 0, st, (const unsigned long long *)keys, n, s->orun.as<int>());
    VO_HIP_CHECK(hipGetLastError());
    s->obs_n = n, s->obs_dirty = false;
  }
  *out = KfObsView{s->graph.as<int>(), s->normals.as<double>(), s->okeys.as<unsigned long long>(), s->orun.as<int>(), s->obs_n};
  return VO_OK;
}

int need(const vo_kfstore *s, const char *W, unsigned layers) {
  static const char *const kEnable[] = {"connections", "culling", "mapping", "local_ba", "point_upkeep", "fuse", "loop", "pose_graph",
                                        "keyframe_create", "loop_fuse", "loop_correct", "loop_merge", "detect_loop"};
  if (!s) return VO_ERR_INVALID;
  const unsigned missing = layers & ~s->layers;
  if (!missing) return VO_OK;
  set_error("%s: vo_kfstore_enable_%s has not been called on this store", W, kEnable[__builtin_ctz(missing)]);
  return VO_ERR_INVALID;
}

int need_keyframe(const vo_kfstore *s, const char *W, int keyframe) {
  if (keyframe >= 0 && keyframe < s->size) return VO_OK;
  set_error("%s: key-frame %d outside [0, %d)", W, keyframe, s->size);
  return VO_ERR_INVALID;
}

int enable_begin(const vo_kfstore *s, const char *W, unsigned required, unsigned layer, bool args_ok) {
  VO_CHECK(need(s, W, required));
  if (!args_ok) return VO_ERR_INVALID;
  if (s->size != 0) {
    set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  return (s->layers & layer) ? kLayerEnabled : VO_OK;
}

int KfWindow::fetch(const uint8_t *dev_win, size_t win_bytes, bool record_only, hipStream_t st, const char *W) {
  VO_CHECK(copy_d2h(stage.data(), dev_win, record_only ? sizeof(rec) : win_bytes, st, W));
  VO_CHECK(stream_sync(st, W));
  memcpy(rec, stage.data(), sizeof(rec));
  rec_known = true;
  return VO_OK;
}

int KfWindow::check_apply(const char *W, unsigned long long store_gen, const uint8_t *dev_win, hipStream_t st) {
  if (!enqueued || gen != store_gen) {
    set_error("%s: no window, or the store has been changed since the last one", W);
    return VO_ERR_INVALID;
  }
  if (!rec_known) VO_CHECK(fetch(dev_win, 0, true, st, W));
  if (rec[kBaStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    set_error("%s: the last window is %s", W, rec[kBaStatus] == VO_KFSTORE_BA_WINDOW_EMPTY ? "empty" : "overflowed");
    return VO_ERR_INVALID;
  }
  return VO_OK;
}

}  // namespace vo

namespace {

// one key-frame's graph row (kfstore.h: kKfGraphInts) from the caller's lists, validated against [0, size)
int graph_row(const vo_kfstore *s, const char *call, int keyframe, int n_nb, const int32_t *nb, int n_ch, const int32_t *ch, int parent,
              int32_t *row) {
  if (n_nb < 0 || n_ch < 0 || (n_nb > 0 && !nb) || (n_ch > 0 && !ch) || parent < -1 || parent >= s->size) {
    vo::set_error("%s: key-frame %d: a negative count, a missing list, or parent %d outside [-1, %d)", call, keyframe, parent, s->size);
    return VO_ERR_INVALID;
  }
  if (n_nb > vo::kKfGraphNb || n_ch > vo::kKfGraphCh) {
    vo::set_error("%s: key-frame %d: %d neighbours / %d children, the store holds %d / %d per key-frame", call, keyframe, n_nb, n_ch,
                  vo::kKfGraphNb, vo::kKfGraphCh);
    return VO_ERR_CAPACITY;
  }
  for (int i = 0; i < vo::kKfGraphInts; i++) row[i] = -1;
  row[0] = n_nb, row[1] = n_ch, row[2] = parent, row[3] = 0;
  for (int i = 0; i < n_nb; i++) {
    if (nb[i] < 0 || nb[i] >= s->size) {
      vo::set_error("%s: key-frame %d: neighbour %d outside [0, %d)", call, keyframe, nb[i], s->size);
      return VO_ERR_INVALID;
    }
    row[4 + i] = nb[i];
  }
  for (int i = 0; i < n_ch; i++) {
    if (ch[i] < 0 || ch[i] >= s->size || (i > 0 && ch[i] <= ch[i - 1])) {
      vo::set_error("%s: key-frame %d: child %d outside [0, %d) or not in ascending order", call, keyframe, ch[i], s->size);
      return VO_ERR_INVALID;
    }
    row[16 + i] = ch[i];
  }
  return VO_OK;
}

int graph_has_writer(const char *call) {
  vo::set_error("%s: the store maintains its graph itself (vo_kfstore_enable_connections)", call);
  return VO_ERR_INVALID;
}

}  // namespace

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
  V.o_angle = o, o = vo::up16(o + NK * 4);
  V.o_mind = o, o = vo::up16(o + NK * 4);
  V.o_maxd = o, o = vo::up16(o + NK * 4);
  V.o_ids = o, o = vo::up16(o + NK * 4);
  V.o_node = o, o = vo::up16(o + NK * 4);
  V.o_start = o, o = vo::up16(o + (NK + 1) * 4);
  V.o_feat = o, o = vo::up16(o + NK * 4);
  V.o_points = o, o = vo::up16(o + NK * 24);
  V.o_desc = o, o = vo::up16(o + NK * 32);
  V.o_pdesc = o, o = vo::up16(o + NK * 32);
  V.o_flags = o, o = vo::up16(o + NK);
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
  // the graph (no neighbours, no children, no parent until set), the normals (zero until set) and the observation index
  {
    const size_t ents = (size_t)max_keyframes * NK;
    if (ents > ((size_t)1 << 30)) {
      vo::set_error("vo_kfstore_create: %zu feature entries, the observation index addresses 2^30", ents);
      return fail(VO_ERR_CAPACITY);
    }
    int cap = kObsChunk;
    while ((size_t)cap < ents) cap <<= 1;
    s->okeys_cap = cap;
    std::vector<int32_t> rows((size_t)max_keyframes * vo::kKfGraphInts, -1);
    for (int k = 0; k < max_keyframes; k++) rows[(size_t)k * vo::kKfGraphInts] = rows[(size_t)k * vo::kKfGraphInts + 1] = 0;
    if (s->graph.reserve(rows.size() * 4) != VO_OK || s->normals.reserve(ents * 24) != VO_OK || s->okeys.reserve((size_t)cap * 8) != VO_OK ||
        s->orun.reserve((size_t)cap * 4) != VO_OK)
      return fail(VO_ERR_HIP);
    if (hipMemcpy(s->graph.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(s->normals.p, 0, ents * 24) != hipSuccess || hipMemset(s->orun.p, 0, (size_t)cap * 4) != hipSuccess) {
      vo::set_error("vo_kfstore_create: initialising the graph and the normals failed");
      return fail(VO_ERR_HIP);
    }
  }
  *out = s;
  return VO_OK;
}

void vo_kfstore_destroy(vo_kfstore *s) {
  if (!s) return;
  if (s->ev_in) (void)hipEventDestroy(s->ev_in);
  if (s->ev_out) (void)hipEventDestroy(s->ev_out);
  if (s->conn) vo::connections_destroy(s->conn);
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
  s->obs_dirty = true, s->gen++;
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
  s->obs_dirty = true, s->gen++;
  return VO_OK;
}

int vo_kfstore_set_bad(vo_kfstore *s, int keyframe, int bad) {
  if (!s || keyframe < 0 || keyframe >= s->size) return VO_ERR_INVALID;
  s->gen++;
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
  s->obs_dirty = true, s->gen++;
  VO_HIP_CHECK(hipStreamSynchronize(s->st));
  return VO_OK;
}

int vo_kfstore_set_graph(vo_kfstore *s, int keyframe, int n_neighbors, const int32_t *neighbors, int n_children,
                         const int32_t *children, int parent) {
  if (!s || keyframe < 0 || keyframe >= s->size) return VO_ERR_INVALID;
  if (s->conn) return graph_has_writer("vo_kfstore_set_graph");
  int32_t row[vo::kKfGraphInts];
  VO_CHECK(graph_row(s, "vo_kfstore_set_graph", keyframe, n_neighbors, neighbors, n_children, children, parent, row));
  s->gen++;
  const char *W = "vo_kfstore_set_graph";
  VO_CHECK(vo::copy_h2d(s->graph.as<int>() + (size_t)keyframe * vo::kKfGraphInts, row, sizeof(row), s->st, W));
  return vo::stream_sync(s->st, W);  // (row is a local: the copy must have read it)
}

int vo_kfstore_set_graph_batch(vo_kfstore *s, int first, int count, const int32_t *n_neighbors, const int32_t *neighbors,
                               const int32_t *n_children, const int32_t *children, const int32_t *parent) {
  if (!s || first < 0 || count < 0 || first + (long long)count > s->size ||
      (count > 0 && (!n_neighbors || !neighbors || !n_children || !children || !parent)))
    return VO_ERR_INVALID;
  if (s->conn) return graph_has_writer("vo_kfstore_set_graph_batch");
  if (count == 0) return VO_OK;
  std::vector<int32_t> rows((size_t)count * vo::kKfGraphInts);
  for (int k = 0; k < count; k++)
    VO_CHECK(graph_row(s, "vo_kfstore_set_graph_batch", first + k, n_neighbors[k], neighbors + (size_t)k * vo::kKfGraphNb, n_children[k],
                       children + (size_t)k * vo::kKfGraphCh, parent[k], rows.data() + (size_t)k * vo::kKfGraphInts));
  const char *W = "vo_kfstore_set_graph_batch";
  s->gen++;
  VO_CHECK(vo::copy_h2d(s->graph.as<int>() + (size_t)first * vo::kKfGraphInts, rows.data(), rows.size() * 4, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_set_normals(vo_kfstore *s, int keyframe, const double *normals) {
  if (!s || keyframe < 0 || keyframe >= s->size) return VO_ERR_INVALID;
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!normals) return VO_ERR_INVALID;
  s->gen++;
  const char *W = "vo_kfstore_set_normals";
  VO_CHECK(vo::copy_h2d(s->normals.as<double>() + (size_t)keyframe * s->NK * 3, normals, n * 24, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_get_flags(vo_kfstore *s, int keyframe, uint8_t *flags, int32_t *bad) {
  const char *W = "vo_kfstore_get_flags";
  if (!s) return VO_ERR_INVALID;
  VO_CHECK(vo::need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  int32_t head[2] = {0, 0};
  VO_CHECK(vo::copy_d2h(head, s->record(keyframe), 8, s->st, W));
  if (flags && n > 0) VO_CHECK(vo::copy_d2h(flags, s->record(keyframe) + s->V.o_flags, n, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  if (bad) *bad = head[1];
  return VO_OK;
}

}  // extern "C"
