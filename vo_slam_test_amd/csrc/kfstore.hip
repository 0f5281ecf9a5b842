// kfstore.hip -- the key-frame feature store: everything the relocalisation route reads of a
// key-frame, resident on the device, addressed by the insertion number the key-frame database (kfdb.hip) uses.  One
// fixed-size record per key-frame (vo_common.h: KfStoreView), so that the host insert is one staging copy and the route's
// kernels reach a key-frame's arrays from its number alone.
#include "vo_common.h"

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
  // what vo_tracker_build_local_map reads beyond the records (vo_common.h: KfObsView)
  vo::OwnedDevBuf graph, normals, okeys, orun;
  int okeys_cap = 0;      // keys the index holds: the power of two above max_kf * NK, at least one chunk
  bool obs_dirty = true;  // an insert or update_points has happened since the index was built
  int obs_n = 0;          // keys the built index spans (a power of two covering size * NK)
  vo::KfConnections *conn = nullptr;  // vo_kfstore_enable_connections: the graph is then maintained on the device (section 4h)
  vo::OwnedDevBuf cull;               // vo_kfstore_enable_culling: the columns and words of section 4i
  vo::KfCullView X{};
  bool culling = false;
  vo::OwnedDevBuf map;                // vo_kfstore_enable_mapping: the arrays of section 4j
  vo::KfMapView M{};
  size_t map_bytes = 0;
  bool mapping = false;
  vo::OwnedDevBuf ba;                 // vo_kfstore_enable_local_ba: the arrays of section 4k
  vo::OwnedPinnedBuf ba_stage;        // the window coming down, or a solver's result going up: one copy each
  vo::KfBaView B{};
  bool local_ba = false;
  // the generation word: every call that writes the store advances it; an apply is valid for the window of its generation
  unsigned long long gen = 0, ba_gen = 0;
  bool ba_window = false, ba_rec_known = false;  // a window has been enqueued; its record has been fetched
  int32_t ba_rec[vo::kBaRecInts] = {0};
  std::vector<double> ba_poses, ba_points;  // the composed call's solver state (sized by the capacities: no allocation per call)
  std::vector<uint8_t> ba_erase;
  vo::OwnedDevBuf up;                 // vo_kfstore_enable_point_upkeep: the block of section 4l
  vo::OwnedPinnedBuf up_stage;        // a host form's lists going up: one copy
  vo::KfUpkeepView U{};
  bool upkeep = false;
  vo::OwnedDevBuf fu;                 // vo_kfstore_enable_fuse: the block of section 4m
  vo::KfFuseView F{};
  bool fuse = false;
  vo::OwnedDevBuf lp;                 // vo_kfstore_enable_loop: the block of section 4n
  vo::OwnedPinnedBuf lp_stage;        // a host form's candidates and rand() values going up, the results coming down: one copy each
  vo::KfLoopView L{};
  bool loop = false, loop_called = false;
  int loop_fix_scale = 1;             // of the last compute_sim3: what compute_sim3_continue refines with
  vo::OwnedDevBuf pg;                 // vo_kfstore_enable_pose_graph: the block of section 4o
  vo::OwnedPinnedBuf pg_stage;        // a window's inputs or a solver's result going up, the window coming down: one copy each
  vo::KfPgView P{};
  bool pose_graph = false, pg_window = false, pg_rec_known = false;
  unsigned long long pg_gen = 0;
  int32_t pg_rec[vo::kPgRecInts] = {0};
  int pg_counts[3] = {0, 0, 0};       // n_corr, n_lc, n_cp of the last window: where its inputs lie in P.in
  std::vector<int32_t> pg_ledge;      // the loop edges as the host knows them: [max_kf][1 + VO_KFSTORE_MAX_LOOP_EDGES], count first
  std::vector<double> pg_q, pg_t;     // the composed call's solver state (sized by the capacities: no allocation per call)
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

int kfstore_obs_view(vo_kfstore *s, KfObsView *out) {
  if (!s || !out) return VO_ERR_INVALID;
  if (s->obs_dirty) {
    int n = kObsChunk;
    while ((long long)n < (long long)s->size * s->NK) n <<= 1;  // (<= okeys_cap: size <= max_kf)
    unsigned long long *keys = s->okeys.as<unsigned long long>();
    hipStream_t st = s->st;
    KfStoreView V = kfstore_view(s);
    hipLaunchKernelGGL(k_obs_fill, dim3(n / 256), dim3(256), 0, st, V, (const int *)(s->culling ? s->X.erased : nullptr), keys, n);
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

}  // namespace vo

namespace {

// one key-frame's graph row (vo_common.h: kKfGraphInts) from the caller's lists, validated against [0, size)
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

int need_connections(const vo_kfstore *s, const char *call) {
  if (s && s->conn) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_connections has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_culling(const vo_kfstore *s, const char *call) {
  if (s && s->culling) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_culling has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_mapping(const vo_kfstore *s, const char *call) {
  if (s && s->mapping) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_mapping has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_local_ba(const vo_kfstore *s, const char *call) {
  if (s && s->local_ba) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_local_ba has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_upkeep(const vo_kfstore *s, const char *call) {
  if (s && s->upkeep) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_point_upkeep has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_fuse(const vo_kfstore *s, const char *call) {
  if (s && s->fuse) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_fuse has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_loop(const vo_kfstore *s, const char *call) {
  if (s && s->loop) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_loop has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_pose_graph(const vo_kfstore *s, const char *call) {
  if (s && s->pose_graph) return VO_OK;
  if (s) vo::set_error("%s: vo_kfstore_enable_pose_graph has not been called on this store", call);
  return VO_ERR_INVALID;
}

int need_keyframe(const vo_kfstore *s, const char *call, int keyframe) {
  if (keyframe >= 0 && keyframe < s->size) return VO_OK;
  vo::set_error("%s: key-frame %d outside [0, %d)", call, keyframe, s->size);
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

int vo_kfstore_enable_connections(vo_kfstore *s) {
  if (!s) return VO_ERR_INVALID;
  if (s->size != 0) {
    vo::set_error("vo_kfstore_enable_connections: the store holds %d key-frames, the call is valid on an empty store only", s->size);
    return VO_ERR_INVALID;
  }
  if (s->conn) return VO_OK;
  return vo::connections_create(&s->conn, s->max_kf, s->graph.as<int>(), s->st);
}

int vo_kfstore_enable_culling(vo_kfstore *s) {
  const char *W = "vo_kfstore_enable_culling";
  VO_CHECK(need_connections(s, W));
  if (s->size != 0) {
    vo::set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  if (s->culling) return VO_OK;
  VO_CHECK(s->cull.reserve(vo::cull_bytes(s->max_kf, s->NK)));
  s->X = vo::cull_layout(s->cull.p, s->max_kf, s->NK);
  VO_CHECK(vo::cull_init(s->X, s->max_kf, s->st));
  VO_CHECK(vo::stream_sync(s->st, W));
  vo::connections_set_erased(s->conn, s->X.erased);
  s->culling = true;
  return VO_OK;
}

int vo_kfstore_set_keypoints(vo_kfstore *s, int keyframe, const int32_t *octave, const float *depth, const float *u_right) {
  const char *W = "vo_kfstore_set_keypoints";
  VO_CHECK(need_culling(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe], NK = (size_t)s->NK;
  if (n == 0) return VO_OK;
  if (!octave || !depth || !u_right) return VO_ERR_INVALID;
  s->gen++;
  // the three columns of a key-frame lie side by side: staged whole (the defaults beyond n), one copy
  uint8_t *h = s->stage.data();  // (a record is longer than 12 bytes a feature)
  int32_t *ho = reinterpret_cast<int32_t *>(h);
  float *hd = reinterpret_cast<float *>(h) + NK, *hu = hd + NK;
  for (size_t i = 0; i < NK; i++) ho[i] = i < n ? octave[i] : 0, hd[i] = i < n ? depth[i] : -1.f, hu[i] = i < n ? u_right[i] : -1.f;
  VO_CHECK(vo::copy_h2d(vo::cull_octave(s->X, keyframe), h, NK * 12, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_set_keypoints_dev(vo_kfstore *s, int keyframe, const int32_t *dev_octave, const float *dev_depth, const float *dev_u_right) {
  const char *W = "vo_kfstore_set_keypoints_dev";
  VO_CHECK(need_culling(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!dev_octave || !dev_depth || !dev_u_right) return VO_ERR_INVALID;
  s->gen++;
  VO_HIP_CHECK(hipMemcpyAsync(vo::cull_octave(s->X, keyframe), dev_octave, n * 4, hipMemcpyDeviceToDevice, s->st));
  VO_HIP_CHECK(hipMemcpyAsync(vo::cull_depth(s->X, keyframe), dev_depth, n * 4, hipMemcpyDeviceToDevice, s->st));
  VO_HIP_CHECK(hipMemcpyAsync(vo::cull_uright(s->X, keyframe), dev_u_right, n * 4, hipMemcpyDeviceToDevice, s->st));
  return VO_OK;
}

int vo_kfstore_set_erase_lock(vo_kfstore *s, int keyframe, int on) {
  const char *W = "vo_kfstore_set_erase_lock";
  VO_CHECK(need_culling(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  s->gen++;
  return vo::cull_set_lock(s->X, keyframe, on, s->st);
}

int vo_kfstore_cull_keyframes(vo_kfstore *s, int current, float th_depth) {
  const char *W = "vo_kfstore_cull_keyframes";
  VO_CHECK(need_culling(s, W));
  VO_CHECK(need_keyframe(s, W, current));
  // (that `current` has not been erased only the device knows: the kernels then walk no candidate and raise the sticky
  //  VO_KFSTORE_CONNECTIONS_INVALID)
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  VO_CHECK(vo::cull_enqueue(vo::kfstore_view(s), O, vo::connections_view(s->conn), s->X, current, th_depth, s->st));
  s->obs_dirty = true, s->gen++;  // (whether anything was erased only the device knows)
  return vo::connections_order(s->conn, s->size, s->st);
}

int vo_kfstore_erase_keyframe(vo_kfstore *s, int keyframe) {
  const char *W = "vo_kfstore_erase_keyframe";
  VO_CHECK(need_culling(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  VO_CHECK(vo::erase_enqueue(vo::kfstore_view(s), O, vo::connections_view(s->conn), s->X, keyframe, s->st));
  s->obs_dirty = true, s->gen++;
  return vo::connections_order(s->conn, s->size, s->st);
}

int vo_kfstore_cull_result(vo_kfstore *s, int32_t *n_candidates, int32_t *keyframes, int32_t *mp_cnt, int32_t *re_obs, int32_t *decision) {
  const char *W = "vo_kfstore_cull_result";
  VO_CHECK(need_culling(s, W));
  if (!n_candidates) return VO_ERR_INVALID;
  std::vector<int32_t> rec((size_t)s->size * 4 + 4);
  int32_t n = 0;
  VO_CHECK(vo::copy_d2h(&n, s->X.n_rec, 4, s->st, W));
  if (s->size > 0) VO_CHECK(vo::copy_d2h(rec.data(), s->X.rec, (size_t)s->size * 16, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  n = std::min(std::max(n, 0), s->size);
  *n_candidates = n;
  for (int t = 0; t < n; t++) {
    if (keyframes) keyframes[t] = rec[(size_t)t * 4];
    if (mp_cnt) mp_cnt[t] = rec[(size_t)t * 4 + 1];
    if (re_obs) re_obs[t] = rec[(size_t)t * 4 + 2];
    if (decision) decision[t] = rec[(size_t)t * 4 + 3];
  }
  return VO_OK;
}

int vo_kfstore_cull_state(vo_kfstore *s, int keyframe, int32_t *erased, int32_t *locked, int32_t *pending) {
  const char *W = "vo_kfstore_cull_state";
  VO_CHECK(need_culling(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  int32_t w[3] = {0, 0, 0};
  VO_CHECK(vo::copy_d2h(w, s->X.erased + keyframe, 4, s->st, W));
  VO_CHECK(vo::copy_d2h(w + 1, s->X.locked + keyframe, 4, s->st, W));
  VO_CHECK(vo::copy_d2h(w + 2, s->X.pending + keyframe, 4, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  if (erased) *erased = w[0];
  if (locked) *locked = w[1];
  if (pending) *pending = w[2];
  return VO_OK;
}

int vo_kfstore_get_flags(vo_kfstore *s, int keyframe, uint8_t *flags, int32_t *bad) {
  const char *W = "vo_kfstore_get_flags";
  if (!s) return VO_ERR_INVALID;
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  int32_t head[2] = {0, 0};
  VO_CHECK(vo::copy_d2h(head, s->record(keyframe), 8, s->st, W));
  if (flags && n > 0) VO_CHECK(vo::copy_d2h(flags, s->record(keyframe) + s->V.o_flags, n, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  if (bad) *bad = head[1];
  return VO_OK;
}

int vo_kfstore_enable_mapping(vo_kfstore *s, const float cam[6], int n_levels, const float *scale_factors, int32_t first_point_id) {
  const char *W = "vo_kfstore_enable_mapping";
  VO_CHECK(need_culling(s, W));
  if (!cam || !scale_factors || n_levels < 1 || n_levels > 16 || first_point_id < 0) return VO_ERR_INVALID;
  if (s->size != 0) {
    vo::set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  if (s->mapping) return VO_OK;
  if (s->NK > 16384) {
    vo::set_error("%s: %d features per key-frame, the search kernel handles 16384", W, s->NK);
    return VO_ERR_CAPACITY;
  }
  s->map_bytes = vo::mapping_bytes(s->max_kf, s->NK);
  VO_CHECK(s->map.reserve(s->map_bytes));
  s->M = vo::mapping_layout(s->map.p, s->max_kf, s->NK);
  s->M.n_levels = n_levels;
  for (int i = 0; i < 6; i++) s->M.cam[i] = cam[i];
  for (int i = 0; i < 16; i++) s->M.sf[i] = scale_factors[i < n_levels ? i : n_levels - 1];
  VO_CHECK(vo::mapping_init(s->M, s->map_bytes, first_point_id, s->st));
  VO_CHECK(vo::stream_sync(s->st, W));
  s->mapping = true;
  return VO_OK;
}

int vo_kfstore_set_pose(vo_kfstore *s, int keyframe, const double *Tcw12) {
  const char *W = "vo_kfstore_set_pose";
  VO_CHECK(need_mapping(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  if (!Tcw12) return VO_ERR_INVALID;
  s->gen++;
  // the pose-set word lies behind the pose (the thirteenth slot): one copy
  double *h = reinterpret_cast<double *>(s->stage.data());
  memcpy(h, Tcw12, 96);
  const int32_t one[2] = {1, 0};
  memcpy(h + 12, one, 8);
  VO_CHECK(vo::copy_h2d(vo::np_pose(s->M, keyframe), h, vo::kNpPoseDoubles * 8, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_set_pose_dev(vo_kfstore *s, int keyframe, const double *dev_Tcw12) {
  const char *W = "vo_kfstore_set_pose_dev";
  VO_CHECK(need_mapping(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  if (!dev_Tcw12) return VO_ERR_INVALID;
  s->gen++;
  return vo::mapping_set_pose_dev(s->M, keyframe, dev_Tcw12, s->st);
}

int vo_kfstore_set_keypoint_xy(vo_kfstore *s, int keyframe, const float *xy) {
  const char *W = "vo_kfstore_set_keypoint_xy";
  VO_CHECK(need_mapping(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe], NK = (size_t)s->NK;
  if (n == 0) return VO_OK;
  if (!xy) return VO_ERR_INVALID;
  s->gen++;
  // the two columns of a key-frame lie side by side: staged whole (zero beyond n), one copy
  float *hx = reinterpret_cast<float *>(s->stage.data()), *hy = hx + NK;  // (a record is longer than 8 bytes a feature)
  for (size_t i = 0; i < NK; i++) hx[i] = i < n ? xy[2 * i] : 0.f, hy[i] = i < n ? xy[2 * i + 1] : 0.f;
  VO_CHECK(vo::copy_h2d(vo::np_x(s->M, keyframe), hx, NK * 8, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_set_keypoint_xy_dev(vo_kfstore *s, int keyframe, const float *dev_xy) {
  const char *W = "vo_kfstore_set_keypoint_xy_dev";
  VO_CHECK(need_mapping(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const int n = s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!dev_xy) return VO_ERR_INVALID;
  s->gen++;
  return vo::mapping_split_xy(s->M, keyframe, n, dev_xy, s->st);
}

int vo_kfstore_next_point_id(vo_kfstore *s, int32_t *id) {
  const char *W = "vo_kfstore_next_point_id";
  VO_CHECK(need_mapping(s, W));
  if (!id) return VO_ERR_INVALID;
  VO_CHECK(vo::copy_d2h(id, s->M.counter, 4, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_create_map_points(vo_kfstore *s, int current, int max_neighbors) {
  const char *W = "vo_kfstore_create_map_points";
  VO_CHECK(need_mapping(s, W));
  VO_CHECK(need_keyframe(s, W, current));
  if (max_neighbors < 1 || max_neighbors > vo::kKfGraphNb) {
    vo::set_error("%s: max_neighbors %d outside [1, %d]", W, max_neighbors, vo::kKfGraphNb);
    return VO_ERR_INVALID;
  }
  // (that `current` has been erased or has no pose only the device knows: k_tri_walk then reaches no neighbour and raises
  //  the sticky VO_KFSTORE_CONNECTIONS_INVALID)
  const vo::KfStoreView V = vo::kfstore_view(s);
  const vo::KfConnView C = vo::connections_view(s->conn);
  for (int i = 0; i < max_neighbors; i++) {  // step i + 1 reads the flags step i wrote: walk, replay, create per neighbour
    VO_CHECK(vo::tri_walk_replay(V, s->X, s->M, s->graph.as<int>(), C.status, current, i, s->st));
    VO_CHECK(vo::np_create(V, s->X, s->M, s->normals.as<double>(), s->local_ba ? s->B.ref_kf : nullptr, current, i, s->st));
  }
  s->obs_dirty = true, s->gen++;  // (whether anything was created only the device knows)
  if (s->upkeep) VO_CHECK(vo::upkeep_created_enqueue(s->M, s->U, C.status, current, s->st));  // addedMapPoints_.push_back (:355)
  return VO_OK;
}

int vo_kfstore_new_points_result(vo_kfstore *s, int32_t *n_neighbors, int32_t *neighbor_kf, int32_t *status, int32_t *n_matches,
                                 int32_t *n_created, int32_t *created, int created_capacity) {
  const char *W = "vo_kfstore_new_points_result";
  VO_CHECK(need_mapping(s, W));
  if (!n_neighbors || created_capacity < 0 || (created_capacity > 0 && !created)) return VO_ERR_INVALID;
  int32_t rec[vo::kNpRecInts] = {0};
  VO_CHECK(vo::copy_d2h(rec, s->M.rec, sizeof(rec), s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  const int n = std::min(std::max(rec[0], 0), vo::kKfGraphNb);
  const int total = std::min(std::max(rec[1], 0), vo::kKfGraphNb * s->NK);
  *n_neighbors = n;
  for (int i = 0; i < vo::kKfGraphNb; i++) {
    if (neighbor_kf) neighbor_kf[i] = i < n ? rec[4 + 4 * i] : -1;
    if (status) status[i] = i < n ? rec[4 + 4 * i + 1] : VO_KFSTORE_NP_NOT_REACHED;
    if (n_matches) n_matches[i] = i < n ? rec[4 + 4 * i + 2] : 0;
    if (n_created) n_created[i] = i < n ? rec[4 + 4 * i + 3] : 0;
  }
  const int rows = std::min(total, created_capacity);
  if (rows > 0) {
    VO_CHECK(vo::copy_d2h(created, s->M.created, (size_t)rows * 16, s->st, W));
    VO_CHECK(vo::stream_sync(s->st, W));
  }
  if (total > created_capacity) {
    vo::set_error("%s: the call created %d points, created_capacity is %d", W, total, created_capacity);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

int vo_kfstore_get_points(vo_kfstore *s, int keyframe, uint8_t *flags, int32_t *ids, double *points, uint8_t *point_desc,
                          float *min_distance, float *max_distance, double *normals) {
  const char *W = "vo_kfstore_get_points";
  if (!s) return VO_ERR_INVALID;
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  const vo::KfStoreView &V = s->V;
  const uint8_t *r = s->record(keyframe);
  if (flags) VO_CHECK(vo::copy_d2h(flags, r + V.o_flags, n, s->st, W));
  if (ids) VO_CHECK(vo::copy_d2h(ids, r + V.o_ids, n * 4, s->st, W));
  if (points) VO_CHECK(vo::copy_d2h(points, r + V.o_points, n * 24, s->st, W));
  if (point_desc) VO_CHECK(vo::copy_d2h(point_desc, r + V.o_pdesc, n * 32, s->st, W));
  if (min_distance) VO_CHECK(vo::copy_d2h(min_distance, r + V.o_mind, n * 4, s->st, W));
  if (max_distance) VO_CHECK(vo::copy_d2h(max_distance, r + V.o_maxd, n * 4, s->st, W));
  if (normals) VO_CHECK(vo::copy_d2h(normals, s->normals.as<double>() + (size_t)keyframe * s->NK * 3, n * 24, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_get_pose(vo_kfstore *s, int keyframe, double *Tcw12, int32_t *pose_set) {
  const char *W = "vo_kfstore_get_pose";
  VO_CHECK(need_mapping(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  double h[vo::kNpPoseDoubles];
  VO_CHECK(vo::copy_d2h(h, vo::np_pose(s->M, keyframe), sizeof(h), s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  if (Tcw12) memcpy(Tcw12, h, 96);
  if (pose_set) memcpy(pose_set, h + 12, 4);
  return VO_OK;
}

int vo_kfstore_enable_local_ba(vo_kfstore *s, int max_cams, int max_points, int max_edges) {
  const char *W = "vo_kfstore_enable_local_ba";
  VO_CHECK(need_mapping(s, W));
  if (max_cams < 1 || max_points < 1 || max_edges < 1) return VO_ERR_INVALID;
  if (s->size != 0) {
    vo::set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  if (s->local_ba) return VO_OK;
  VO_CHECK(s->ba.reserve(vo::ba_store_bytes(s->max_kf, s->NK, max_cams, max_points, max_edges)));
  s->B = vo::ba_store_layout(s->ba.p, s->max_kf, s->NK, max_cams, max_points, max_edges);
  VO_CHECK(s->ba_stage.reserve(std::max(s->B.win_bytes, s->B.in_bytes)));
  s->ba_poses.resize((size_t)max_cams * 6), s->ba_points.resize((size_t)max_points * 3), s->ba_erase.resize((size_t)max_edges + 1);
  VO_CHECK(vo::ba_store_init(s->B, s->max_kf, s->st));
  VO_CHECK(vo::stream_sync(s->st, W));
  s->local_ba = true;
  return VO_OK;
}

int vo_kfstore_set_point_refs(vo_kfstore *s, int keyframe, const int32_t *ref_kf) {
  const char *W = "vo_kfstore_set_point_refs";
  VO_CHECK(need_local_ba(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!ref_kf) return VO_ERR_INVALID;
  for (size_t i = 0; i < n; i++)
    if (ref_kf[i] < -1 || ref_kf[i] >= s->size) {
      vo::set_error("%s: feature %zu: reference key-frame %d outside [-1, %d)", W, i, ref_kf[i], s->size);
      return VO_ERR_INVALID;
    }
  s->gen++;
  VO_CHECK(vo::copy_h2d(s->B.ref_kf + (size_t)keyframe * s->NK, ref_kf, n * 4, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_set_point_refs_dev(vo_kfstore *s, int keyframe, const int32_t *dev_ref_kf) {
  const char *W = "vo_kfstore_set_point_refs_dev";
  VO_CHECK(need_local_ba(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!dev_ref_kf) return VO_ERR_INVALID;
  s->gen++;
  VO_HIP_CHECK(hipMemcpyAsync(s->B.ref_kf + (size_t)keyframe * s->NK, dev_ref_kf, n * 4, hipMemcpyDeviceToDevice, s->st));
  return VO_OK;
}

int vo_kfstore_get_point_refs(vo_kfstore *s, int keyframe, int32_t *ref_kf) {
  const char *W = "vo_kfstore_get_point_refs";
  VO_CHECK(need_local_ba(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!ref_kf) return VO_ERR_INVALID;
  VO_CHECK(vo::copy_d2h(ref_kf, s->B.ref_kf + (size_t)keyframe * s->NK, n * 4, s->st, W));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_local_ba_window(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_local_ba_window";
  VO_CHECK(need_local_ba(s, W));
  VO_CHECK(need_keyframe(s, W, current));
  // (that `current` has been erased, or that a camera has no pose, only the device knows: the window is then empty)
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  VO_CHECK(vo::ba_window_enqueue(vo::kfstore_view(s), O, vo::connections_view(s->conn), s->X, s->M, s->B, current, s->st));
  s->ba_window = true, s->ba_rec_known = false, s->ba_gen = s->gen;
  return VO_OK;
}

}  // extern "C"

namespace {

// the window as one copy into the staging block; the record is then known on the host
int ba_fetch_window(vo_kfstore *s, const char *W, bool record_only) {
  VO_CHECK(vo::copy_d2h(s->ba_stage.data(), s->B.win, record_only ? sizeof(s->ba_rec) : s->B.win_bytes, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  memcpy(s->ba_rec, s->ba_stage.data(), sizeof(s->ba_rec));
  s->ba_rec_known = true;
  return VO_OK;
}

template <class T>
const T *ba_staged(const vo_kfstore *s, const T *dev) {
  return reinterpret_cast<const T *>(s->ba_stage.data() + (reinterpret_cast<const uint8_t *>(dev) - s->B.win));
}

}  // namespace

extern "C" {

int vo_kfstore_local_ba_window_result(vo_kfstore *s, int32_t *record, int32_t *cam_keyframe, uint8_t *cam_fixed, double *poses6,
                                      int32_t *point_id, double *points, int32_t *edge_cam, int32_t *edge_point,
                                      int32_t *edge_feature, double *edge_obs, double *edge_inv_sigma) {
  const char *W = "vo_kfstore_local_ba_window_result";
  VO_CHECK(need_local_ba(s, W));
  VO_CHECK(ba_fetch_window(s, W, false));
  const int32_t *r = s->ba_rec;
  if (record) memcpy(record, r, sizeof(s->ba_rec));
  if (r[vo::kBaStatus] != VO_KFSTORE_BA_WINDOW_OK) return VO_OK;
  const size_t nc = (size_t)r[vo::kBaNCams], np = (size_t)r[vo::kBaNPoints], ne = (size_t)r[vo::kBaNEdges];
  const vo::KfBaView &B = s->B;
  if (cam_keyframe) memcpy(cam_keyframe, ba_staged(s, B.cam_kf), nc * 4);
  if (cam_fixed) memcpy(cam_fixed, ba_staged(s, B.cam_fixed), nc);
  if (poses6) memcpy(poses6, ba_staged(s, B.poses6), nc * 48);
  if (point_id) memcpy(point_id, ba_staged(s, B.pt_id), np * 4);
  if (points) memcpy(points, ba_staged(s, B.points), np * 24);
  if (edge_cam) memcpy(edge_cam, ba_staged(s, B.e_cam), ne * 4);
  if (edge_point) memcpy(edge_point, ba_staged(s, B.e_pt), ne * 4);
  if (edge_feature) memcpy(edge_feature, ba_staged(s, B.e_feat), ne * 4);
  if (edge_obs) memcpy(edge_obs, ba_staged(s, B.e_obs), ne * 24);
  if (edge_inv_sigma) memcpy(edge_inv_sigma, ba_staged(s, B.e_isg), ne * 8);
  return VO_OK;
}

int vo_kfstore_local_ba_apply(vo_kfstore *s, const double *poses6, const double *points, const uint8_t *edge_erase) {
  const char *W = "vo_kfstore_local_ba_apply";
  VO_CHECK(need_local_ba(s, W));
  if (!s->ba_window || s->ba_gen != s->gen) {
    vo::set_error("%s: no window, or the store has been changed since the last one", W);
    return VO_ERR_INVALID;
  }
  if (!s->ba_rec_known) VO_CHECK(ba_fetch_window(s, W, true));
  const int32_t *r = s->ba_rec;
  if (r[vo::kBaStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    vo::set_error("%s: the last window is %s", W, r[vo::kBaStatus] == VO_KFSTORE_BA_WINDOW_EMPTY ? "empty" : "overflowed");
    return VO_ERR_INVALID;
  }
  const size_t nc = (size_t)r[vo::kBaNCams], np = (size_t)r[vo::kBaNPoints], ne = (size_t)r[vo::kBaNEdges];
  if (!poses6 || (np > 0 && !points) || (ne > 0 && !edge_erase)) return VO_ERR_INVALID;
  // staged as the kernels read it: Tcw12 per camera (SE3::exp on the host, :786-788) | points | erase bytes
  uint8_t *h = s->ba_stage.data();
  double *T = reinterpret_cast<double *>(h);
  for (size_t c = 0; c < nc; c++) VO_CHECK(vo_se3_exp(poses6 + 6 * c, T + 12 * c, T + 12 * c + 9));
  if (np) memcpy(h + nc * 96, points, np * 24);
  if (ne) memcpy(h + nc * 96 + np * 24, edge_erase, ne);
  const size_t bytes = nc * 96 + np * 24 + ne;
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));  // (not stale: nothing has changed since the window)
  VO_CHECK(vo::copy_h2d(s->B.in, h, bytes, s->st, W));
  VO_CHECK(vo::ba_apply_enqueue(vo::kfstore_view(s), O, s->X, s->M, s->B, s->normals.as<double>(), vo::connections_view(s->conn).status,
                                (int)nc, (int)np, (int)ne, s->st));
  s->obs_dirty = true, s->gen++;
  return vo::stream_sync(s->st, W);  // (the staging block is free again)
}

int vo_kfstore_refresh_points(vo_kfstore *s, int n, const int32_t *ids) {
  const char *W = "vo_kfstore_refresh_points";
  VO_CHECK(need_local_ba(s, W));
  if (n < 0 || (n > 0 && !ids)) return VO_ERR_INVALID;
  if (n > s->B.max_points) {
    vo::set_error("%s: %d ids, the store was enabled for %d points", W, n, s->B.max_points);
    return VO_ERR_CAPACITY;
  }
  for (int i = 0; i < n; i++)
    if (ids[i] < 0) {
      vo::set_error("%s: entry %d: id %d is negative", W, i, ids[i]);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  VO_CHECK(vo::copy_h2d(s->B.ids_in, ids, (size_t)n * 4, s->st, W));
  VO_CHECK(vo::ba_refresh_enqueue(vo::kfstore_view(s), O, s->X, s->M, s->B, s->normals.as<double>(), vo::connections_view(s->conn).status, n,
                                  s->st));
  s->gen++;  // (flags and ids stay: the index does not go stale)
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_local_ba(vo_kfstore *s, vo_ba *ba, int current, const volatile unsigned char *stop, vo_lm_summary *summaries) {
  const char *W = "vo_kfstore_local_ba";
  VO_CHECK(need_local_ba(s, W));
  if (!ba) return VO_ERR_INVALID;
  VO_CHECK(vo_kfstore_local_ba_window(s, current));
  VO_CHECK(ba_fetch_window(s, W, false));  // the ONE device-to-host copy
  const int32_t *r = s->ba_rec;
  if (r[vo::kBaStatus] == VO_KFSTORE_BA_WINDOW_OVERFLOW) {
    vo::set_error("%s: %d cameras, %d points, %d edges; the store was enabled for %d, %d, %d", W, r[vo::kBaNCams], r[vo::kBaNPoints],
                  r[vo::kBaNEdges], s->B.max_cams, s->B.max_points, s->B.max_edges);
    return VO_ERR_CAPACITY;
  }
  if (r[vo::kBaStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    vo::set_error("%s: the window of key-frame %d is empty (erased, or a camera without a pose)", W, current);
    return VO_ERR_INVALID;
  }
  const vo::KfBaView &B = s->B;
  const double cam[5] = {s->M.cam[0], s->M.cam[1], s->M.cam[2], s->M.cam[3], s->M.cam[4]};  // float members widened (:543-548)
  VO_CHECK(vo_ba_reset(ba, r[vo::kBaNCams], ba_staged(s, B.poses6), ba_staged(s, B.cam_fixed), r[vo::kBaNPoints], ba_staged(s, B.points),
                       r[vo::kBaNEdges], ba_staged(s, B.e_cam), ba_staged(s, B.e_pt), ba_staged(s, B.e_obs), ba_staged(s, B.e_isg), cam));
  VO_CHECK(vo_ba_local_ba(ba, stop, s->ba_erase.data(), summaries));  // (VO_ERR_STOPPED: the return at :594, no write-back)
  VO_CHECK(vo_ba_get_state(ba, s->ba_poses.data(), s->ba_points.data()));
  return vo_kfstore_local_ba_apply(s, s->ba_poses.data(), s->ba_points.data(), s->ba_erase.data());
}

// ---- the loop pose graph from the store
int vo_kfstore_enable_pose_graph(vo_kfstore *s, int max_edges, int max_corrected, int max_corrected_points) {
  const char *W = "vo_kfstore_enable_pose_graph";
  VO_CHECK(need_local_ba(s, W));
  if (max_edges < 1 || max_corrected < 1 || max_corrected_points < 1) return VO_ERR_INVALID;
  if (s->size != 0) {
    vo::set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  if (s->pose_graph) return VO_OK;
  VO_CHECK(s->pg.reserve(vo::pg_store_bytes(s->max_kf, s->NK, max_edges, max_corrected, max_corrected_points)));
  s->P = vo::pg_store_layout(s->pg.p, s->max_kf, s->NK, max_edges, max_corrected, max_corrected_points);
  VO_CHECK(s->pg_stage.reserve(std::max(s->P.win_bytes, std::max(s->P.in_bytes, s->P.sol_bytes))));
  s->pg_ledge.assign((size_t)s->max_kf * (1 + VO_KFSTORE_MAX_LOOP_EDGES), 0);
  s->pg_q.resize((size_t)s->P.max_nodes * 4), s->pg_t.resize((size_t)s->P.max_nodes * 3);
  VO_CHECK(vo::pg_store_init(s->P, s->st));
  VO_CHECK(vo::stream_sync(s->st, W));
  s->pose_graph = true;
  return VO_OK;
}

int vo_kfstore_add_loop_edge(vo_kfstore *s, int a, int b) {
  const char *W = "vo_kfstore_add_loop_edge";
  VO_CHECK(need_pose_graph(s, W));
  VO_CHECK(need_keyframe(s, W, a));
  VO_CHECK(need_keyframe(s, W, b));
  if (a == b) {
    vo::set_error("%s: key-frame %d cannot be its own loop edge", W, a);
    return VO_ERR_INVALID;
  }
  const int stride = 1 + VO_KFSTORE_MAX_LOOP_EDGES;
  int32_t *ra = s->pg_ledge.data() + (size_t)a * stride, *rb = s->pg_ledge.data() + (size_t)b * stride;
  const bool a_has = std::find(ra + 1, ra + 1 + ra[0], b) != ra + 1 + ra[0], b_has = std::find(rb + 1, rb + 1 + rb[0], a) != rb + 1 + rb[0];
  if ((!a_has && ra[0] >= VO_KFSTORE_MAX_LOOP_EDGES) || (!b_has && rb[0] >= VO_KFSTORE_MAX_LOOP_EDGES)) {
    vo::set_error("%s: key-frame %d or %d holds %d loop edges already", W, a, b, VO_KFSTORE_MAX_LOOP_EDGES);
    return VO_ERR_CAPACITY;
  }
  if (!a_has) ra[1 + ra[0]++] = b;
  if (!b_has) rb[1 + rb[0]++] = a;
  s->gen++;
  return vo::pg_add_loop_edge(s->P, s->X, a, b, s->st);  // (a repeat still sets both locks, as addLoopEdge does)
}

int vo_kfstore_get_loop_edges(vo_kfstore *s, int keyframe, int32_t *n, int32_t *edges) {
  const char *W = "vo_kfstore_get_loop_edges";
  VO_CHECK(need_pose_graph(s, W));
  VO_CHECK(need_keyframe(s, W, keyframe));
  int32_t h[1 + VO_KFSTORE_MAX_LOOP_EDGES];
  VO_CHECK(vo::copy_d2h(h, s->P.n_ledge + keyframe, 4, s->st, W));
  VO_CHECK(vo::copy_d2h(h + 1, s->P.ledge + (size_t)keyframe * VO_KFSTORE_MAX_LOOP_EDGES, VO_KFSTORE_MAX_LOOP_EDGES * 4, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  const int cnt = std::min(std::max(h[0], 0), VO_KFSTORE_MAX_LOOP_EDGES);
  if (n) *n = cnt;
  if (edges) memcpy(edges, h + 1, (size_t)cnt * 4);
  return VO_OK;
}

}  // extern "C"

namespace {

int pg_check_counts(const vo_kfstore *s, const char *W, int curr, int match, int n_corr, int n_lc, int n_cp) {
  VO_CHECK(need_keyframe(s, W, curr));
  VO_CHECK(need_keyframe(s, W, match));
  if (n_corr < 0 || n_lc < 0 || n_cp < 0) return VO_ERR_INVALID;
  if (n_corr > s->P.max_corr || n_lc > s->P.max_edges || n_cp > s->P.max_cp) {
    vo::set_error("%s: %d corrected key-frames, %d loop connections, %d corrected points; the store was enabled for %d, %d, %d", W, n_corr,
                  n_lc, n_cp, s->P.max_corr, s->P.max_edges, s->P.max_cp);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

int pg_enqueue_window(vo_kfstore *s, int curr, int match, int n_corr, int n_lc, int n_cp) {
  const vo::PgInputs I = vo::pg_inputs(s->P.in, n_corr, n_lc, n_cp);
  VO_CHECK(vo::pg_window_enqueue(vo::kfstore_view(s), vo::connections_view(s->conn), s->X, s->M, s->P, I, curr, match, s->st));
  s->pg_counts[0] = n_corr, s->pg_counts[1] = n_lc, s->pg_counts[2] = n_cp;
  s->pg_window = true, s->pg_rec_known = false, s->pg_gen = s->gen;
  return VO_OK;
}

// the window as one copy into the staging block; the record is then known on the host
int pg_fetch_window(vo_kfstore *s, const char *W, bool record_only) {
  VO_CHECK(vo::copy_d2h(s->pg_stage.data(), s->P.win, record_only ? sizeof(s->pg_rec) : s->P.win_bytes, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  memcpy(s->pg_rec, s->pg_stage.data(), sizeof(s->pg_rec));
  s->pg_rec_known = true;
  return VO_OK;
}

template <class T>
T *pg_staged(const vo_kfstore *s, const T *dev) {
  return reinterpret_cast<T *>(s->pg_stage.data() + (reinterpret_cast<const uint8_t *>(dev) - s->P.win));
}

}  // namespace

extern "C" {

int vo_kfstore_pose_graph_window(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *corr_kf, const double *S_corr,
                                 const double *S_uncorr, const int32_t *lc_start, const int32_t *lc_kf, int n_cp, const int32_t *cp_id,
                                 const int32_t *cp_ref) {
  const char *W = "vo_kfstore_pose_graph_window";
  VO_CHECK(need_pose_graph(s, W));
  if (n_corr < 0 || n_cp < 0 || !lc_start || (n_corr > 0 && (!corr_kf || !S_corr || !S_uncorr)) || (n_cp > 0 && (!cp_id || !cp_ref)))
    return VO_ERR_INVALID;
  if (lc_start[0] != 0 || lc_start[n_corr] < 0 || (lc_start[n_corr] > 0 && !lc_kf)) {
    vo::set_error("%s: the loop connections do not start at 0, or end at %d without a list", W, lc_start[n_corr]);
    return VO_ERR_INVALID;
  }
  const int n_lc = lc_start[n_corr];
  VO_CHECK(pg_check_counts(s, W, curr, match, n_corr, n_lc, n_cp));
  for (int r = 0; r < n_corr; r++) {
    if (corr_kf[r] < 0 || corr_kf[r] >= s->size || (r > 0 && corr_kf[r - 1] >= corr_kf[r])) {
      vo::set_error("%s: corrected key-frame %d (entry %d) outside [0, %d) or not in ascending order", W, corr_kf[r], r, s->size);
      return VO_ERR_INVALID;
    }
    if (lc_start[r + 1] < lc_start[r] || lc_start[r + 1] > n_lc) {
      vo::set_error("%s: the loop connections of entry %d run from %d to %d of %d", W, r, lc_start[r], lc_start[r + 1], n_lc);
      return VO_ERR_INVALID;
    }
    for (int e = lc_start[r]; e < lc_start[r + 1]; e++)
      if (lc_kf[e] < 0 || lc_kf[e] >= s->size || (e > lc_start[r] && lc_kf[e - 1] >= lc_kf[e])) {
        vo::set_error("%s: loop connection %d of key-frame %d outside [0, %d) or not in ascending order", W, lc_kf[e], corr_kf[r], s->size);
        return VO_ERR_INVALID;
      }
  }
  for (int e = 0; e < n_cp; e++)
    if (cp_id[e] < 0 || (e > 0 && cp_id[e - 1] >= cp_id[e]) || cp_ref[e] < 0 || cp_ref[e] >= s->size) {
      vo::set_error("%s: corrected point %d (entry %d) negative or not in ascending order, or its reference %d outside [0, %d)", W, cp_id[e],
                    e, cp_ref[e], s->size);
      return VO_ERR_INVALID;
    }
  const vo::PgInputs H = vo::pg_inputs(s->pg_stage.data(), n_corr, n_lc, n_cp);
  memcpy(H.S_corr, S_corr, (size_t)n_corr * 64), memcpy(H.S_unc, S_uncorr, (size_t)n_corr * 64);
  memcpy(H.corr_kf, corr_kf, (size_t)n_corr * 4), memcpy(H.lc_start, lc_start, ((size_t)n_corr + 1) * 4);
  memcpy(H.lc_kf, lc_kf, (size_t)n_lc * 4), memcpy(H.cp_id, cp_id, (size_t)n_cp * 4), memcpy(H.cp_ref, cp_ref, (size_t)n_cp * 4);
  VO_CHECK(vo::copy_h2d(s->P.in, s->pg_stage.data(), H.bytes, s->st, W));  // the one copy
  VO_CHECK(pg_enqueue_window(s, curr, match, n_corr, n_lc, n_cp));
  return vo::stream_sync(s->st, W);  // (the staging block is free again)
}

int vo_kfstore_pose_graph_window_dev(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *dev_corr_kf, const double *dev_S_corr,
                                     const double *dev_S_uncorr, const int32_t *dev_lc_start, int n_lc, const int32_t *dev_lc_kf, int n_cp,
                                     const int32_t *dev_cp_id, const int32_t *dev_cp_ref) {
  const char *W = "vo_kfstore_pose_graph_window_dev";
  VO_CHECK(need_pose_graph(s, W));
  if (!dev_lc_start || (n_corr > 0 && (!dev_corr_kf || !dev_S_corr || !dev_S_uncorr)) || (n_lc > 0 && !dev_lc_kf) ||
      (n_cp > 0 && (!dev_cp_id || !dev_cp_ref)))
    return VO_ERR_INVALID;
  VO_CHECK(pg_check_counts(s, W, curr, match, n_corr, n_lc, n_cp));
  const vo::PgInputs I = vo::pg_inputs(s->P.in, n_corr, n_lc, n_cp);
  auto d2d = [&](void *dst, const void *src, size_t bytes) {
    return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->st) == hipSuccess;
  };
  if (!d2d(I.S_corr, dev_S_corr, (size_t)n_corr * 64) || !d2d(I.S_unc, dev_S_uncorr, (size_t)n_corr * 64) ||
      !d2d(I.corr_kf, dev_corr_kf, (size_t)n_corr * 4) || !d2d(I.lc_start, dev_lc_start, ((size_t)n_corr + 1) * 4) ||
      !d2d(I.lc_kf, dev_lc_kf, (size_t)n_lc * 4) || !d2d(I.cp_id, dev_cp_id, (size_t)n_cp * 4) || !d2d(I.cp_ref, dev_cp_ref, (size_t)n_cp * 4)) {
    vo::set_error("%s: hipMemcpyAsync failed", W);
    return VO_ERR_HIP;
  }
  return pg_enqueue_window(s, curr, match, n_corr, n_lc, n_cp);
}

int vo_kfstore_pose_graph_window_result(vo_kfstore *s, int32_t *record, int32_t *node_kf, double *quats, double *trans, double *scales,
                                        int32_t *edge_i, int32_t *edge_j, double *q_meas, double *t_meas, double *s_meas) {
  const char *W = "vo_kfstore_pose_graph_window_result";
  VO_CHECK(need_pose_graph(s, W));
  VO_CHECK(pg_fetch_window(s, W, false));
  const int32_t *r = s->pg_rec;
  if (record) memcpy(record, r, sizeof(s->pg_rec));
  if (r[vo::kPgStatus] != VO_KFSTORE_BA_WINDOW_OK) return VO_OK;
  const size_t nn = (size_t)r[vo::kPgNNodes], ne = (size_t)r[vo::kPgNEdges];
  const vo::KfPgView &P = s->P;
  if (node_kf) memcpy(node_kf, pg_staged(s, P.node_kf), nn * 4);
  if (quats) memcpy(quats, pg_staged(s, P.quats), nn * 32);
  if (trans) memcpy(trans, pg_staged(s, P.trans), nn * 24);
  if (scales) memcpy(scales, pg_staged(s, P.scales), nn * 8);
  if (edge_i) memcpy(edge_i, pg_staged(s, P.e_i), ne * 4);
  if (edge_j) memcpy(edge_j, pg_staged(s, P.e_j), ne * 4);
  if (q_meas) memcpy(q_meas, pg_staged(s, P.q_meas), ne * 32);
  if (t_meas) memcpy(t_meas, pg_staged(s, P.t_meas), ne * 24);
  if (s_meas) memcpy(s_meas, pg_staged(s, P.s_meas), ne * 8);
  return VO_OK;
}

int vo_kfstore_pose_graph_apply(vo_kfstore *s, const double *quats, const double *trans) {
  const char *W = "vo_kfstore_pose_graph_apply";
  VO_CHECK(need_pose_graph(s, W));
  if (!s->pg_window || s->pg_gen != s->gen) {
    vo::set_error("%s: no window, or the store has been changed since the last one", W);
    return VO_ERR_INVALID;
  }
  if (!s->pg_rec_known) VO_CHECK(pg_fetch_window(s, W, true));
  const int32_t *r = s->pg_rec;
  if (r[vo::kPgStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    vo::set_error("%s: the last window is %s", W, r[vo::kPgStatus] == VO_KFSTORE_BA_WINDOW_EMPTY ? "empty" : "overflowed");
    return VO_ERR_INVALID;
  }
  if (!quats || !trans) return VO_ERR_INVALID;
  const size_t nn = (size_t)r[vo::kPgNNodes];
  uint8_t *h = s->pg_stage.data();
  memcpy(h, quats, nn * 32), memcpy(h + nn * 32, trans, nn * 24);  // staged as k_pg_poses reads it: quats | trans
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));  // (rebuilt when stale: the refresh list is read off it)
  VO_CHECK(vo::copy_h2d(s->P.sol, h, nn * 56, s->st, W));
  const vo::PgInputs I = vo::pg_inputs(s->P.in, s->pg_counts[0], s->pg_counts[1], s->pg_counts[2]);
  const vo::KfStoreView V = vo::kfstore_view(s);
  VO_CHECK(vo::pg_apply_enqueue(V, O, s->X, s->M, s->B, s->P, I, (int)nn, s->st));
  VO_CHECK(vo::ba_refresh_list_enqueue(V, O, s->X, s->M, s->B, s->normals.as<double>(), vo::connections_view(s->conn).status,
                                       s->size * s->NK, s->P.rl, s->st));  // updateNormalAndDepth of every live point (:1299)
  s->obs_dirty = true, s->gen++, s->pg_rec_known = false;
  return vo::stream_sync(s->st, W);  // (the staging block is free again)
}

int vo_kfstore_pose_graph(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *corr_kf, const double *S_corr, const double *S_uncorr,
                          const int32_t *lc_start, const int32_t *lc_kf, int n_cp, const int32_t *cp_id, const int32_t *cp_ref,
                          int max_iterations, vo_lm_summary *summary) {
  const char *W = "vo_kfstore_pose_graph";
  VO_CHECK(need_pose_graph(s, W));
  VO_CHECK(vo_kfstore_pose_graph_window(s, curr, match, n_corr, corr_kf, S_corr, S_uncorr, lc_start, lc_kf, n_cp, cp_id, cp_ref));
  VO_CHECK(pg_fetch_window(s, W, false));  // the ONE device-to-host copy
  const int32_t *r = s->pg_rec;
  if (r[vo::kPgStatus] == VO_KFSTORE_BA_WINDOW_OVERFLOW) {
    vo::set_error("%s: %d nodes, %d edges; the solver takes %d nodes and the store was enabled for %d edges", W, r[vo::kPgNNodes],
                  r[vo::kPgNEdges], s->P.max_nodes, s->P.max_edges);
    return VO_ERR_CAPACITY;
  }
  if (r[vo::kPgStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    vo::set_error("%s: the window is empty (curr or match erased, a key-frame without a pose, or lists only the device could refuse)", W);
    return VO_ERR_INVALID;
  }
  const vo::KfPgView &P = s->P;
  const size_t nn = (size_t)r[vo::kPgNNodes];
  memcpy(s->pg_q.data(), pg_staged(s, P.quats), nn * 32), memcpy(s->pg_t.data(), pg_staged(s, P.trans), nn * 24);
  // whatever the solver refuses is returned and nothing is written back (the shim's rule, optimizer_hip.inl:280-287)
  VO_CHECK(vo_pose_graph_solve((int)nn, s->pg_q.data(), s->pg_t.data(), pg_staged(s, P.scales), r[vo::kPgFixed], r[vo::kPgNEdges],
                               pg_staged(s, P.e_i), pg_staged(s, P.e_j), pg_staged(s, P.q_meas), pg_staged(s, P.t_meas),
                               pg_staged(s, P.s_meas), 1, max_iterations, summary));
  return vo_kfstore_pose_graph_apply(s, s->pg_q.data(), s->pg_t.data());
}

int vo_kfstore_update_connections_dev(vo_kfstore *s, int n, const int32_t *dev_keyframes) {
  VO_CHECK(need_connections(s, "vo_kfstore_update_connections_dev"));
  if (n < 0 || (n > 0 && !dev_keyframes)) return VO_ERR_INVALID;
  if (n == 0 || s->size == 0) return VO_OK;
  VO_CHECK(vo::connections_reserve(s->conn, n, nullptr));  // (before the index: nothing is enqueued when it fails)
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  s->gen++;  // (the ordered lists are what a window starts from)
  return vo::connections_update(s->conn, vo::kfstore_view(s), O, n, dev_keyframes, s->st);
}

int vo_kfstore_update_connections(vo_kfstore *s, int n, const int32_t *keyframes) {
  const char *W = "vo_kfstore_update_connections";
  VO_CHECK(need_connections(s, W));
  if (n < 0 || (n > 0 && !keyframes)) return VO_ERR_INVALID;
  for (int i = 0; i < n; i++)
    if (keyframes[i] < 0 || keyframes[i] >= s->size) {
      vo::set_error("%s: entry %d: key-frame %d outside [0, %d)", W, i, keyframes[i], s->size);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  int *dev_list = nullptr;
  VO_CHECK(vo::connections_reserve(s->conn, n, &dev_list));
  VO_CHECK(vo::copy_h2d(dev_list, keyframes, (size_t)n * 4, s->st, W));
  VO_CHECK(vo_kfstore_update_connections_dev(s, n, dev_list));
  return vo::stream_sync(s->st, W);  // (the caller's list is free on return)
}

int vo_kfstore_connections_status(vo_kfstore *s, int32_t *word) {
  VO_CHECK(need_connections(s, "vo_kfstore_connections_status"));
  if (!word) return VO_ERR_INVALID;
  int w = 0;
  VO_CHECK(vo::connections_status(s->conn, s->st, &w));
  *word = w;
  return VO_OK;
}

int vo_kfstore_get_connections(vo_kfstore *s, int keyframe, int32_t *n_connected, int32_t *weights, int32_t *n_ordered,
                               int32_t *ordered, int32_t *ordered_weights, int32_t *parent, int32_t *n_children, int32_t *children) {
  VO_CHECK(need_connections(s, "vo_kfstore_get_connections"));
  if (keyframe < 0 || keyframe >= s->size) return VO_ERR_INVALID;
  return vo::connections_get(s->conn, s->size, keyframe, s->st, n_connected, weights, n_ordered, ordered, ordered_weights, parent,
                             n_children, children);
}

int vo_kfstore_enable_point_upkeep(vo_kfstore *s, int max_recent) {
  const char *W = "vo_kfstore_enable_point_upkeep";
  VO_CHECK(need_local_ba(s, W));
  if (max_recent < 1) return VO_ERR_INVALID;
  if (s->size != 0) {
    vo::set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  if (s->upkeep) return VO_OK;
  VO_CHECK(s->up.reserve(vo::upkeep_bytes(max_recent, s->NK)));
  s->U = vo::upkeep_layout(s->up.p, max_recent, s->NK);
  VO_CHECK(s->up_stage.reserve((size_t)s->U.L * 12));
  VO_CHECK(vo::connections_reserve(s->conn, 1, nullptr));  // process_new_keyframe's update of one key-frame allocates nothing
  VO_CHECK(vo::upkeep_init(s->U, s->st));
  VO_CHECK(vo::stream_sync(s->st, W));
  s->upkeep = true;
  return VO_OK;
}

int vo_kfstore_compute_descriptors_dev(vo_kfstore *s, int n, const int32_t *dev_ids) {
  const char *W = "vo_kfstore_compute_descriptors_dev";
  VO_CHECK(need_upkeep(s, W));
  if (n < 0 || (n > 0 && !dev_ids)) return VO_ERR_INVALID;
  if (n > s->U.L) {
    vo::set_error("%s: %d ids, the store takes %d (max_recent + max_features)", W, n, s->U.L);
    return VO_ERR_CAPACITY;
  }
  if (n == 0) return VO_OK;
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  s->gen++;  // (flags and ids stay: the index does not go stale)
  return vo::upkeep_descriptors_enqueue(vo::kfstore_view(s), O, s->U, vo::connections_view(s->conn).status, n, dev_ids, s->st);
}

int vo_kfstore_compute_descriptors(vo_kfstore *s, int n, const int32_t *ids) {
  const char *W = "vo_kfstore_compute_descriptors";
  VO_CHECK(need_upkeep(s, W));
  if (n < 0 || (n > 0 && !ids)) return VO_ERR_INVALID;
  if (n > s->U.L) {
    vo::set_error("%s: %d ids, the store takes %d (max_recent + max_features)", W, n, s->U.L);
    return VO_ERR_CAPACITY;
  }
  for (int i = 0; i < n; i++)
    if (ids[i] < 0) {
      vo::set_error("%s: entry %d: id %d is negative", W, i, ids[i]);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  memcpy(s->up_stage.data(), ids, (size_t)n * 4);
  VO_CHECK(vo::copy_h2d(s->U.list, s->up_stage.data(), (size_t)n * 4, s->st, W));
  VO_CHECK(vo_kfstore_compute_descriptors_dev(s, n, s->U.list));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_process_new_keyframe(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_process_new_keyframe";
  VO_CHECK(need_upkeep(s, W));
  VO_CHECK(need_keyframe(s, W, current));
  // (that `current` has been erased only the device knows: nothing is then listed, and the sticky INVALID is raised)
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  const vo::KfStoreView V = vo::kfstore_view(s);
  VO_CHECK(vo::upkeep_process_enqueue(V, O, s->X, s->M, s->B, s->U, s->normals.as<double>(), vo::connections_view(s->conn).status, current,
                                      s->st));
  s->gen++;  // (flags and ids stay: the index does not go stale)
  return vo::connections_update(s->conn, V, O, 1, s->U.head + 2, s->st);  // keyframe_curr_->updateConnections() (:128)
}

int vo_kfstore_add_point_stats_dev(vo_kfstore *s, int n, const int32_t *dev_ids, const int32_t *dev_visible, const int32_t *dev_found) {
  const char *W = "vo_kfstore_add_point_stats_dev";
  VO_CHECK(need_upkeep(s, W));
  if (n < 0 || (n > 0 && (!dev_ids || !dev_visible || !dev_found))) return VO_ERR_INVALID;
  s->gen++;
  return vo::upkeep_stats_enqueue(s->U, n, dev_ids, dev_visible, dev_found, s->st);
}

int vo_kfstore_add_point_stats(vo_kfstore *s, int n, const int32_t *ids, const int32_t *visible, const int32_t *found) {
  const char *W = "vo_kfstore_add_point_stats";
  VO_CHECK(need_upkeep(s, W));
  if (n < 0 || (n > 0 && (!ids || !visible || !found))) return VO_ERR_INVALID;
  if (n > s->U.L) {
    vo::set_error("%s: %d ids, the store takes %d (max_recent + max_features)", W, n, s->U.L);
    return VO_ERR_CAPACITY;
  }
  for (int i = 0; i < n; i++)
    if (visible[i] < 0 || found[i] < 0) {
      vo::set_error("%s: entry %d: a negative increment (%d visible, %d found)", W, i, visible[i], found[i]);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  // staged as the block's list holds them: ids | visible | found, L entries each; one copy
  const size_t L = (size_t)s->U.L;
  int32_t *h = reinterpret_cast<int32_t *>(s->up_stage.data());
  memset(h, 0xff, L * 4), memset(h + L, 0, L * 8);  // (beyond n: no id, no increment)
  memcpy(h, ids, (size_t)n * 4), memcpy(h + L, visible, (size_t)n * 4), memcpy(h + 2 * L, found, (size_t)n * 4);
  VO_CHECK(vo::copy_h2d(s->U.list, h, L * 12, s->st, W));
  VO_CHECK(vo_kfstore_add_point_stats_dev(s, n, s->U.list, s->U.list + L, s->U.list + 2 * L));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_cull_map_points(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_cull_map_points";
  VO_CHECK(need_upkeep(s, W));
  VO_CHECK(need_keyframe(s, W, current));
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  VO_CHECK(vo::upkeep_cull_enqueue(vo::kfstore_view(s), O, s->X, s->U, current, s->st));
  s->obs_dirty = true, s->gen++;  // (whether anything was erased only the device knows)
  return VO_OK;
}

int vo_kfstore_recent_points(vo_kfstore *s, int32_t *n, int32_t *ids, int32_t *first_kf, int32_t *found, int32_t *visible) {
  const char *W = "vo_kfstore_recent_points";
  VO_CHECK(need_upkeep(s, W));
  const size_t R = (size_t)s->U.R;
  std::vector<int32_t> h(4 * R + 4);
  VO_CHECK(vo::copy_d2h(h.data(), s->U.head, 16, s->st, W));
  const int32_t *cols[4] = {s->U.id, s->U.first_kf, s->U.found, s->U.visible};
  for (int c = 0; c < 4; c++) VO_CHECK(vo::copy_d2h(h.data() + 4 + c * R, cols[c], R * 4, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  const int cnt = std::min(std::max(h[0], 0), s->U.R);
  std::vector<int> order((size_t)cnt);
  for (int i = 0; i < cnt; i++) order[(size_t)i] = i;
  const int32_t *id = h.data() + 4;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return id[a] < id[b]; });  // (an id has one entry)
  int32_t *out[4] = {ids, first_kf, found, visible};
  for (int c = 0; c < 4; c++)
    if (out[c])
      for (int i = 0; i < cnt; i++) out[c][i] = h[4 + c * R + (size_t)order[(size_t)i]];
  if (n) *n = cnt;
  return VO_OK;
}

int vo_kfstore_upkeep_result(vo_kfstore *s, int32_t *record, int32_t *erased_ids) {
  const char *W = "vo_kfstore_upkeep_result";
  VO_CHECK(need_upkeep(s, W));
  int32_t rec[vo::kUpRecInts];
  std::vector<int32_t> er((size_t)s->U.R);
  VO_CHECK(vo::copy_d2h(rec, s->U.rec, sizeof(rec), s->st, W));
  if (erased_ids) VO_CHECK(vo::copy_d2h(er.data(), s->U.erased, er.size() * 4, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  if (record) memcpy(record, rec, sizeof(rec));
  if (erased_ids) {
    const int ne = rec[vo::kUpKind] == VO_KFSTORE_UPKEEP_CULL ? std::min(std::max(rec[vo::kUpNErased], 0), s->U.R) : 0;
    std::sort(er.begin(), er.begin() + ne);
    memcpy(erased_ids, er.data(), (size_t)ne * 4);
  }
  return VO_OK;
}

int vo_kfstore_enable_fuse(vo_kfstore *s, const float bounds[4], int max_candidates) {
  const char *W = "vo_kfstore_enable_fuse";
  VO_CHECK(need_upkeep(s, W));
  if (!bounds || max_candidates < 1 || !(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2])) return VO_ERR_INVALID;
  if (s->size != 0) {
    vo::set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  if (s->NK > 4096) {
    vo::set_error("%s: %d features per key-frame, the search stages at most 4096", W, s->NK);
    return VO_ERR_CAPACITY;
  }
  if (s->fuse) return VO_OK;
  const size_t bytes = vo::fuse_bytes(s->NK, max_candidates, s->okeys_cap);
  VO_CHECK(s->fu.reserve(bytes));
  s->F = vo::fuse_layout(s->fu.p, s->NK, max_candidates, s->okeys_cap, bounds);
  VO_CHECK(s->up_stage.reserve((size_t)s->F.list_cap * 4));
  VO_HIP_CHECK(hipMemsetAsync(s->fu.p, 0, bytes, s->st));
  VO_HIP_CHECK(hipMemsetAsync(s->F.targets, 0xff, 64 * 4, s->st));  // (no call yet: no step)
  VO_CHECK(vo::stream_sync(s->st, W));
  s->fuse = true;
  return VO_OK;
}

static vo::FuseArgs fuse_args(vo_kfstore *s, const vo::KfObsView &O) {
  const vo::KfConnView C = vo::connections_view(s->conn);
  return vo::FuseArgs{vo::kfstore_view(s), O, C, s->X, s->M, s->B, s->U, s->F, s->normals.as<double>(), C.status};
}

int vo_kfstore_fuse_map_points_dev(vo_kfstore *s, int target, int n, const int32_t *dev_ids, float threshold) {
  const char *W = "vo_kfstore_fuse_map_points_dev";
  VO_CHECK(need_fuse(s, W));
  VO_CHECK(need_keyframe(s, W, target));
  if (n < 0 || (n > 0 && !dev_ids) || !(threshold > 0.f)) return VO_ERR_INVALID;
  if (n > s->F.list_cap) {
    vo::set_error("%s: %d ids, the store takes %d (60 * max_features)", W, n, s->F.list_cap);
    return VO_ERR_CAPACITY;
  }
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  VO_CHECK(vo::fuse_single_enqueue(fuse_args(s, O), target, n, dev_ids, threshold, s->st));
  s->obs_dirty = true, s->gen++;  // (whether anything matched only the device knows)
  return VO_OK;
}

int vo_kfstore_fuse_map_points(vo_kfstore *s, int target, int n, const int32_t *ids, float threshold) {
  const char *W = "vo_kfstore_fuse_map_points";
  VO_CHECK(need_fuse(s, W));
  VO_CHECK(need_keyframe(s, W, target));
  if (n < 0 || (n > 0 && !ids) || !(threshold > 0.f)) return VO_ERR_INVALID;
  if (n > s->F.list_cap) {
    vo::set_error("%s: %d ids, the store takes %d (60 * max_features)", W, n, s->F.list_cap);
    return VO_ERR_CAPACITY;
  }
  if (n > 0) {
    memcpy(s->up_stage.data(), ids, (size_t)n * 4);
    VO_CHECK(vo::copy_h2d(s->F.list, s->up_stage.data(), (size_t)n * 4, s->st, W));
  }
  VO_CHECK(vo_kfstore_fuse_map_points_dev(s, target, n, s->F.list, threshold));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_search_in_neighbors(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_search_in_neighbors";
  VO_CHECK(need_fuse(s, W));
  VO_CHECK(need_keyframe(s, W, current));
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));  // the index the overlay stands on
  VO_CHECK(vo::fuse_neighbors_enqueue(fuse_args(s, O), current, s->st));
  s->obs_dirty = true, s->gen++;
  VO_CHECK(vo::kfstore_obs_view(s, &O));  // the one rebuild behind the fuses, whatever their number
  const vo::FuseArgs A = fuse_args(s, O);
  VO_CHECK(vo::fuse_live_list_enqueue(A, current, s->st));
  VO_CHECK(vo::upkeep_descriptors_enqueue(A.S, O, s->U, A.status, s->NK, s->F.snap, s->st));             // computeDescriptor (:426)
  VO_CHECK(vo::ba_refresh_list_enqueue(A.S, O, s->X, s->M, s->B, A.normals, A.status, s->NK, s->F.snap, s->st));  // (:427)
  return vo::connections_update(s->conn, A.S, O, 1, s->F.head + 2, s->st);  // keyframe_curr_->updateConnections() (:431)
}

int vo_kfstore_fuse_result(vo_kfstore *s, int32_t *record, int32_t *targets, int32_t *per_target) {
  const char *W = "vo_kfstore_fuse_result";
  VO_CHECK(need_fuse(s, W));
  int32_t head[4], tg[64], rec[64 * vo::kFuseRecInts];
  VO_CHECK(vo::copy_d2h(head, s->F.head, sizeof(head), s->st, W));
  VO_CHECK(vo::copy_d2h(tg, s->F.targets, sizeof(tg), s->st, W));
  VO_CHECK(vo::copy_d2h(rec, s->F.rec, sizeof(rec), s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  int32_t out_rec[8] = {0}, out_t[VO_KFSTORE_FUSE_MAX_STEPS], out_p[VO_KFSTORE_FUSE_MAX_STEPS * 6];
  memset(out_t, 0xff, sizeof(out_t)), memset(out_p, 0, sizeof(out_p));
  const int n_t = std::min(std::max(head[0], 0), vo::kFuseFinal);
  int n = 0;
  for (int step = 0; step <= vo::kFuseFinal; step++) {
    if (step < vo::kFuseFinal ? step >= n_t : tg[step] < 0) continue;
    out_t[n] = tg[step];
    for (int c = 0; c < 6; c++) out_p[n * 6 + c] = rec[step * vo::kFuseRecInts + 1 + c], out_rec[1 + c] += out_p[n * 6 + c];
    n++;
  }
  out_rec[0] = n;
  if (record) memcpy(record, out_rec, sizeof(out_rec));
  if (targets) memcpy(targets, out_t, sizeof(out_t));
  if (per_target) memcpy(per_target, out_p, sizeof(out_p));
  return VO_OK;
}

int vo_kfstore_enable_loop(vo_kfstore *s, int max_candidates, int max_loop_points, int max_rand) {
  const char *W = "vo_kfstore_enable_loop";
  VO_CHECK(need_fuse(s, W));
  if (max_candidates < 1 || max_candidates > VO_KFSTORE_LOOP_MAX_CANDIDATES || max_loop_points < 1 || max_rand < 3) return VO_ERR_INVALID;
  if (s->size != 0) {
    vo::set_error("%s: the store holds %d key-frames, the call is valid on an empty store only", W, s->size);
    return VO_ERR_INVALID;
  }
  if (s->loop) return VO_OK;
  const size_t bytes = vo::loop_bytes(s->NK, max_candidates, max_loop_points, max_rand, s->okeys_cap);
  VO_CHECK(s->lp.reserve(bytes));
  s->L = vo::loop_layout(s->lp.p, s->NK, max_candidates, max_loop_points, max_rand, s->okeys_cap);
  const size_t down = (size_t)(vo::kLoopStateInts + VO_KFSTORE_LOOP_MAX_CANDIDATES * vo::kLoopPerInts + s->NK + max_loop_points) * 4 + 26 * 8;
  VO_CHECK(s->lp_stage.reserve(std::max(((size_t)VO_KFSTORE_LOOP_MAX_CANDIDATES + (size_t)max_rand) * 4, down)));
  VO_CHECK(vo::loop_init(s->L, s->M, bytes, s->st));  // (synchronises: its tables are host temporaries)
  s->loop = true;
  return VO_OK;
}

static vo::LoopArgs loop_args(vo_kfstore *s, const vo::KfObsView &O) {
  const vo::KfConnView C = vo::connections_view(s->conn);
  return vo::LoopArgs{vo::kfstore_view(s), O, C, s->X, s->M, s->F, s->L, C.status};
}

// the candidates and the rand() values are in the block already (L.cand, L.rand)
static int loop_compute_enqueue(vo_kfstore *s, int current, int n_cand, int fix_scale, int n_rand, int32_t rand_max, int max_rounds) {
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));  // "who observes p in key-frame j" (launches only, and only when the index is stale)
  const vo::LoopArgs A = loop_args(s, O);
  VO_CHECK(vo::loop_begin_enqueue(A, current, n_cand, fix_scale ? 1 : 0, n_rand, rand_max, s->st));
  s->loop_fix_scale = fix_scale ? 1 : 0, s->loop_called = true;
  return vo::loop_rounds_enqueue(A, max_rounds, s->loop_fix_scale, s->st);
}

static int loop_check(vo_kfstore *s, const char *W, int n_cand, const void *cand, int n_rand, const void *rand_values, int32_t rand_max,
                      int max_rounds) {
  VO_CHECK(need_loop(s, W));
  if (n_cand < 1 || !cand || n_rand < 0 || (n_rand > 0 && !rand_values) || rand_max < 1 || max_rounds < 0) return VO_ERR_INVALID;
  if (n_cand > s->L.C || n_rand > s->L.max_rand) {
    vo::set_error("%s: %d candidates / %d rand() values, the block was enabled for %d / %d", W, n_cand, n_rand, s->L.C, s->L.max_rand);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

int vo_kfstore_compute_sim3_dev(vo_kfstore *s, int current, int n_cand, const int32_t *dev_cand, int fix_scale, int n_rand,
                                const int32_t *dev_rand_values, int32_t rand_max, int max_rounds) {
  const char *W = "vo_kfstore_compute_sim3_dev";
  VO_CHECK(loop_check(s, W, n_cand, dev_cand, n_rand, dev_rand_values, rand_max, max_rounds));
  VO_HIP_CHECK(hipMemcpyAsync(s->L.cand, dev_cand, (size_t)n_cand * 4, hipMemcpyDeviceToDevice, s->st));
  if (n_rand > 0) VO_HIP_CHECK(hipMemcpyAsync(s->L.rand, dev_rand_values, (size_t)n_rand * 4, hipMemcpyDeviceToDevice, s->st));
  return loop_compute_enqueue(s, current, n_cand, fix_scale, n_rand, rand_max, max_rounds);
}

int vo_kfstore_compute_sim3(vo_kfstore *s, int current, int n_cand, const int32_t *cand, int fix_scale, int n_rand,
                            const int32_t *rand_values, int32_t rand_max, int max_rounds) {
  const char *W = "vo_kfstore_compute_sim3";
  VO_CHECK(loop_check(s, W, n_cand, cand, n_rand, rand_values, rand_max, max_rounds));
  VO_CHECK(need_keyframe(s, W, current));
  for (int i = 0; i < n_cand; i++) VO_CHECK(need_keyframe(s, W, cand[i]));
  // one copy: [16 candidates | rand() values] lands on L.cand .. L.rand, which the block keeps side by side
  int32_t *up = reinterpret_cast<int32_t *>(s->lp_stage.data());
  memset(up, 0xff, VO_KFSTORE_LOOP_MAX_CANDIDATES * 4);
  memcpy(up, cand, (size_t)n_cand * 4);
  if (n_rand > 0) memcpy(up + VO_KFSTORE_LOOP_MAX_CANDIDATES, rand_values, (size_t)n_rand * 4);
  VO_CHECK(vo::copy_h2d(s->L.cand, up, ((size_t)VO_KFSTORE_LOOP_MAX_CANDIDATES + (size_t)n_rand) * 4, s->st, W));
  VO_CHECK(loop_compute_enqueue(s, current, n_cand, fix_scale, n_rand, rand_max, max_rounds));
  return vo::stream_sync(s->st, W);
}

int vo_kfstore_compute_sim3_continue(vo_kfstore *s, int max_rounds) {
  const char *W = "vo_kfstore_compute_sim3_continue";
  VO_CHECK(need_loop(s, W));
  if (max_rounds < 0) return VO_ERR_INVALID;
  if (!s->loop_called) {
    vo::set_error("%s: no vo_kfstore_compute_sim3 has been enqueued on this store", W);
    return VO_ERR_INVALID;
  }
  vo::KfObsView O;
  VO_CHECK(vo::kfstore_obs_view(s, &O));
  return vo::loop_rounds_enqueue(loop_args(s, O), max_rounds, s->loop_fix_scale, s->st);
}

int vo_kfstore_loop_result(vo_kfstore *s, int32_t *record, int32_t *per_cand, double *Scm, double *Scw, int32_t *match_ids,
                           int32_t *n_loop_points, int32_t *loop_point_ids) {
  const char *W = "vo_kfstore_loop_result";
  VO_CHECK(need_loop(s, W));
  const vo::KfLoopView &L = s->L;
  int32_t st[vo::kLoopStateInts], per[VO_KFSTORE_LOOP_MAX_CANDIDATES * vo::kLoopPerInts];
  double sims[26];
  VO_CHECK(vo::copy_d2h(st, L.st, sizeof(st), s->st, W));
  VO_CHECK(vo::copy_d2h(per, L.per, sizeof(per), s->st, W));
  VO_CHECK(vo::copy_d2h(sims, L.Scm, 13 * 8, s->st, W));
  VO_CHECK(vo::copy_d2h(sims + 13, L.Scw, 13 * 8, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  const int n_cur = std::min(std::max(st[vo::kLsNCur], 0), s->NK), n_lp = st[vo::kLsState] >= 2 ? std::min(std::max(st[vo::kLsNLoop], 0), L.P) : 0;
  if (match_ids && n_cur > 0) VO_CHECK(vo::copy_d2h(match_ids, L.match_ids, (size_t)n_cur * 4, s->st, W));
  if (loop_point_ids && n_lp > 0) VO_CHECK(vo::copy_d2h(loop_point_ids, L.loop_ids, (size_t)n_lp * 4, s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  if (record) {
    memset(record, 0, 16 * 4);
    memcpy(record, st, 9 * 4);
  }
  if (per_cand) memcpy(per_cand, per, (size_t)L.C * vo::kLoopPerInts * 4);
  if (Scm) memcpy(Scm, sims, 13 * 8);
  if (Scw) memcpy(Scw, sims + 13, 13 * 8);
  if (n_loop_points) *n_loop_points = n_lp;
  return VO_OK;
}

int vo_kfstore_loop_solver_inputs(vo_kfstore *s, int position, int32_t *n, double *cam1_points, double *cam2_points, double *pixels1,
                                  double *pixels2, int32_t *max_err1, int32_t *max_err2, int32_t *matched_index) {
  const char *W = "vo_kfstore_loop_solver_inputs";
  VO_CHECK(need_loop(s, W));
  const vo::KfLoopView &L = s->L;
  if (position < 0 || position >= L.C || !n) return VO_ERR_INVALID;
  int32_t per[vo::kLoopPerInts];
  VO_CHECK(vo::copy_d2h(per, L.per + position * vo::kLoopPerInts, sizeof(per), s->st, W));
  VO_CHECK(vo::stream_sync(s->st, W));
  const size_t N = (size_t)std::min(std::max(per[vo::kLpN], 0), s->NK), o = (size_t)position * s->NK;
  *n = (int32_t)N;
  if (N == 0) return VO_OK;
  if (cam1_points) VO_CHECK(vo::copy_d2h(cam1_points, L.pc1 + o * 3, N * 24, s->st, W));
  if (cam2_points) VO_CHECK(vo::copy_d2h(cam2_points, L.pc2 + o * 3, N * 24, s->st, W));
  if (pixels1) VO_CHECK(vo::copy_d2h(pixels1, L.px1 + o * 2, N * 16, s->st, W));
  if (pixels2) VO_CHECK(vo::copy_d2h(pixels2, L.px2 + o * 2, N * 16, s->st, W));
  if (max_err1) VO_CHECK(vo::copy_d2h(max_err1, L.me1 + o, N * 4, s->st, W));
  if (max_err2) VO_CHECK(vo::copy_d2h(max_err2, L.me2 + o, N * 4, s->st, W));
  if (matched_index) VO_CHECK(vo::copy_d2h(matched_index, L.midx + o, N * 4, s->st, W));
  return vo::stream_sync(s->st, W);
}

}  // extern "C"
