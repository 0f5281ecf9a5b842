// cull.hip -- redundant key-frames culled on the device: LocalMapping::cullingKeyFrames
// (localMapping.cpp:434-494) with KeyFrame::eraseKeyFrame, eraseConnection (keyframe.cpp:400-526) and
// MapPoint::eraseObservedKF (mappoint.cpp:333-381), over the key-frame store's observation index and connection state.
//   k_cull_count  a workgroup per candidate of the current key-frame's ordered list, a thread per feature: the feature's
//                 gates, then its id's run of the index for obs(id) and the observers at a close enough octave.  It counts
//                 against the state the call starts with: SPECULATIVE, exact until something is erased.
//   k_cull_apply  ONE workgroup walks the candidates in order.  Until the first erase of the call it takes the counted pair
//                 as it is; from then on it counts every later candidate again, with the same device function, against the
//                 state the erases left.  An erase runs inside it: threads parallel over the other key-frame (weights),
//                 over the erased key-frame's features (observations) and over its children (a re-parenting round).
//   (the caller follows with connections.hip's ordering pass over the touched key-frames)
// As in connections.hip nothing depends on which thread runs when: the counts are integer sums, a step of the sequence
// writes every word or byte from one thread, and the re-parenting choice is the maximum of distinct keys.
#include "kfstore.h"

#include "obs_walk.h"

#include <algorithm>

namespace {

using namespace vo;

constexpr int kMaxKf = VO_KFSTORE_CONNECTIONS_MAX_KEYFRAMES;
constexpr int kThreshold = 15;  // the threshold of a key-frame's own list (keyframe.cpp:100; connections.hip)
constexpr int kMinObs = 3;      // `int min_obs = 3` (localMapping.cpp:436)
constexpr int kSeqThreads = 1024;
constexpr int kPer = kMaxKf / kSeqThreads;  // key-frames per thread of the sequential kernels
enum { kKept = 0, kErased = 1, kPending = 2, kSkipped = 3 };

// The sequential kernels are ONE workgroup: what a step writes and a later step reads stays inside it, so the accesses and
// the fence are workgroup-scope (connections.hip's discipline; no device-scope fence inside the sequence).
__device__ __forceinline__ int load_wg(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void store_wg(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint8_t load_wg(const uint8_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void store_wg(uint8_t *p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void end_step() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __syncthreads();
}

// the store's records are the kernels' to write where the erase says so: the bad word and the flags bytes
__device__ __forceinline__ int *bad_word(const KfStoreView &S, int k) { return const_cast<int *>(kf_head(S, k)) + 1; }
__device__ __forceinline__ uint8_t *flag_byte(const KfStoreView &S, unsigned entry) {
  const unsigned k = entry / (unsigned)S.NK;
  return const_cast<uint8_t *>(kf_sec<uint8_t>(S, (int)k, S.o_flags)) + (entry - k * (unsigned)S.NK);
}
__device__ __forceinline__ int n_features(const KfStoreView &S, int k) { return min(max(kf_head(S, k)[0], 0), S.NK); }

// the workgroup's sums of a and b in every thread; s: 2 * N ints.  Barriers in front and behind.
template <int N>
__device__ __forceinline__ void block_sum2(int &a, int &b, int *s) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = a, s[N + tid] = b;
  __syncthreads();
  for (int w = N / 2; w > 0; w >>= 1) {
    if (tid < w) s[tid] += s[tid + w], s[N + tid] += s[N + tid + w];
    __syncthreads();
  }
  a = s[0], b = s[N];
}
template <int N>
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long *s) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int w = N / 2; w > 0; w >>= 1) {
    if (tid < w) s[tid] = s[tid + w] > s[tid] ? s[tid + w] : s[tid];
    __syncthreads();
  }
  return s[0];
}

// Feature i of candidate k (localMapping.cpp:449-485): mp_cnt and re_obs grow by what it contributes.  kSeq: inside the
// sequence -- a key of the index is live iff its key-frame is not erased and its flags byte still has bit 0, and the words an
// erase writes are read at workgroup scope; otherwise every key of the index is live (it was built from this state).
template <bool kSeq>
__device__ __forceinline__ void cull_feature(const KfStoreView &S, const KfObsView &O, const KfCullView &X, int k, int i, float th_depth,
                                             int &mp_cnt, int &re_obs) {
  const uint8_t *fl = kf_sec<uint8_t>(S, k, S.o_flags) + i;
  if (!((kSeq ? load_wg(fl) : *fl) & 1)) return;  // `if (!mp || mp->isBad())`
  const int id = kf_sec<int>(S, k, S.o_ids)[i];
  if (id < 0) return;
  const float d = cull_depth(X, k)[i];
  if (d < 0.f || d > th_depth) return;  // (:455)
  mp_cnt++;
  const int level1 = cull_octave(X, k)[i] + 1;
  int obs = 0, seen = 0;  // getObsCnt() (mappoint.cpp:60-63) and obskf (:463-480), both from one walk
  obs_run_holders(
      O, S.NK, S.size, O.run[(size_t)k * S.NK + i], id,
      [&](int kk, unsigned e) { return !kSeq || (!load_wg(X.erased + kk) && (load_wg(flag_byte(S, e)) & 1)); },
      [&](int kk, int f) {
        obs += cull_uright(X, kk)[f] >= 0.f ? 2 : 1;
        const int bad = kSeq ? load_wg(bad_word(S, kk)) : kf_head(S, kk)[1];
        if (kk != k && !bad && cull_octave(X, kk)[f] <= level1) seen++;
        return !(obs > kMinObs && seen >= kMinObs);  // (both only grow: the answer is known)
      });
  if (obs > kMinObs && seen >= kMinObs) re_obs++;
}

template <bool kSeq, int N>
__device__ __forceinline__ void cull_candidate(const KfStoreView &S, const KfObsView &O, const KfCullView &X, int k, float th_depth,
                                               int &mp_cnt, int &re_obs, int *s) {
  mp_cnt = re_obs = 0;
  const int n = n_features(S, k);
  for (int i = threadIdx.x; i < n; i += N) cull_feature<kSeq>(S, O, X, k, i, th_depth, mp_cnt, re_obs);
  block_sum2<N>(mp_cnt, re_obs, s);
}

// (an erased current key-frame has no list: the call walks nothing)
__device__ __forceinline__ int n_candidates(const KfConnView &C, const KfCullView &X, int current, int size) {
  return X.erased[current] ? 0 : min(max(C.n_ordered[current], 0), size);
}

__global__ __launch_bounds__(256) void k_cull_count(KfStoreView S, KfObsView O, KfConnView C, KfCullView X, int current, float th_depth) {
  __shared__ int s[512];
  const int t = blockIdx.x;
  const int n = n_candidates(C, X, current, S.size);
  if (t == 0 && threadIdx.x == 0) {
    X.n_rec[0] = n;
    if (X.erased[current]) atomicOr(C.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  }
  if (t >= n) return;  // (uniform over the workgroup, like every return below)
  const int k = C.ordered[(size_t)current * C.max_kf + t];
  if (k <= 0 || k >= S.size || kf_head(S, k)[1] || X.erased[k]) {  // `if (kf->isBad() || kf->id_ == 0) continue;` (:445)
    if (threadIdx.x == 0) X.rec[t] = make_int4(k, 0, 0, kSkipped);
    return;
  }
  int mp_cnt, re_obs;
  cull_candidate<false, 256>(S, O, X, k, th_depth, mp_cnt, re_obs, s);
  if (threadIdx.x == 0) X.rec[t] = make_int4(k, mp_cnt, re_obs, kKept);
}

// (weight, child, candidate) so that the largest key is the reference's choice (keyframe.cpp:440-467): the strictly largest
// weight, the first child in ascending number, the first candidate in the child's list order -- equal weights stand in
// descending number there
__device__ __forceinline__ unsigned long long parent_key(int w, int c, int x) {
  return ((unsigned long long)(unsigned)w << 32) | ((unsigned long long)(unsigned)(0xffff - c) << 16) | (unsigned)x;
}

// KeyFrame::eraseKeyFrame (keyframe.cpp:400-491) for key-frame k != 0, not erased, not locked.  Every thread of the ONE
// workgroup calls it; it ends with a finished step.  s64: kSeqThreads words.
__device__ void erase_keyframe(const KfStoreView &S, const KfObsView &O, const KfConnView &C, const KfCullView &X, int k,
                               unsigned long long *s64) {
  const int tid = threadIdx.x, size = S.size, NK = S.NK;
  const size_t ld = (size_t)C.max_kf;
  // (:415-416) eraseConnection(k) on every key-frame of k's OWN map; (:426) k's map is cleared.  A key-frame that keeps a
  // weight for k without k keeping one for it is not visited (quirk Q-E1).
  for (int j = tid; j < size; j += kSeqThreads) {
    int *wkj = C.W + (size_t)k * ld + j;
    if (load_wg(wkj) == 0) continue;
    int *wjk = C.W + (size_t)j * ld + k;
    if (load_wg(wjk) != 0) store_wg(wjk, 0), store_wg(C.mode + j, 1), store_wg(C.touched + j, 1);  // updateBestCovisibles: the whole map
    store_wg(wkj, 0);
  }
  // (:418-420) eraseObservedKF(k) on every map point of k.  The thread of k's observation of the id (its lowest-numbered
  // entry) does the id's work; threads of other ids touch other bytes.
  const int n = n_features(S, k);
  const uint8_t *flags = kf_sec<uint8_t>(S, k, S.o_flags);
  const int *ids = kf_sec<int>(S, k, S.o_ids);
  for (int i = tid; i < n; i += kSeqThreads) {
    if (!(load_wg(flags + i) & 1)) continue;
    const int id = ids[i];
    if (id < 0) continue;
    const unsigned mine = (unsigned)k * (unsigned)NK + (unsigned)i;
    const int start = O.run[mine];
    bool owner = false;
    int left = 0;  // observe_cnt_ once k is gone
    obs_run_holders(
        O, NK, size, start, id,
        [&](int kk, unsigned e) { return kk == k || (!load_wg(X.erased + kk) && (load_wg(flag_byte(S, e)) & 1)); },
        [&](int kk, int f) {
          if (kk == k) return owner = (unsigned)f == (unsigned)i;  // (another feature of k observes: nothing to do here)
          left += cull_uright(X, kk)[f] >= 0.f ? 2 : 1;
          return true;
        });
    if (!owner || left > 2) continue;
    // eraseMapPoint (mappoint.cpp:362-381): bit 0 means "exists and is not bad", so it goes in every feature that carries
    // the id, k's own included
    obs_run_each(O, start, id, [&](unsigned e) {
      const int kk = (int)(e / (unsigned)NK);
      if (kk < size && (kk == k || !load_wg(X.erased + kk))) {
        uint8_t *b = flag_byte(S, e);
        const uint8_t v = load_wg(b);
        if (v & 1) store_wg(b, (uint8_t)(v & ~1));
      }
      return true;
    });
  }
  end_step();
  // (:429-483) the children look for a new parent among {parent} and the children already placed
  const int parent = load_wg(C.parent + k);
  bool child[kPer], active[kPer];
  int lo[kPer], only[kPer];  // x is in the child's ordered list iff W >= lo, or (only >= 0) x == only
  unsigned long long best[kPer];
  for (int r = 0; r < kPer; r++) {
    const int j = tid + r * kSeqThreads;
    child[r] = j < size && j != k && load_wg(C.parent + j) == k && !load_wg(X.erased + j);
    active[r] = child[r] && !load_wg(bad_word(S, j));  // `if (kf->isBad()) continue;` (:443)
    lo[r] = 1, only[r] = -1, best[r] = 0;
    if (active[r] && load_wg(C.mode + j) == 0) {  // the thresholded list, or the single first strictly largest weight
      const int *row = C.W + (size_t)j * ld;
      int nt = 0, wmax = 0, kfmax = -1;
      for (int x = 0; x < size; x++) {
        const int w = load_wg(row + x);
        if (w >= kThreshold) nt++;
        if (w > wmax) wmax = w, kfmax = x;
      }
      if (nt > 0) lo[r] = kThreshold;
      else lo[r] = 0x7fffffff, only[r] = kfmax;
    }
  }
  int placed = parent;  // the candidate that joined last (-1: none; a key-frame without a parent starts from the empty set)
  for (;;) {
    unsigned long long mine = 0;
    for (int r = 0; r < kPer; r++) {
      const int j = tid + r * kSeqThreads;
      if (!active[r]) continue;
      if (placed >= 0) {
        const int w = load_wg(C.W + (size_t)j * ld + placed);
        if (w > 0 && (w >= lo[r] || placed == only[r])) best[r] = max(best[r], parent_key(w, j, placed));
      }
      mine = max(mine, best[r]);
    }
    const unsigned long long win = block_max<kSeqThreads>(mine, s64);
    if (win == 0) break;  // `else break;` (:475)
    const int c = 0xffff - (int)((win >> 16) & 0xffffu), x = (int)(win & 0xffffu);
    if (tid == (c & (kSeqThreads - 1))) {
      store_wg(C.parent + c, x), store_wg(C.touched + c, 1), store_wg(C.touched + x, 1);
      for (int r = 0; r < kPer; r++)
        if (r == c / kSeqThreads) child[r] = active[r] = false;
    }
    placed = c;
  }
  bool any = false;
  for (int r = 0; r < kPer; r++) {
    const int j = tid + r * kSeqThreads;
    if (!child[r]) continue;  // (:479-483) the rest, bad ones included, go to k's parent
    store_wg(C.parent + j, parent), store_wg(C.touched + j, 1);
    any = true;
  }
  if ((any || tid == 0) && parent >= 0) store_wg(C.touched + parent, 1);  // (:485) and k leaves its parent's children
  if (tid == 0) {
    store_wg(C.mode + k, 1), store_wg(C.touched + k, 1);
    store_wg(X.erased + k, 1), store_wg(bad_word(S, k), 1);  // (:487; parent[k] stays: the caller's Tcp_)
  }
  end_step();
}

__global__ __launch_bounds__(kSeqThreads) void k_cull_apply(KfStoreView S, KfObsView O, KfConnView C, KfCullView X, int current,
                                                           float th_depth) {
  __shared__ unsigned long long s64[kSeqThreads];
  int *s = reinterpret_cast<int *>(s64);
  const int n = n_candidates(C, X, current, S.size);
  const int *cand = C.ordered + (size_t)current * C.max_kf;  // (rewritten by the ordering pass only: the snapshot of :439)
  bool recount = false;
  for (int t = 0; t < n; t++) {
    const int k = cand[t];
    if (k <= 0 || k >= S.size || load_wg(bad_word(S, k)) || load_wg(X.erased + k)) {
      if (threadIdx.x == 0) X.rec[t] = make_int4(k, 0, 0, kSkipped);
      continue;
    }
    int mp_cnt, re_obs;
    if (recount) cull_candidate<true, kSeqThreads>(S, O, X, k, th_depth, mp_cnt, re_obs, s);
    else {
      const int4 r = X.rec[t];
      mp_cnt = r.y, re_obs = r.z;
    }
    int decision = kKept;
    if (10 * re_obs > 9 * mp_cnt) {  // `re_obs > 0.9 * mp_cnt` (:487), exact for every count a store holds
      if (X.locked[k]) {             // notEraseLoopDetecting_ (keyframe.cpp:408-412)
        decision = kPending;
        if (threadIdx.x == 0) X.pending[k] = 1;
      } else {
        decision = kErased, recount = true;
        erase_keyframe(S, O, C, X, k, s64);
      }
    }
    if (threadIdx.x == 0) X.rec[t] = make_int4(k, mp_cnt, re_obs, decision);
  }
}

__global__ __launch_bounds__(kSeqThreads) void k_erase_one(KfStoreView S, KfObsView O, KfConnView C, KfCullView X, int k) {
  __shared__ unsigned long long s64[kSeqThreads];
  if (k <= 0 || k >= S.size || X.erased[k]) return;  // `if (id_ == 0) return;` (keyframe.cpp:402)
  if (X.locked[k]) {
    if (threadIdx.x == 0) X.pending[k] = 1;
    return;
  }
  erase_keyframe(S, O, C, X, k, s64);
}

__global__ void k_cull_init(KfCullView X, int max_kf) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)max_kf * X.NK;
  if (e < total) {
    const int k = (int)(e / X.NK), i = (int)(e - (size_t)k * X.NK);
    cull_octave(X, k)[i] = 0, cull_depth(X, k)[i] = -1.f, cull_uright(X, k)[i] = -1.f;  // Frame::findDepth's "no depth"
  }
  if (e < (size_t)max_kf) X.erased[e] = X.locked[e] = X.pending[e] = 0, X.rec[e] = make_int4(-1, 0, 0, 0);
  if (e == 0) X.n_rec[0] = 0;
}

__global__ void k_cull_lock(KfCullView X, int k, int on) {
  if (threadIdx.x == 0) X.locked[k] = on;
}

}  // namespace

namespace {

// cull_bytes is what cull_layout hands out of one block; cull_init writes the defaults; cull_enqueue is k_cull_count +
// k_cull_apply, erase_enqueue the erase alone, both without the ordering pass.  Launches only.
size_t cull_bytes(int max_kf, int NK) { return ((size_t)3 * max_kf * NK + (size_t)7 * max_kf + 4) * 4; }

KfCullView cull_layout(void *block, int max_kf, int NK) {
  KfCullView X{};
  const size_t K = (size_t)max_kf;
  int *p = reinterpret_cast<int *>(block);
  X.NK = NK;
  X.rec = reinterpret_cast<int4 *>(p), p += 4 * K;  // (first: 16-byte aligned)
  X.n_rec = p, p += 4;
  X.erased = p, X.locked = p + K, X.pending = p + 2 * K, p += 3 * K;
  X.cols = p;
  return X;
}

int cull_init(const KfCullView &X, int max_kf, hipStream_t st) {
  const size_t total = (size_t)max_kf * X.NK;
  hipLaunchKernelGGL(k_cull_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, max_kf);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int cull_set_lock(const KfCullView &X, int k, int on, hipStream_t st) {
  hipLaunchKernelGGL(k_cull_lock, dim3(1), dim3(64), 0, st, X, k, on ? 1 : 0);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int cull_enqueue(const KfStoreView &S, const KfObsView &O, const KfConnView &C, const KfCullView &X, int current, float th_depth,
                 hipStream_t st) {
  // (a key-frame's list holds at most size - 1 others; the workgroups beyond its length return at once)
  hipLaunchKernelGGL(k_cull_count, dim3(S.size), dim3(256), 0, st, S, O, C, X, current, th_depth);
  hipLaunchKernelGGL(k_cull_apply, dim3(1), dim3(kSeqThreads), 0, st, S, O, C, X, current, th_depth);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int erase_enqueue(const KfStoreView &S, const KfObsView &O, const KfConnView &C, const KfCullView &X, int keyframe, hipStream_t st) {
  hipLaunchKernelGGL(k_erase_one, dim3(1), dim3(kSeqThreads), 0, st, S, O, C, X, keyframe);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_culling(vo_kfstore *s) {
  const char *W = "vo_kfstore_enable_culling";
  if (const int rc = enable_begin(s, W, kLayerConnections, kLayerCulling)) return rc < 0 ? rc : VO_OK;
  VO_CHECK(s->cull.reserve(cull_bytes(s->max_kf, s->NK)));
  s->X = cull_layout(s->cull.p, s->max_kf, s->NK);
  VO_CHECK(cull_init(s->X, s->max_kf, s->st));
  VO_CHECK(stream_sync(s->st, W));
  connections_set_erased(s->conn, s->X.erased);
  s->layers |= kLayerCulling;
  return VO_OK;
}

int vo_kfstore_set_keypoints(vo_kfstore *s, int keyframe, const int32_t *octave, const float *depth, const float *u_right) {
  const char *W = "vo_kfstore_set_keypoints";
  VO_CHECK(need(s, W, kLayerCulling));
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
  VO_CHECK(copy_h2d(cull_octave(s->X, keyframe), h, NK * 12, s->st, W));
  return stream_sync(s->st, W);
}

int vo_kfstore_set_keypoints_dev(vo_kfstore *s, int keyframe, const int32_t *dev_octave, const float *dev_depth, const float *dev_u_right) {
  const char *W = "vo_kfstore_set_keypoints_dev";
  VO_CHECK(need(s, W, kLayerCulling));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!dev_octave || !dev_depth || !dev_u_right) return VO_ERR_INVALID;
  s->gen++;
  VO_HIP_CHECK(hipMemcpyAsync(cull_octave(s->X, keyframe), dev_octave, n * 4, hipMemcpyDeviceToDevice, s->st));
  VO_HIP_CHECK(hipMemcpyAsync(cull_depth(s->X, keyframe), dev_depth, n * 4, hipMemcpyDeviceToDevice, s->st));
  VO_HIP_CHECK(hipMemcpyAsync(cull_uright(s->X, keyframe), dev_u_right, n * 4, hipMemcpyDeviceToDevice, s->st));
  return VO_OK;
}

int vo_kfstore_set_erase_lock(vo_kfstore *s, int keyframe, int on) {
  const char *W = "vo_kfstore_set_erase_lock";
  VO_CHECK(need(s, W, kLayerCulling));
  VO_CHECK(need_keyframe(s, W, keyframe));
  s->gen++;
  return cull_set_lock(s->X, keyframe, on, s->st);
}

int vo_kfstore_cull_keyframes(vo_kfstore *s, int current, float th_depth) {
  const char *W = "vo_kfstore_cull_keyframes";
  VO_CHECK(need(s, W, kLayerCulling));
  VO_CHECK(need_keyframe(s, W, current));
  // (that `current` has not been erased only the device knows: the kernels then walk no candidate and raise the sticky
  //  VO_KFSTORE_CONNECTIONS_INVALID)
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  VO_CHECK(cull_enqueue(kfstore_view(s), O, connections_view(s->conn), s->X, current, th_depth, s->st));
  s->obs_dirty = true, s->gen++;  // (whether anything was erased only the device knows)
  return connections_order(s->conn, s->size, s->st);
}

int vo_kfstore_erase_keyframe(vo_kfstore *s, int keyframe) {
  const char *W = "vo_kfstore_erase_keyframe";
  VO_CHECK(need(s, W, kLayerCulling));
  VO_CHECK(need_keyframe(s, W, keyframe));
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  VO_CHECK(erase_enqueue(kfstore_view(s), O, connections_view(s->conn), s->X, keyframe, s->st));
  s->obs_dirty = true, s->gen++;
  return connections_order(s->conn, s->size, s->st);
}

int vo_kfstore_cull_result(vo_kfstore *s, int32_t *n_candidates, int32_t *keyframes, int32_t *mp_cnt, int32_t *re_obs, int32_t *decision) {
  const char *W = "vo_kfstore_cull_result";
  VO_CHECK(need(s, W, kLayerCulling));
  if (!n_candidates) return VO_ERR_INVALID;
  std::vector<int32_t> rec((size_t)s->size * 4 + 4);
  int32_t n = 0;
  VO_CHECK(copy_d2h(&n, s->X.n_rec, 4, s->st, W));
  if (s->size > 0) VO_CHECK(copy_d2h(rec.data(), s->X.rec, (size_t)s->size * 16, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
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
  VO_CHECK(need(s, W, kLayerCulling));
  VO_CHECK(need_keyframe(s, W, keyframe));
  int32_t w[3] = {0, 0, 0};
  VO_CHECK(copy_d2h(w, s->X.erased + keyframe, 4, s->st, W));
  VO_CHECK(copy_d2h(w + 1, s->X.locked + keyframe, 4, s->st, W));
  VO_CHECK(copy_d2h(w + 2, s->X.pending + keyframe, 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  if (erased) *erased = w[0];
  if (locked) *locked = w[1];
  if (pending) *pending = w[2];
  return VO_OK;
}

}  // extern "C"
