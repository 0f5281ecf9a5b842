// local_ba_store.hip -- local bundle adjustment from the key-frame store: the window of
// Optimizer::solveLocalBAPoseAndPoint (optimizer_ceres.cpp:449-592) assembled on the device from the observation index, its
// write-back (:757-804) with MapPoint::eraseObservedKF / eraseMapPoint (mappoint.cpp:333-381), and
// MapPoint::updateNormalAndDepth (mappoint.cpp:66-116).  The solve in between is vo_ba's, unchanged (kfstore.hip).
//   k_ba_cams    ONE workgroup: `current`, then its ordered list in list order, bad entries marked but left out
//   k_ba_count   a thread per (list position, feature): is this entry the first occurrence of its id?  Counts per workgroup
//   k_ba_points  the same grid: the first occurrences ranked in order (workgroup counts summed, ballot ranks inside), the
//                point's id and position, and ONE walk over its holders: edges counted, holders without a camera counted,
//                non-local non-bad holders marked as fixed cameras
//   k_ba_layout  ONE workgroup: fixed cameras in ascending key-frame number, the capacities, a camera per thread for
//                [upsilon; omega] = log(Tcw), the exclusive scan of the points' edge counts
//   k_ba_edges   a lane per point: its holders again, each edge written at the point's offset
//   k_ba_erase   a lane per point: the erased edges' key-frames leave the holders, the point dies when obs <= 2; a thread
//                per free camera writes its pose
//   k_ba_refresh a lane per point: the new position into every live feature that carries it, then updateNormalAndDepth
//                (refresh_point.h: the body, shared with the loop correction)
// Nothing depends on which thread runs when: positions come from counts and scans, the atomics are integer sums, and every
// byte and word of the store has one writer per launch (an entry of the index carries one id, a point has one lane).
// Compiled with -ffp-contract=off: the refresh rounds every double operation on its own, in the order section 4k writes down.
#include "kfstore.h"

#include "ba_math.h"
#include "new_points_geom.h"
#include "obs_walk.h"
#include "refresh_point.h"

#include <algorithm>

namespace {

using namespace vo;

enum { kOk = VO_KFSTORE_BA_WINDOW_OK, kEmpty = VO_KFSTORE_BA_WINDOW_EMPTY, kOverflow = VO_KFSTORE_BA_WINDOW_OVERFLOW };

struct BaLayout {
  uint8_t *block;
  size_t at = 0;
  template <class T>
  void take(T *&field, size_t bytes) {
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += up16(bytes);
  }
};

void ba_layout(BaLayout &L, KfBaView &B, int max_kf, int NK, int C, int P, int E) {
  const size_t K = (size_t)max_kf, N = (size_t)NK;
  L.take(B.ref_kf, K * N * 4);
  L.take(B.mark, K * 4);
  L.take(B.fixm, K * 4);
  L.take(B.lcam, K * 4);
  L.take(B.blk, ((K * N + 255) / 256) * 4);
  L.take(B.pt_ne, ((size_t)P + 1) * 4);
  L.take(B.ids_in, (size_t)P * 4);
  L.take(B.dead, (size_t)P);
  const size_t w0 = L.at;
  L.take(B.rec, (size_t)kBaRecInts * 4);
  L.take(B.cam_kf, (size_t)C * 4);
  L.take(B.cam_fixed, (size_t)C);
  L.take(B.poses6, (size_t)C * 48);
  L.take(B.pt_id, (size_t)P * 4);
  L.take(B.points, (size_t)P * 24);
  L.take(B.e_cam, (size_t)E * 4);
  L.take(B.e_pt, (size_t)E * 4);
  L.take(B.e_feat, (size_t)E * 4);
  L.take(B.e_obs, (size_t)E * 24);
  L.take(B.e_isg, (size_t)E * 8);
  B.win = reinterpret_cast<uint8_t *>(B.rec), B.win_bytes = L.at - w0;
  B.in_bytes = up16((size_t)C * 96 + (size_t)P * 24 + (size_t)E);
  L.take(B.in, B.in_bytes);
}

__device__ __forceinline__ int n_features(const KfStoreView &S, int k) { return min(max(kf_head(S, k)[0], 0), S.NK); }
__device__ __forceinline__ bool kf_bad(const KfStoreView &S, int k) { return kf_head(S, k)[1] != 0; }
__device__ __forceinline__ uint8_t *flag_byte(const KfStoreView &S, unsigned entry) {
  const unsigned k = entry / (unsigned)S.NK;
  return const_cast<uint8_t *>(kf_sec<uint8_t>(S, (int)k, S.o_flags)) + (entry - k * (unsigned)S.NK);
}

// exclusive prefix of `flag` over the workgroup in thread order; *total = the workgroup's sum (local_map.hip's block_rank).
// s_w: one int per wavefront.  Two barriers.
__device__ __forceinline__ int block_rank(bool flag, int *s_w, int *total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = (int)blockDim.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int below = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int base = 0, sum = 0;
  for (int i = 0; i < nw; i++) {
    const int c = s_w[i];
    if (i < w) base += c;
    sum += c;
  }
  *total = sum;
  return base + below;
}

struct WinArgs {
  KfStoreView S;
  KfObsView O;
  KfConnView C;
  KfCullView X;
  KfMapView M;
  KfBaView B;
  int current;
};

// ---- 1. local cameras (:449-463)
__global__ __launch_bounds__(1024) void k_ba_cams(WinArgs A) {
  __shared__ int s_w[16];
  const int tid = threadIdx.x, size = A.S.size, cur = A.current;
  const KfBaView &B = A.B;
  for (int k = tid; k < size; k += 1024) B.mark[k] = 0, B.fixm[k] = 0;
  if (tid < kBaRecInts) B.rec[tid] = tid == kBaCurrent ? cur : 0;
  __syncthreads();
  if (A.X.erased[cur] || !*np_pose_set(A.M, cur)) {  // (uniform) the window is empty
    if (tid == 0) B.rec[kBaStatus] = kEmpty, atomicOr(A.C.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
    return;
  }
  if (tid == 0) B.mark[cur] = 1, B.lcam[0] = cur;
  const int n = min(max(A.C.n_ordered[cur], 0), size);
  const int *list = A.C.ordered + (size_t)cur * A.C.max_kf;
  int base = 1;
  for (int t0 = 0; t0 < n; t0 += 1024) {
    const int t = t0 + tid, j = t < n ? list[t] : -1;
    const bool valid = j >= 0 && j < size && j != cur;
    const bool take = valid && !kf_bad(A.S, j);  // `if (!kf->isBad())` (:461)
    int total;
    const int pos = base + block_rank(take, s_w, &total);
    if (take && pos < size) B.mark[j] = pos + 1, B.lcam[pos] = j;  // (a list without repeats never reaches size)
    else if (valid) B.mark[j] = -1;  // localBAKFId_ is set before the test (:459): never a fixed camera
    base += total;
  }
  if (tid == 0) B.rec[kBaNLocal] = base;
}

// entry x = (list position, feature) of the local cameras: does it hold the FIRST occurrence of its id (:480-499)?  The keys of
// an id ascend in (key-frame, feature); an occurrence at a smaller (list position, entry) ends the walk (local_map.hip's test)
__device__ __forceinline__ bool ba_first(const WinArgs &A, int x, int n_local, int &k, int &i, int &id, unsigned &e) {
  const int NK = A.S.NK, size = A.S.size;
  if (x >= n_local * NK) return false;
  const int j = x / NK;
  i = x - j * NK, k = A.B.lcam[j];
  if (i >= n_features(A.S, k) || !(kf_sec<uint8_t>(A.S, k, A.S.o_flags)[i] & 1)) return false;
  id = kf_sec<int>(A.S, k, A.S.o_ids)[i];
  if (id < 0) return false;
  e = (unsigned)k * (unsigned)NK + (unsigned)i;
  const int own = j + 1;
  for (int s = max(A.O.run[e], 0); s < A.O.n_keys && (int)(A.O.keys[s] >> 32) == id; s++) {
    const unsigned ee = (unsigned)(A.O.keys[s] & 0xffffffffu);
    const int kk = (int)(ee / (unsigned)NK);
    if (kk >= size) continue;
    const int p = A.B.mark[kk];
    if (p > 0 && (p < own || (p == own && ee < e))) return false;
  }
  return true;
}

__global__ __launch_bounds__(256) void k_ba_count(WinArgs A) {
  int cnt = 0;
  if (A.B.rec[kBaStatus] == kOk) {
    int k, i, id;
    unsigned e;
    cnt = __syncthreads_count(ba_first(A, blockIdx.x * 256 + threadIdx.x, A.B.rec[kBaNLocal], k, i, id, e));
  }
  if (threadIdx.x == 0) A.B.blk[blockIdx.x] = cnt;
}

// ---- 2. points (:465-500), and per point the holder walk of :502-528 / :555-591 for counts and fixed marks
__global__ __launch_bounds__(256) void k_ba_points(WinArgs A) {
  __shared__ int s_w[4], s_sum[256];
  const KfBaView &B = A.B;
  if (B.rec[kBaStatus] != kOk) return;  // (uniform)
  const int tid = threadIdx.x, b = blockIdx.x, NK = A.S.NK, size = A.S.size;
  int part = 0;
  for (int t = tid; t < b; t += 256) part += B.blk[t];
  s_sum[tid] = part;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) s_sum[tid] += s_sum[tid + w];
    __syncthreads();
  }
  const int base = s_sum[0];
  int k = 0, i = 0, id = -1;
  unsigned e = 0;
  const bool first = B.blk[b] > 0 && ba_first(A, b * 256 + tid, B.rec[kBaNLocal], k, i, id, e);
  int total;
  const int q = base + block_rank(first, s_w, &total);
  if (first) {
    int n_edges = 0, n_dropped = 0;
    obs_run_holders(
        A.O, NK, size, A.O.run[e], id, [](int, unsigned) { return true; },
        [&](int kk, int) {
          const int m = B.mark[kk];
          if (m > 0) n_edges++;
          else if (m == 0 && !kf_bad(A.S, kk)) B.fixm[kk] = 1, n_edges++;  // (:512-525; every writer writes 1)
          else n_dropped++;  // a bad holder has no pose block (:561 would dereference null)
          return true;
        });
    if (q < B.max_points) {
      const double *P = kf_sec<double>(A.S, k, A.S.o_points) + 3 * (size_t)i;
      B.pt_id[q] = id, B.pt_ne[q] = n_edges;
      B.points[3 * (size_t)q] = P[0], B.points[3 * (size_t)q + 1] = P[1], B.points[3 * (size_t)q + 2] = P[2];
    }
    if (n_edges) atomicAdd(B.rec + kBaNEdges, n_edges);
    if (n_dropped) atomicAdd(B.rec + kBaNDropped, n_dropped);
  }
  if (b == (int)gridDim.x - 1 && tid == 0) B.rec[kBaNPoints] = base + total;
}

// ---- 3. fixed cameras (:502-528), capacities, 5. poses, and the edge offsets
__global__ __launch_bounds__(1024) void k_ba_layout(WinArgs A) {
  __shared__ int s_w[16], s_scan[1024];
  const KfBaView &B = A.B;
  if (B.rec[kBaStatus] != kOk) return;  // (uniform, like every return below)
  const int tid = threadIdx.x, size = A.S.size;
  const int n_local = B.rec[kBaNLocal], n_points = B.rec[kBaNPoints], n_edges = B.rec[kBaNEdges];
  for (int c = tid; c < min(n_local, B.max_cams); c += 1024) B.cam_kf[c] = B.lcam[c];
  int base = n_local;
  for (int k0 = 0; k0 < size; k0 += 1024) {
    const int k = k0 + tid;
    const bool f = k < size && B.fixm[k] != 0;
    int total;
    const int pos = base + block_rank(f, s_w, &total);
    if (f) {
      B.mark[k] = pos + 1;
      if (pos < B.max_cams) B.cam_kf[pos] = k;
    }
    base += total;
  }
  const int n_cams = base;
  if (tid == 0) B.rec[kBaNCams] = n_cams, B.rec[kBaNFixed] = n_cams - n_local;
  if (n_cams > B.max_cams || n_points > B.max_points || n_edges > B.max_edges) {  // nothing is truncated: the counts are true
    if (tid == 0) B.rec[kBaStatus] = kOverflow, atomicOr(A.C.status, (int)VO_KFSTORE_LOCAL_BA_CAPACITY);
    return;
  }
  __syncthreads();  // cam_kf is complete
  int no_pose = 0;
  for (int c = tid; c < n_cams; c += 1024) {
    const int k = B.cam_kf[c];
    B.cam_fixed[c] = (c >= n_local || k == 0) ? 1 : 0;  // (:578)
    if (!*np_pose_set(A.M, k)) {
      no_pose = 1;
      continue;
    }
    const double *T = np_pose(A.M, k);
    ba::se3_log_from_R(T, T + 9, B.poses6 + 6 * (size_t)c);
  }
  if (__syncthreads_or(no_pose)) {
    if (tid == 0) {
      for (int r = kBaNCams; r <= kBaNDropped; r++) B.rec[r] = 0;
      B.rec[kBaStatus] = kEmpty, atomicOr(A.C.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
    }
    return;
  }
  // pt_ne: counts -> exclusive offsets, pt_ne[n_points] = n_edges
  int carry = 0;
  for (int p0 = 0; p0 < n_points; p0 += 1024) {
    const int p = p0 + tid, v = p < n_points ? B.pt_ne[p] : 0;
    s_scan[tid] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int add = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    if (p < n_points) B.pt_ne[p] = carry + s_scan[tid] - v;
    carry += s_scan[1023];
    __syncthreads();
  }
  if (tid == 0) B.pt_ne[n_points] = n_edges;
}

// ---- 4. edges (:550-592)
__global__ __launch_bounds__(256) void k_ba_edges(WinArgs A) {
  const KfBaView &B = A.B;
  if (B.rec[kBaStatus] != kOk) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= B.rec[kBaNPoints]) return;
  const int id = B.pt_id[j];
  int at = B.pt_ne[j];
  obs_run_holders(
      A.O, A.S.NK, A.S.size, obs_lower_bound(A.O, id), id, [](int, unsigned) { return true; },
      [&](int kk, int f) {
        const int c = B.mark[kk];
        if (c <= 0) return true;
        const size_t d = (size_t)at++;
        B.e_cam[d] = c - 1, B.e_pt[d] = j, B.e_feat[d] = f;
        B.e_obs[3 * d] = (double)np_x(A.M, kk)[f], B.e_obs[3 * d + 1] = (double)np_y(A.M, kk)[f];
        B.e_obs[3 * d + 2] = (double)cull_uright(A.X, kk)[f];
        B.e_isg[d] = __ddiv_rn(1.0, (double)A.M.sf[min(max(cull_octave(A.X, kk)[f], 0), 15)]);  // (:564)
        return true;
      });
}

struct ApplyArgs {
  KfStoreView S;
  KfObsView O;
  KfCullView X;
  KfMapView M;
  KfBaView B;
  double *normals;
  int *status;
  int n_cams, n_points, n_edges;
};

// ---- a. erased edges, b. point death, c. poses (:760-791)
__global__ __launch_bounds__(256) void k_ba_erase(ApplyArgs A) {
  const KfBaView &B = A.B;
  const int t = blockIdx.x * 256 + threadIdx.x, NK = A.S.NK, size = A.S.size;
  if (t < A.n_cams && !B.cam_fixed[t]) {
    const double *src = reinterpret_cast<const double *>(B.in) + 12 * (size_t)t;
    double *dst = np_pose(A.M, B.cam_kf[t]);
    for (int c = 0; c < 12; c++) dst[c] = src[c];
  }
  if (t >= A.n_points) return;
  const uint8_t *erase = B.in + (size_t)A.n_cams * 96 + (size_t)A.n_points * 24;
  const int id = B.pt_id[t], end = B.pt_ne[t + 1], start = obs_lower_bound(A.O, id);
  int ei = B.pt_ne[t], prev = -1, left = 0, n_erased = 0, n_f0 = 0;
  // the point's edges and its keys both ascend in key-frame number: one merge.  Bit 0 goes in EVERY feature of an erased
  // edge's key-frame that carries the id (the store has one fact where the reference has two: no Q-B3, and a second feature
  // does not turn the key-frame back into a holder)
  obs_run_each(A.O, start, id, [&](unsigned e) {
    const int kk = (int)(e / (unsigned)NK);
    if (kk >= size) return true;
    while (ei < end && B.cam_kf[B.e_cam[ei]] < kk) ei++;
    if (ei < end && B.cam_kf[B.e_cam[ei]] == kk && erase[ei]) {
      uint8_t *fb = flag_byte(A.S, e);
      *fb = (uint8_t)(*fb & ~1);
      if (kk != prev) n_erased++, n_f0 += e - (unsigned)kk * (unsigned)NK == 0u;
    } else if (kk != prev) {
      left += cull_uright(A.X, kk)[e - (unsigned)kk * (unsigned)NK] >= 0.f ? 2 : 1;  // observe_cnt_ of what remains
    }
    prev = kk;
    return true;
  });
  const bool dies = n_erased > 0 && left <= 2;  // (mappoint.cpp:353: only an erase looks at the count)
  B.dead[t] = dies ? 1 : 0;
  if (dies)  // eraseMapPoint (mappoint.cpp:362-381), as section 4i does: bit 0 in every feature that carries the id
    obs_run_each(A.O, start, id, [&](unsigned e) {
      if ((int)(e / (unsigned)NK) < size) {
        uint8_t *fb = flag_byte(A.S, e);
        *fb = (uint8_t)(*fb & ~1);
      }
      return true;
    });
  if (n_erased) atomicAdd(B.rec + kBaNErased, n_erased);
  if (n_f0) atomicAdd(B.rec + kBaNFeature0, n_f0);
  if (dies) atomicAdd(B.rec + kBaNDead, 1);
}

// ---- d. points (:793-803) and MapPoint::updateNormalAndDepth (mappoint.cpp:66-116) for the n ids of `ids`; new_pos: [n][3]
// or NULL (the position is the store's row at the id's first live key); dead: [n] or NULL.  The index may be older than the
// flags: a key is live iff its flags byte has bit 0 now.
__global__ __launch_bounds__(256) void k_ba_refresh(ApplyArgs A, int n, const int *ids, const double *new_pos, const uint8_t *dead) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n || (dead && dead[t])) return;  // dead points are not refreshed, rows of cleared features keep their bytes
  const int id = ids[t];
  if (id < 0) return;  // (a device list's "no point here": the host forms validate their ids)
  double p[3] = {0, 0, 0};
  if (new_pos) p[0] = new_pos[3 * (size_t)t], p[1] = new_pos[3 * (size_t)t + 1], p[2] = new_pos[3 * (size_t)t + 2];
  refresh_point(A.S, A.O, A.X, A.M, A.B.ref_kf, A.normals, A.status, id, p, new_pos != nullptr);  // (refresh_point.h)
}

__global__ void k_ba_init(KfBaView B) {
  if (threadIdx.x < kBaRecInts) B.rec[threadIdx.x] = threadIdx.x == kBaStatus ? (int)kEmpty : 0;
}

}  // namespace

namespace {

size_t ba_store_bytes(int max_kf, int NK, int max_cams, int max_points, int max_edges) {
  BaLayout L{nullptr};
  KfBaView B{};
  ba_layout(L, B, max_kf, NK, max_cams, max_points, max_edges);
  return L.at;
}

KfBaView ba_store_layout(void *block, int max_kf, int NK, int max_cams, int max_points, int max_edges) {
  BaLayout L{reinterpret_cast<uint8_t *>(block)};
  KfBaView B{};
  ba_layout(L, B, max_kf, NK, max_cams, max_points, max_edges);
  B.max_cams = max_cams, B.max_points = max_points, B.max_edges = max_edges, B.NK = NK;
  return B;
}

int ba_store_init(const KfBaView &B, int max_kf, hipStream_t st) {
  VO_HIP_CHECK(hipMemsetAsync(B.ref_kf, 0xff, (size_t)max_kf * B.NK * 4, st));  // -1: unknown
  hipLaunchKernelGGL(k_ba_init, dim3(1), dim3(64), 0, st, B);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// five launches: local cameras, first-occurrence counts, points (with their edge counts and the fixed marks), layout (fixed
// cameras, capacities, poses, edge offsets), edges
int ba_window_enqueue(const KfStoreView &S, const KfObsView &O, const KfConnView &C, const KfCullView &X, const KfMapView &M,
                      const KfBaView &B, int current, hipStream_t st) {
  WinArgs A{S, O, C, X, M, B, current};
  const unsigned grid = (unsigned)(((size_t)S.size * S.NK + 255) / 256);  // (the local cameras are at most `size`)
  hipLaunchKernelGGL(k_ba_cams, dim3(1), dim3(1024), 0, st, A);
  hipLaunchKernelGGL(k_ba_count, dim3(grid), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_ba_points, dim3(grid), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_ba_layout, dim3(1), dim3(1024), 0, st, A);
  hipLaunchKernelGGL(k_ba_edges, dim3((unsigned)((B.max_points + 255) / 256)), dim3(256), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// two launches on the inputs in B.in: erase + death (and the poses), then write + refresh
int ba_apply_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                     double *normals, int *status, int n_cams, int n_points, int n_edges, hipStream_t st) {
  ApplyArgs A{S, O, X, M, B, normals, status, n_cams, n_points, n_edges};
  const int n = n_cams > n_points ? n_cams : n_points;
  hipLaunchKernelGGL(k_ba_erase, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
  if (n_points > 0)
    hipLaunchKernelGGL(k_ba_refresh, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, st, A, n_points, (const int *)B.pt_id,
                       reinterpret_cast<const double *>(B.in + (size_t)n_cams * 96), (const uint8_t *)B.dead);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// the refresh alone for the n ids in B.ids_in
int ba_refresh_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                       double *normals, int *status, int n, hipStream_t st) {
  if (n <= 0) return VO_OK;
  ApplyArgs A{S, O, X, M, B, normals, status, 0, 0, 0};
  hipLaunchKernelGGL(k_ba_refresh, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, n, (const int *)B.ids_in,
                     (const double *)nullptr, (const uint8_t *)nullptr);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace

namespace vo {

int ba_refresh_list_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                            double *normals, int *status, int n, const int *dev_ids, hipStream_t st) {
  if (n <= 0) return VO_OK;
  ApplyArgs A{S, O, X, M, B, normals, status, 0, 0, 0};
  hipLaunchKernelGGL(k_ba_refresh, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, n, dev_ids, (const double *)nullptr,
                     (const uint8_t *)nullptr);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace vo

extern "C" {

int vo_kfstore_enable_local_ba(vo_kfstore *s, int max_cams, int max_points, int max_edges) {
  const char *W = "vo_kfstore_enable_local_ba";
  const bool args_ok = max_cams >= 1 && max_points >= 1 && max_edges >= 1;
  if (const int rc = enable_begin(s, W, kLayerMapping, kLayerLocalBa, args_ok)) return rc < 0 ? rc : VO_OK;
  VO_CHECK(s->ba.reserve(ba_store_bytes(s->max_kf, s->NK, max_cams, max_points, max_edges)));
  s->B = ba_store_layout(s->ba.p, s->max_kf, s->NK, max_cams, max_points, max_edges);
  VO_CHECK(s->ba_win.stage.reserve(std::max(s->B.win_bytes, s->B.in_bytes)));
  s->ba_poses.resize((size_t)max_cams * 6), s->ba_points.resize((size_t)max_points * 3), s->ba_erase.resize((size_t)max_edges + 1);
  VO_CHECK(ba_store_init(s->B, s->max_kf, s->st));
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerLocalBa;
  return VO_OK;
}

int vo_kfstore_set_point_refs(vo_kfstore *s, int keyframe, const int32_t *ref_kf) {
  const char *W = "vo_kfstore_set_point_refs";
  VO_CHECK(need(s, W, kLayerLocalBa));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!ref_kf) return VO_ERR_INVALID;
  for (size_t i = 0; i < n; i++)
    if (ref_kf[i] < -1 || ref_kf[i] >= s->size) {
      set_error("%s: feature %zu: reference key-frame %d outside [-1, %d)", W, i, ref_kf[i], s->size);
      return VO_ERR_INVALID;
    }
  s->gen++;
  VO_CHECK(copy_h2d(s->B.ref_kf + (size_t)keyframe * s->NK, ref_kf, n * 4, s->st, W));
  return stream_sync(s->st, W);
}

int vo_kfstore_set_point_refs_dev(vo_kfstore *s, int keyframe, const int32_t *dev_ref_kf) {
  const char *W = "vo_kfstore_set_point_refs_dev";
  VO_CHECK(need(s, W, kLayerLocalBa));
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
  VO_CHECK(need(s, W, kLayerLocalBa));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!ref_kf) return VO_ERR_INVALID;
  VO_CHECK(copy_d2h(ref_kf, s->B.ref_kf + (size_t)keyframe * s->NK, n * 4, s->st, W));
  return stream_sync(s->st, W);
}

int vo_kfstore_local_ba_window(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_local_ba_window";
  VO_CHECK(need(s, W, kLayerLocalBa));
  VO_CHECK(need_keyframe(s, W, current));
  // (that `current` has been erased, or that a camera has no pose, only the device knows: the window is then empty)
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  VO_CHECK(ba_window_enqueue(kfstore_view(s), O, connections_view(s->conn), s->X, s->M, s->B, current, s->st));
  s->ba_win.begin(s->gen);
  return VO_OK;
}

int vo_kfstore_local_ba_window_result(vo_kfstore *s, int32_t *record, int32_t *cam_keyframe, uint8_t *cam_fixed, double *poses6,
                                      int32_t *point_id, double *points, int32_t *edge_cam, int32_t *edge_point,
                                      int32_t *edge_feature, double *edge_obs, double *edge_inv_sigma) {
  const char *W = "vo_kfstore_local_ba_window_result";
  VO_CHECK(need(s, W, kLayerLocalBa));
  const KfBaView &B = s->B;
  const KfWindow &win = s->ba_win;
  VO_CHECK(s->ba_win.fetch(B.win, B.win_bytes, false, s->st, W));
  const int32_t *r = win.rec;
  if (record) memcpy(record, r, sizeof(win.rec));
  if (r[kBaStatus] != VO_KFSTORE_BA_WINDOW_OK) return VO_OK;
  const size_t nc = (size_t)r[kBaNCams], np = (size_t)r[kBaNPoints], ne = (size_t)r[kBaNEdges];
  if (cam_keyframe) memcpy(cam_keyframe, win.staged(B.cam_kf, B.win), nc * 4);
  if (cam_fixed) memcpy(cam_fixed, win.staged(B.cam_fixed, B.win), nc);
  if (poses6) memcpy(poses6, win.staged(B.poses6, B.win), nc * 48);
  if (point_id) memcpy(point_id, win.staged(B.pt_id, B.win), np * 4);
  if (points) memcpy(points, win.staged(B.points, B.win), np * 24);
  if (edge_cam) memcpy(edge_cam, win.staged(B.e_cam, B.win), ne * 4);
  if (edge_point) memcpy(edge_point, win.staged(B.e_pt, B.win), ne * 4);
  if (edge_feature) memcpy(edge_feature, win.staged(B.e_feat, B.win), ne * 4);
  if (edge_obs) memcpy(edge_obs, win.staged(B.e_obs, B.win), ne * 24);
  if (edge_inv_sigma) memcpy(edge_inv_sigma, win.staged(B.e_isg, B.win), ne * 8);
  return VO_OK;
}

int vo_kfstore_local_ba_apply(vo_kfstore *s, const double *poses6, const double *points, const uint8_t *edge_erase) {
  const char *W = "vo_kfstore_local_ba_apply";
  VO_CHECK(need(s, W, kLayerLocalBa));
  VO_CHECK(s->ba_win.check_apply(W, s->gen, s->B.win, s->st));
  const int32_t *r = s->ba_win.rec;
  const size_t nc = (size_t)r[kBaNCams], np = (size_t)r[kBaNPoints], ne = (size_t)r[kBaNEdges];
  if (!poses6 || (np > 0 && !points) || (ne > 0 && !edge_erase)) return VO_ERR_INVALID;
  // staged as the kernels read it: Tcw12 per camera (SE3::exp on the host, :786-788) | points | erase bytes
  uint8_t *h = s->ba_win.stage.data();
  double *T = reinterpret_cast<double *>(h);
  for (size_t c = 0; c < nc; c++) VO_CHECK(vo_se3_exp(poses6 + 6 * c, T + 12 * c, T + 12 * c + 9));
  if (np) memcpy(h + nc * 96, points, np * 24);
  if (ne) memcpy(h + nc * 96 + np * 24, edge_erase, ne);
  const size_t bytes = nc * 96 + np * 24 + ne;
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // (not stale: nothing has changed since the window)
  VO_CHECK(copy_h2d(s->B.in, h, bytes, s->st, W));
  VO_CHECK(ba_apply_enqueue(kfstore_view(s), O, s->X, s->M, s->B, s->normals.as<double>(), connections_view(s->conn).status, (int)nc,
                            (int)np, (int)ne, s->st));
  s->obs_dirty = true, s->gen++;
  return stream_sync(s->st, W);  // (the staging block is free again)
}

int vo_kfstore_refresh_points(vo_kfstore *s, int n, const int32_t *ids) {
  const char *W = "vo_kfstore_refresh_points";
  VO_CHECK(need(s, W, kLayerLocalBa));
  if (n < 0 || (n > 0 && !ids)) return VO_ERR_INVALID;
  if (n > s->B.max_points) {
    set_error("%s: %d ids, the store was enabled for %d points", W, n, s->B.max_points);
    return VO_ERR_CAPACITY;
  }
  for (int i = 0; i < n; i++)
    if (ids[i] < 0) {
      set_error("%s: entry %d: id %d is negative", W, i, ids[i]);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  VO_CHECK(copy_h2d(s->B.ids_in, ids, (size_t)n * 4, s->st, W));
  VO_CHECK(ba_refresh_enqueue(kfstore_view(s), O, s->X, s->M, s->B, s->normals.as<double>(), connections_view(s->conn).status, n, s->st));
  s->gen++;  // (flags and ids stay: the index does not go stale)
  return stream_sync(s->st, W);
}

int vo_kfstore_local_ba(vo_kfstore *s, vo_ba *ba, int current, const volatile unsigned char *stop, vo_lm_summary *summaries) {
  const char *W = "vo_kfstore_local_ba";
  VO_CHECK(need(s, W, kLayerLocalBa));
  if (!ba) return VO_ERR_INVALID;
  VO_CHECK(vo_kfstore_local_ba_window(s, current));
  const KfBaView &B = s->B;
  const KfWindow &win = s->ba_win;
  VO_CHECK(s->ba_win.fetch(B.win, B.win_bytes, false, s->st, W));  // the ONE device-to-host copy
  const int32_t *r = win.rec;
  if (r[kBaStatus] == VO_KFSTORE_BA_WINDOW_OVERFLOW) {
    set_error("%s: %d cameras, %d points, %d edges; the store was enabled for %d, %d, %d", W, r[kBaNCams], r[kBaNPoints], r[kBaNEdges],
              B.max_cams, B.max_points, B.max_edges);
    return VO_ERR_CAPACITY;
  }
  if (r[kBaStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    set_error("%s: the window of key-frame %d is empty (erased, or a camera without a pose)", W, current);
    return VO_ERR_INVALID;
  }
  const double cam[5] = {s->M.cam[0], s->M.cam[1], s->M.cam[2], s->M.cam[3], s->M.cam[4]};  // float members widened (:543-548)
  VO_CHECK(vo_ba_reset(ba, r[kBaNCams], win.staged(B.poses6, B.win), win.staged(B.cam_fixed, B.win), r[kBaNPoints],
                       win.staged(B.points, B.win), r[kBaNEdges], win.staged(B.e_cam, B.win), win.staged(B.e_pt, B.win),
                       win.staged(B.e_obs, B.win), win.staged(B.e_isg, B.win), cam));
  VO_CHECK(vo_ba_local_ba(ba, stop, s->ba_erase.data(), summaries));  // (VO_ERR_STOPPED: the return at :594, no write-back)
  VO_CHECK(vo_ba_get_state(ba, s->ba_poses.data(), s->ba_points.data()));
  return vo_kfstore_local_ba_apply(s, s->ba_poses.data(), s->ba_points.data(), s->ba_erase.data());
}

}  // extern "C"
