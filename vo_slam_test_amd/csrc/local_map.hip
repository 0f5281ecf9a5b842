// local_map.hip -- vo_tracker_build_local_map's kernels: VisualOdometry::updateLocalKeyFrames and
// updateLocalMapPoints (visualOdometry.cpp:595-724) for every frame of a batch, from the key-frame store.  Two launches, a
// workgroup per frame each:
//   k_lm_keyframes  votes through the observation index (:598-614), the voters in ascending key-frame number with the best
//                   one (:625-639), the expansion over the covisibility graph and the spanning tree (:641-690)
//   k_lm_points     the list's key-frames in list order, their flagged features in index order, first occurrence of an id
//                   wins (:700-724) -- decided per entry from the observation index, compacted in order by a block scan,
//                   written straight into the tracker's local-map arrays
// Nothing here depends on which thread runs when: the vote counts are integer sums, the list is built by one thread, and
// "first occurrence" is a property of the sorted index, not of an atomic race.
#include "kfstore.h"

namespace {

using namespace vo;

constexpr int kMaxKf = VO_TRACKER_LOCAL_MAX_KEYFRAMES;
constexpr int kStop = 80;  // `if (localKeyframes_.size() > 80) break;` (:643)

__device__ __forceinline__ int load_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive prefix of `flag` (0 / 1) over the workgroup in thread order; *total = the workgroup's sum.  s_w: one int per
// wavefront.  Two barriers.
__device__ __forceinline__ int block_rank(bool flag, int *s_w, int *total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = (int)blockDim.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int below = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();  // (s_w of the previous round has been read)
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

// first key position whose id is >= `id`
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

__device__ __forceinline__ bool kf_bad(const KfStoreView &S, int k) { return kf_head(S, k)[1] != 0; }

__global__ __launch_bounds__(256) void k_lm_keyframes(LocalMapArgs A) {
  __shared__ int s_list[kMaxKf];
  __shared__ int s_w[4];
  __shared__ unsigned long long s_best[256];
  __shared__ int s_len;
  const int f = blockIdx.x, tid = threadIdx.x, size = A.S.size, NK = A.S.NK;
  int *votes = A.votes + (size_t)f * A.S.max_kf;
  const size_t o = (size_t)f * A.cap;
  const bool off = A.winner && A.winner[f] < 0;  // VO_TRACK_RELOC_FAILED: an empty local map, nothing else touched
  // (the scratch row is written and read by different threads of the workgroup, through device-scope accesses with a
  //  device-scope fence in front of each barrier that separates a writer from another thread's access to the same word)
  for (int k = tid; k < size; k += 256) store_agent(votes + k, 0);
  __threadfence();
  __syncthreads();
  // ---- 1. votes: every non-null slot, every key-frame that holds its id
  if (!off) {
    const int n = min(max(A.fn[f], 0), A.cap);
    int rk = -1, rn = 0;
    if (A.ref_kf) {
      rk = A.ref_kf[f];
      rn = rk >= 0 && rk < size ? min(max(kf_head(A.S, rk)[0], 0), NK) : 0;
    }
    for (int i = tid; i < n; i += 256) {
      if (!A.fhas[o + i]) continue;
      int id = -1;
      if (A.sid) {
        id = A.sid[o + i];
      } else {
        const int a = A.assigned[o + i];
        if (a >= 0 && a < rn) id = kf_sec<int>(A.S, rk, A.S.o_ids)[a];
      }
      bool held = false;
      if (id >= 0) {
        int prev = -1;
        for (int s = obs_lower_bound(A.O, id); s < A.O.n_keys && (int)(A.O.keys[s] >> 32) == id; s++) {
          const int k = (int)((unsigned)(A.O.keys[s] & 0xffffffffu) / (unsigned)NK);
          if (k == prev || k >= size) continue;  // (two features of one key-frame: one observation)
          prev = k, held = true;
          atomicAdd(votes + k, 1);
        }
      }
      if (!held) {  // `mp->isBad()`: the slot is nulled (:612)
        A.fhas[o + i] = 0, A.fobs[o + i] = 0;
        if (A.sid) A.sid[o + i] = -1;
      }
    }
  }
  __threadfence();
  __syncthreads();
  // ---- 2. voters in ascending key-frame number, bad ones skipped; the first with the strictly largest count
  int base = 0, best_c = 0, best_k = -1;
  for (int k0 = 0; k0 < size; k0 += 256) {
    const int k = k0 + tid;
    const int c = k < size ? load_agent(votes + k) : 0;
    const bool v = c > 0 && !kf_bad(A.S, k);
    if (v && c > best_c) best_c = c, best_k = k;
    int total;
    const int pos = base + block_rank(v, s_w, &total);
    if (v && pos < kMaxKf) s_list[pos] = k;
    base += total;
  }
  s_best[tid] = best_k < 0 ? 0ull : ((unsigned long long)(unsigned)best_c << 32) | (unsigned)(0x7fffffff - best_k);
  __syncthreads();
  // ---- 3. expansion: one thread, as the reference's loop is sequential
  if (tid == 0) {
    unsigned long long b = 0;
    for (int i = 0; i < 256; i++) b = s_best[i] > b ? s_best[i] : b;
    A.best[f] = b ? 0x7fffffff - (int)(b & 0xffffffffu) : -1;
    const int nv = base;
    int L = min(nv, kMaxKf);
    if (nv > kMaxKf) atomicOr(A.err, (int)kStoreErrLocalKfs);
    for (int v = 0; v < nv && L <= kStop; v++) {  // (L <= 80 here implies nv <= 80: every voter walked is in s_list)
      const int *g = A.O.graph + (size_t)s_list[v] * kKfGraphInts;
      const int n_nb = min(max(g[0], 0), kKfGraphNb), n_ch = min(max(g[1], 0), kKfGraphCh), parent = g[2];
      // a key-frame is marked (trackFrameId_ == the frame's id) when it is a voter or was added: votes != 0 and not bad
      for (int j = 0; j < n_nb; j++) {
        const int k = g[4 + j];
        if (k < 0 || k >= size || kf_bad(A.S, k)) continue;
        if (load_agent(votes + k) == 0) {
          s_list[L++] = k, store_agent(votes + k, -1);
          break;
        }
      }
      for (int j = 0; j < n_ch; j++) {
        const int k = g[16 + j];
        if (k < 0 || k >= size || kf_bad(A.S, k)) continue;
        if (load_agent(votes + k) == 0) {
          s_list[L++] = k, store_agent(votes + k, -1);
          break;
        }
      }
      if (parent >= 0 && parent < size && !kf_bad(A.S, parent) && load_agent(votes + parent) == 0)
        s_list[L++] = parent, store_agent(votes + parent, -1);
    }
    s_len = L;
    A.n_kf[f] = nv > kMaxKf ? nv : L;
  }
  __syncthreads();
  const int L = s_len;
  for (int j = tid; j < kMaxKf; j += 256) A.lkf[(size_t)f * kMaxKf + j] = j < L ? s_list[j] : -1;
  // the scratch row becomes list position + 1 per key-frame (0: not in the list) for k_lm_points
  for (int k = tid; k < size; k += 256) store_agent(votes + k, 0);
  __threadfence();
  __syncthreads();
  for (int j = tid; j < L; j += 256) store_agent(votes + s_list[j], j + 1);
}

__global__ __launch_bounds__(1024) void k_lm_points(LocalMapArgs A) {
  __shared__ int s_w[16];
  __shared__ int s_kf[kMaxKf], s_n[kMaxKf];
  const int f = blockIdx.x, tid = threadIdx.x, size = A.S.size, NK = A.S.NK;
  const int *lpos = A.votes + (size_t)f * A.S.max_kf;
  const int L = min(max(A.n_kf[f], 0), kMaxKf);
  for (int j = tid; j < L; j += 1024) {
    const int k = A.lkf[(size_t)f * kMaxKf + j];
    s_kf[j] = k, s_n[j] = k >= 0 && k < size ? min(max(kf_head(A.S, k)[0], 0), NK) : 0;
  }
  __syncthreads();
  int ref = -1;
  if (A.ref_kf) {
    ref = A.ref_kf[f];
    if (ref < 0 || ref >= size) ref = -1;
  }
  const size_t lo = (size_t)f * A.stride;
  const int E = L * NK;
  int base = 0;
  for (int x0 = 0; x0 < E; x0 += 1024) {
    const int x = x0 + tid;
    bool first = false;
    int k = 0, i = 0, id = -1, link = -1;
    if (x < E) {
      const int j = x / NK;
      i = x - j * NK, k = s_kf[j];
      if (i < s_n[j] && (kf_sec<uint8_t>(A.S, k, A.S.o_flags)[i] & 1)) id = kf_sec<int>(A.S, k, A.S.o_ids)[i];
    }
    if (id >= 0) {
      // the holder of the id that comes first in (list position, feature index): the keys of an id ascend in (key-frame,
      // feature), so the first key of a key-frame is its lowest feature
      // The walk ends at the first holder that comes earlier (most entries of a well-shared id leave after a key or two);
      // only a first occurrence walks its id's whole run, and takes `link` from it.
      const unsigned e = (unsigned)k * (unsigned)NK + (unsigned)i;
      const int own = x / NK + 1;
      first = true;
      for (int s = A.O.run[e]; s < A.O.n_keys && (int)(A.O.keys[s] >> 32) == id; s++) {
        const unsigned ee = (unsigned)(A.O.keys[s] & 0xffffffffu);
        const int kk = (int)(ee / (unsigned)NK);
        if (kk >= size) continue;
        const int p = lpos[kk];
        if (p > 0 && (p < own || (p == own && ee < e))) {
          first = false;
          break;
        }
        if (kk == ref && link < 0) link = (int)(ee - (unsigned)kk * (unsigned)NK);
      }
    }
    int total;
    const int q = base + block_rank(first, s_w, &total);
    base += total;
    if (first && q < A.max_local) {
      const size_t d = lo + q;
      const double *P = kf_sec<double>(A.S, k, A.S.o_points) + 3 * (size_t)i;
      const double *Nv = A.O.normals + ((size_t)k * NK + i) * 3;
      for (int c = 0; c < 3; c++) A.p1[3 * d + c] = P[c], A.nrm1[3 * d + c] = Nv[c];
      A.mind1[d] = kf_sec<float>(A.S, k, A.S.o_mind)[i], A.maxd1[d] = kf_sec<float>(A.S, k, A.S.o_maxd)[i];
      const uint32_t *pd = kf_sec<uint32_t>(A.S, k, A.S.o_pdesc) + 8 * (size_t)i;
      uint32_t *od = reinterpret_cast<uint32_t *>(A.desc1) + 8 * d;
      for (int c = 0; c < 8; c++) od[c] = pd[c];
      A.pf1[d] = kf_sec<uint8_t>(A.S, k, A.S.o_flags)[i] & 3u;
      A.ids1[d] = id, A.link1[d] = link;
    }
  }
  if (tid == 0) {
    A.n_pts[f] = base;
    if (base > A.max_local) atomicOr(A.err, (int)kStoreErrLocalPoints);
  }
  for (int q = min(base, A.max_local) + tid; q < A.max_local; q += 1024) A.pf1[lo + q] = 0, A.ids1[lo + q] = -1, A.link1[lo + q] = -1;
}

}  // namespace

namespace vo {

int local_map_build(const LocalMapArgs &A, hipStream_t st) {
  hipLaunchKernelGGL(k_lm_keyframes, dim3(A.B), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_lm_points, dim3(A.B), dim3(1024), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace vo
