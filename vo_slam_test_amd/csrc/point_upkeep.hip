// point_upkeep.hip -- map-point upkeep on the device: LocalMapping::processNewKeyFrame
// (localMapping.cpp:100-130) and cullingMapPoints (:496-524) with MapPoint::computeDescriptor (mappoint.cpp:118-179) and
// eraseMapPoint (:362-381), over the key-frame store's observation index.
//   k_up_desc_wave  a wavefront per id of the list: its run of the index 64 keys at a time, the non-bad holders ranked by
//                   ballot counts, lane r = holder r.  Each lane fetches its holder's 8 descriptor words (key -> key-frame,
//                   feature -> row); row i's words are broadcast, the lanes compute the distances, the median is the k-th
//                   smallest by k_median_desc's nine-step bisection over ballot counts.  More than 64 holders: the id goes
//                   to the overflow list (the atomic decides its position there, nothing else).
//   k_up_desc_over  a fixed grid strides the overflow list by the device-side count, a workgroup per id: the holders'
//                   descriptors staged in LDS at k_median_desc's 36-byte pitch (up to 1024), a wavefront per row.
//   k_up_classify   a thread per feature of `current`: is this its observation of the id, does another key-frame hold it
//                   (tracked), is it in the recent list already?
//   k_up_append     ONE workgroup: the new ids counted, then ranked in feature order behind the list -- or none of them
//   k_up_stats      a thread per (id, visible, found): the id's entry by a scan of the list, two integer atomic adds
//   k_up_cull       a thread per entry: holders and obs(p) from the index, the branch, and eraseMapPoint for branches 2 / 3
//   k_up_compact    ONE workgroup: the survivors packed in list order in place, the erased ids listed, the record
// No kernel waits on another workgroup; every loop is bounded by a count read once.  An id has one entry and an entry one
// thread, so every byte an erase clears has one writer; the descriptor of an id listed twice is written twice with the same
// bytes.
#include "kfstore.h"

#include "obs_walk.h"

#include <algorithm>

namespace {

using namespace vo;

constexpr int kSeq = 1024;      // threads of the one-workgroup kernels
constexpr int kOverGrid = 128;  // workgroups that stride the overflow list
enum { kDead = 1, kRatio = 2, kFewObs = 3, kMatured = 4, kKept = 5 };

__device__ __forceinline__ int n_features(const KfStoreView &S, int k) { return min(max(kf_head(S, k)[0], 0), S.NK); }
__device__ __forceinline__ bool kf_bad(const KfStoreView &S, int k) { return kf_head(S, k)[1] != 0; }
__device__ __forceinline__ uint8_t *record_of(const KfStoreView &S, int k) { return const_cast<uint8_t *>(S.base) + (size_t)k * S.rec; }
__device__ __forceinline__ int n_recent(const KfUpkeepView &U) { return min(max(U.head[0], 0), U.R); }

// exclusive prefix of `flag` over the workgroup in thread order; *total = the workgroup's sum.  s_w: one int per
// wavefront.  Two barriers.
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

// position of the n-th set bit of m (n counted from 0, n < popcount(m)): six halvings
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int n) {
  int pos = 0;
  for (int w = 32; w > 0; w >>= 1) {
    const int c = __popcll(m & (((1ull << w) - 1ull) << pos));
    if (n >= c) n -= c, pos += w;
  }
  return pos;
}

// key s of id's run (which starts at `start`): does it belong to the run, and is it its key-frame's OBSERVATION of the id by
// a key-frame that is not bad?  The index is fresh: every key is live, and the keys of a key-frame are adjacent.
__device__ __forceinline__ void run_key(const KfStoreView &S, const KfObsView &O, int start, int id, int s, bool &in, bool &holder,
                                        unsigned &e) {
  const unsigned long long key = s < O.n_keys ? O.keys[s] : ~0ull;
  in = s < O.n_keys && (int)(key >> 32) == id;
  e = (unsigned)(key & 0xffffffffu);
  holder = false;
  if (!in) return;
  const unsigned NK = (unsigned)S.NK, kk = e / NK;
  if ((int)kk >= S.size) return;
  if (s > start && (unsigned)(O.keys[s - 1] & 0xffffffffu) / NK == kk) return;  // a later feature of the same key-frame
  holder = !kf_bad(S, (int)kk);  // (:138)
}

__device__ __forceinline__ const uint32_t *desc_row(const KfStoreView &S, unsigned e) {
  const unsigned NK = (unsigned)S.NK, kk = e / NK;
  return kf_sec<uint32_t>(S, (int)kk, S.o_desc) + 8 * (size_t)(e - kk * NK);
}
__device__ __forceinline__ uint32_t *pdesc_row(const KfStoreView &S, unsigned e) {
  const unsigned NK = (unsigned)S.NK, kk = e / NK;
  return reinterpret_cast<uint32_t *>(record_of(S, (int)kk) + S.o_pdesc) + 8 * (size_t)(e - kk * NK);
}

// ---- MapPoint::computeDescriptor, N <= 64
__global__ __launch_bounds__(256) void k_up_desc_wave(KfStoreView S, KfObsView O, KfUpkeepView U, int n, const int *ids) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n) return;  // (uniform over the wavefront, like every return below)
  const int id = ids[t];
  if (id < 0) return;
  const int start = obs_lower_bound(O, id);
  int N = 0, run_len = 0;
  unsigned mine = 0;  // lane r: the entry of holder r
  for (int pos = start; pos < O.n_keys; pos += 64) {
    bool in, holder;
    unsigned e;
    run_key(S, O, start, id, pos + lane, in, holder, e);
    const unsigned long long hm = __ballot(holder), im = __ballot(in);
    const int cnt = __popcll(hm), want = lane - N;
    const unsigned got = (unsigned)__shfl((int)e, nth_set_bit(hm, want) & 63);
    if (want >= 0 && want < cnt) mine = got;
    N += cnt, run_len += __popcll(im);
    if (im != ~0ull || N > 64) break;
  }
  if (N == 0) return;  // `if (desp.empty()) return;` (:131, :142)
  if (N > 64) {
    if (lane == 0) {
      const int at = atomicAdd(U.head + 1, 1);
      if (at < U.L) U.over[at] = id;
    }
    return;
  }
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (lane < N) {
    const uint4 *d = reinterpret_cast<const uint4 *>(desc_row(S, mine));
    const uint4 a = d[0], b = d[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
  }
  const int k = (N - 1) / 2;  // int(0.5 * (N - 1)) (:166)
  int best_mid = 256, best = 0;  // (:159-160)
  for (int i = 0; i < N; i++) {
    const int row = __builtin_amdgcn_readfirstlane(i);
    int d = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) d += __popc(w[j] ^ (uint32_t)__builtin_amdgcn_readlane((int)w[j], row));
    int lo = 0, hi = 256;  // smallest v with #(d <= v) >= k + 1
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (__popcll(__ballot(lane < N && d <= mid)) >= k + 1) hi = mid;
      else lo = mid + 1;
    }
    if (lo < best_mid) best_mid = lo, best = i;  // strict: the first row wins (:168)
  }
  const int win = __builtin_amdgcn_readfirstlane(best);
  uint4 a, b;
  a.x = (uint32_t)__builtin_amdgcn_readlane((int)w[0], win), a.y = (uint32_t)__builtin_amdgcn_readlane((int)w[1], win);
  a.z = (uint32_t)__builtin_amdgcn_readlane((int)w[2], win), a.w = (uint32_t)__builtin_amdgcn_readlane((int)w[3], win);
  b.x = (uint32_t)__builtin_amdgcn_readlane((int)w[4], win), b.y = (uint32_t)__builtin_amdgcn_readlane((int)w[5], win);
  b.z = (uint32_t)__builtin_amdgcn_readlane((int)w[6], win), b.w = (uint32_t)__builtin_amdgcn_readlane((int)w[7], win);
  for (int s = start + lane; s < start + run_len; s += 64) {  // every feature that carries the id, bad key-frames included
    const unsigned e = (unsigned)(O.keys[s] & 0xffffffffu);
    if ((int)(e / (unsigned)S.NK) >= S.size) continue;
    uint4 *dst = reinterpret_cast<uint4 *>(pdesc_row(S, e));
    dst[0] = a, dst[1] = b;
  }
}

// ---- MapPoint::computeDescriptor, 64 < N <= 1024
__global__ __launch_bounds__(256) void k_up_desc_over(KfStoreView S, KfObsView O, KfUpkeepView U, int *status) {
  __shared__ uint32_t s_d[kUpDescMaxHolders * 9];
  __shared__ unsigned s_ent[kUpDescMaxHolders];
  __shared__ int s_w[4];
  __shared__ unsigned s_best;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_over = min(max(U.head[1], 0), U.L);
  for (int t = blockIdx.x; t < n_over; t += (int)gridDim.x) {
    const int id = U.over[t];
    const int start = obs_lower_bound(O, id);
    int N = 0, run_len = 0;
    for (int pos = start; pos < O.n_keys; pos += 256) {  // (every value that steers the loop is the workgroup's)
      bool in, holder;
      unsigned e;
      run_key(S, O, start, id, pos + tid, in, holder, e);
      int total;
      const int r = N + block_rank(holder, s_w, &total);
      if (holder && r < kUpDescMaxHolders) s_ent[r] = e;
      N += total;
      const int n_in = __syncthreads_count(in);
      run_len += n_in;
      if (n_in < 256) break;
    }
    __syncthreads();
    if (N == 0 || N > kUpDescMaxHolders) {  // the point keeps its descriptor
      if (N > 0 && tid == 0) atomicOr(status, (int)VO_KFSTORE_UPKEEP_CAPACITY);
      continue;
    }
    for (int i = tid; i < N * 8; i += 256) s_d[(i >> 3) * 9 + (i & 7)] = desc_row(S, s_ent[i >> 3])[i & 7];
    if (tid == 0) s_best = 256u << 16;
    __syncthreads();
    const int k = (N - 1) / 2;
    constexpr int NC = kUpDescMaxHolders / 64;
    for (int row = wave; row < N; row += 4) {
      uint32_t a[8];
#pragma unroll
      for (int j = 0; j < 8; j++) a[j] = s_d[row * 9 + j];
      int d[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) {
        d[c] = 0x7fff;
        const int col = lane + 64 * c;
        if (col < N) {
          int sum = 0;
#pragma unroll
          for (int j = 0; j < 8; j++) sum += __popc(a[j] ^ s_d[col * 9 + j]);
          d[c] = sum;
        }
      }
      int lo = 0, hi = 256;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < NC; c++)
          if (64 * c < N) cnt += __popcll(__ballot(d[c] <= mid));
        if (cnt >= k + 1) hi = mid;
        else lo = mid + 1;
      }
      if (lane == 0) atomicMin(&s_best, ((unsigned)lo << 16) | (unsigned)row);  // the smallest median, then the first row
    }
    __syncthreads();
    const uint32_t *win = s_d + (s_best & 0xffffu) * 9;
    for (int s = start + tid; s < start + run_len; s += 256) {
      const unsigned e = (unsigned)(O.keys[s] & 0xffffffffu);
      if ((int)(e / (unsigned)S.NK) >= S.size) continue;
      uint32_t *dst = pdesc_row(S, e);
#pragma unroll
      for (int j = 0; j < 8; j++) dst[j] = win[j];
    }
    __syncthreads();  // the staging arrays are the next id's
  }
}

// ---- processNewKeyFrame: the split (:112-125)
__global__ __launch_bounds__(256) void k_up_classify(KfStoreView S, KfObsView O, KfCullView X, KfUpkeepView U, int *status, int current) {
  const int i = blockIdx.x * 256 + threadIdx.x, NK = S.NK;
  const bool gone = X.erased[current] != 0;
  if (i == 0) {
    U.head[2] = current;
    if (gone) atomicOr(status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  }
  if (i >= NK) return;
  int tracked = -1, fresh = -1;
  if (!gone && i < n_features(S, current) && (kf_sec<uint8_t>(S, current, S.o_flags)[i] & 1)) {
    const int id = kf_sec<int>(S, current, S.o_ids)[i];
    if (id >= 0) {
      const unsigned mine = (unsigned)current * (unsigned)NK + (unsigned)i;
      bool first = true, other = false;
      obs_run_each(O, O.run[mine], id, [&](unsigned e) {
        const int kk = (int)(e / (unsigned)NK);
        if (kk >= S.size) return true;
        if (kk != current) other = true;
        else if (e < mine) first = false;  // a lower feature is current's observation of the id
        return first;
      });
      if (first && other) tracked = id;
      if (first && !other) {
        bool listed = false;
        for (int j = 0, n = n_recent(U); j < n && !listed; j++) listed = U.id[j] == id;
        if (!listed) fresh = id;
      }
    }
  }
  U.list[i] = tracked, U.cand[i] = fresh;
}

// the ids src[i * stride] >= 0, i < n_src, behind the recent list in that order with first_kf = current, found = visible = 1
// -- all of them or none (one workgroup); n_src: NULL or the device-side count, clamped to n_max
__global__ __launch_bounds__(kSeq) void k_up_append(KfUpkeepView U, int *status, int kind, int current, const int *src, int stride,
                                                    int n_max, const int *n_src) {
  __shared__ int s_w[kSeq / 64];
  const int tid = threadIdx.x;
  const int n = n_src ? min(max(*n_src, 0), n_max) : n_max, count0 = n_recent(U);
  int n_new = 0, n_tracked = 0;
  for (int i0 = 0; i0 < n; i0 += kSeq) {
    const int i = i0 + tid;
    int total;
    block_rank(i < n && src[(size_t)i * stride] >= 0, s_w, &total);
    n_new += total;
    if (kind == VO_KFSTORE_UPKEEP_PROCESS) {
      block_rank(i < n && U.list[i] >= 0, s_w, &total);
      n_tracked += total;
    }
  }
  const bool fits = count0 + n_new <= U.R;
  if (fits) {
    int at = count0;
    for (int i0 = 0; i0 < n; i0 += kSeq) {
      const int i = i0 + tid, id = i < n ? src[(size_t)i * stride] : -1;
      int total;
      const int r = at + block_rank(id >= 0, s_w, &total);
      if (id >= 0) U.id[r] = id, U.first_kf[r] = current, U.found[r] = 1, U.visible[r] = 1;  // (mappoint.cpp:38-41)
      at += total;
    }
  }
  __syncthreads();
  if (tid < kUpRecInts) {
    int v = 0;
    if (tid == kUpKind) v = kind;
    if (tid == kUpCurrent) v = current;
    if (tid == kUpNTracked) v = n_tracked;
    if (tid == kUpNNew) v = n_new;
    if (tid == kUpNAppended) v = fits ? n_new : 0;
    if (tid == kUpNRecent) v = fits ? count0 + n_new : count0;
    U.rec[tid] = v;
  }
  if (tid == 0) {
    if (fits) U.head[0] = count0 + n_new;
    else atomicOr(status, (int)VO_KFSTORE_UPKEEP_CAPACITY);
  }
}

// ---- found_cnt_ / visible_cnt_
__global__ __launch_bounds__(256) void k_up_stats(KfUpkeepView U, int n, const int *ids, const int *visible, const int *found) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int id = ids[t];
  if (id < 0) return;
  for (int j = 0, m = n_recent(U); j < m; j++)
    if (U.id[j] == id) {  // (an id has one entry)
      atomicAdd(U.visible + j, visible[t]), atomicAdd(U.found + j, found[t]);
      return;
    }
}

// ---- cullingMapPoints: the branch of every entry, and eraseMapPoint
__global__ __launch_bounds__(256) void k_up_cull(KfStoreView S, KfObsView O, KfCullView X, KfUpkeepView U, int current) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_recent(U)) return;
  const int id = U.id[t], start = obs_lower_bound(O, id), first = U.first_kf[t];
  int holders = 0, obs = 0;  // (the index is fresh: every key is live)
  obs_run_holders(
      O, S.NK, S.size, start, id, [](int, unsigned) { return true; },
      [&](int kk, int f) {
        holders++, obs += cull_uright(X, kk)[f] >= 0.f ? 2 : 1;
        return true;
      });
  int out = kKept;
  if (holders == 0) out = kDead;                                                          // isBad() (:505)
  else if (__fdiv_rn((float)U.found[t], (float)U.visible[t]) < 0.25f) out = kRatio;       // (:507, mappoint.cpp:330)
  else if (current > first + 2 && obs <= 3) out = kFewObs;                                // (:512)
  else if (current > first + 3) out = kMatured;                                           // (:517)
  if (out == kRatio || out == kFewObs)  // eraseMapPoint (mappoint.cpp:362-381): bit 0 in every feature that carries the id
    obs_run_each(O, start, id, [&](unsigned e) {
      const unsigned kk = e / (unsigned)S.NK;
      if ((int)kk < S.size) {
        uint8_t *b = record_of(S, (int)kk) + S.o_flags + (e - kk * (unsigned)S.NK);
        *b = (uint8_t)(*b & ~1);
      }
      return true;
    });
  U.outcome[t] = out;
}

// the survivors in list order, in place (a chunk is read whole before it is written, and nothing moves up); the erased ids;
// the record
__global__ __launch_bounds__(kSeq) void k_up_compact(KfUpkeepView U, int current) {
  __shared__ int s_w[kSeq / 64];
  const int tid = threadIdx.x, count0 = n_recent(U);
  int kept = 0, erased = 0, cnt[6] = {0, 0, 0, 0, 0, 0};
  for (int t0 = 0; t0 < count0; t0 += kSeq) {
    const int t = t0 + tid, out = t < count0 ? U.outcome[t] : 0;
    const int id = t < count0 ? U.id[t] : -1, fk = t < count0 ? U.first_kf[t] : 0;
    const int fo = t < count0 ? U.found[t] : 0, vi = t < count0 ? U.visible[t] : 0;
    int total;
    for (int b = kDead; b <= kMatured; b++) {
      block_rank(out == b, s_w, &total);
      cnt[b] += total;
    }
    const int re = erased + block_rank(out == kRatio || out == kFewObs, s_w, &total);
    if (out == kRatio || out == kFewObs) U.erased[re] = id;
    erased += total;
    const int rk = kept + block_rank(out == kKept, s_w, &total);  // (its barriers stand between the chunk's reads and writes)
    if (out == kKept) U.id[rk] = id, U.first_kf[rk] = fk, U.found[rk] = fo, U.visible[rk] = vi;
    kept += total;
  }
  __syncthreads();
  if (tid < kUpRecInts) {
    int v = 0;
    if (tid == kUpKind) v = VO_KFSTORE_UPKEEP_CULL;
    if (tid == kUpCurrent) v = current;
    if (tid == kUpNDead) v = cnt[kDead];
    if (tid == kUpNRatio) v = cnt[kRatio];
    if (tid == kUpNFewObs) v = cnt[kFewObs];
    if (tid == kUpNMatured) v = cnt[kMatured];
    if (tid == kUpNKept) v = kept;
    if (tid == kUpNErased) v = erased;
    if (tid == kUpNRecent) v = kept;
    U.rec[tid] = v;
  }
  if (tid == 0) U.head[0] = kept;
}

__global__ void k_up_init(KfUpkeepView U) {
  if (threadIdx.x < 4) U.head[threadIdx.x] = 0;
  if (threadIdx.x < kUpRecInts) U.rec[threadIdx.x] = 0;
}

struct UpLayout {
  uint8_t *block;
  size_t at = 0;
  void take(int *&field, size_t ints) {
    field = block ? reinterpret_cast<int *>(block + at) : nullptr;
    at += up16(ints * 4);
  }
};

void up_layout(UpLayout &L, KfUpkeepView &U, int R, int NK) {
  const size_t r = (size_t)R, n = (size_t)NK, l = r + n;
  L.take(U.head, 4);
  L.take(U.id, r), L.take(U.first_kf, r), L.take(U.found, r), L.take(U.visible, r);
  L.take(U.rec, kUpRecInts);
  L.take(U.erased, r);
  L.take(U.list, 3 * l);
  L.take(U.over, l);
  L.take(U.cand, n);
  L.take(U.outcome, r);
  U.R = R, U.NK = NK, U.L = (int)l;
}

}  // namespace

namespace {

size_t upkeep_bytes(int max_recent, int NK) {
  UpLayout L{nullptr};
  KfUpkeepView U{};
  up_layout(L, U, max_recent, NK);
  return L.at;
}

KfUpkeepView upkeep_layout(void *block, int max_recent, int NK) {
  UpLayout L{reinterpret_cast<uint8_t *>(block)};
  KfUpkeepView U{};
  up_layout(L, U, max_recent, NK);
  return U;
}

int upkeep_init(const KfUpkeepView &U, hipStream_t st) {
  hipLaunchKernelGGL(k_up_init, dim3(1), dim3(64), 0, st, U);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace

namespace vo {

int upkeep_descriptors_enqueue(const KfStoreView &S, const KfObsView &O, const KfUpkeepView &U, int *status, int n, const int *dev_ids,
                               hipStream_t st) {
  if (n <= 0) return VO_OK;
  VO_HIP_CHECK(hipMemsetAsync(U.head + 1, 0, 4, st));
  hipLaunchKernelGGL(k_up_desc_wave, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, S, O, U, n, dev_ids);
  hipLaunchKernelGGL(k_up_desc_over, dim3(kOverGrid), dim3(256), 0, st, S, O, U, status);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int upkeep_created_enqueue(const KfMapView &M, const KfUpkeepView &U, int *status, int current, hipStream_t st) {
  // the created rows are (key-frame, idx1, idx2, id): the ids at a stride of four, their number in the result record
  hipLaunchKernelGGL(k_up_append, dim3(1), dim3(kSeq), 0, st, U, status, (int)VO_KFSTORE_UPKEEP_CREATED, current,
                     reinterpret_cast<const int *>(M.created) + 3, 4, kKfGraphNb * M.NK, (const int *)(M.rec + 1));
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace vo

namespace {

// processNewKeyFrame up to the connection update: classify (U.list = the tracked ids, U.cand = the ids to append, per feature
// of `current`), refresh, descriptors, append
int upkeep_process_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                           const KfUpkeepView &U, double *normals, int *status, int current, hipStream_t st) {
  hipLaunchKernelGGL(k_up_classify, dim3((unsigned)((S.NK + 255) / 256)), dim3(256), 0, st, S, O, X, U, status, current);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(ba_refresh_list_enqueue(S, O, X, M, B, normals, status, S.NK, U.list, st));  // updateNormalAndDepth (:119)
  VO_CHECK(upkeep_descriptors_enqueue(S, O, U, status, S.NK, U.list, st));              // computeDescriptor (:120)
  hipLaunchKernelGGL(k_up_append, dim3(1), dim3(kSeq), 0, st, U, status, (int)VO_KFSTORE_UPKEEP_PROCESS, current, (const int *)U.cand, 1,
                     S.NK, (const int *)nullptr);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int upkeep_stats_enqueue(const KfUpkeepView &U, int n, const int *dev_ids, const int *dev_visible, const int *dev_found, hipStream_t st) {
  if (n <= 0) return VO_OK;
  hipLaunchKernelGGL(k_up_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, U, n, dev_ids, dev_visible, dev_found);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int upkeep_cull_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfUpkeepView &U, int current, hipStream_t st) {
  hipLaunchKernelGGL(k_up_cull, dim3((unsigned)((U.R + 255) / 256)), dim3(256), 0, st, S, O, X, U, current);
  hipLaunchKernelGGL(k_up_compact, dim3(1), dim3(kSeq), 0, st, U, current);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// "<W>: n ids, the store takes L": the longest id list a call takes
int up_list_fits(const vo_kfstore *s, const char *W, int n) {
  if (n <= s->U.L) return VO_OK;
  set_error("%s: %d ids, the store takes %d (max_recent + max_features)", W, n, s->U.L);
  return VO_ERR_CAPACITY;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_point_upkeep(vo_kfstore *s, int max_recent) {
  const char *W = "vo_kfstore_enable_point_upkeep";
  if (const int rc = enable_begin(s, W, kLayerLocalBa, kLayerUpkeep, max_recent >= 1)) return rc < 0 ? rc : VO_OK;
  VO_CHECK(s->up.reserve(upkeep_bytes(max_recent, s->NK)));
  s->U = upkeep_layout(s->up.p, max_recent, s->NK);
  VO_CHECK(s->up_stage.reserve((size_t)s->U.L * 12));
  VO_CHECK(connections_reserve(s->conn, 1, nullptr));  // process_new_keyframe's update of one key-frame allocates nothing
  VO_CHECK(upkeep_init(s->U, s->st));
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerUpkeep;
  return VO_OK;
}

int vo_kfstore_compute_descriptors_dev(vo_kfstore *s, int n, const int32_t *dev_ids) {
  const char *W = "vo_kfstore_compute_descriptors_dev";
  VO_CHECK(need(s, W, kLayerUpkeep));
  if (n < 0 || (n > 0 && !dev_ids)) return VO_ERR_INVALID;
  VO_CHECK(up_list_fits(s, W, n));
  if (n == 0) return VO_OK;
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  s->gen++;  // (flags and ids stay: the index does not go stale)
  return upkeep_descriptors_enqueue(kfstore_view(s), O, s->U, connections_view(s->conn).status, n, dev_ids, s->st);
}

int vo_kfstore_compute_descriptors(vo_kfstore *s, int n, const int32_t *ids) {
  const char *W = "vo_kfstore_compute_descriptors";
  VO_CHECK(need(s, W, kLayerUpkeep));
  if (n < 0 || (n > 0 && !ids)) return VO_ERR_INVALID;
  VO_CHECK(up_list_fits(s, W, n));
  for (int i = 0; i < n; i++)
    if (ids[i] < 0) {
      set_error("%s: entry %d: id %d is negative", W, i, ids[i]);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  memcpy(s->up_stage.data(), ids, (size_t)n * 4);
  VO_CHECK(copy_h2d(s->U.list, s->up_stage.data(), (size_t)n * 4, s->st, W));
  VO_CHECK(vo_kfstore_compute_descriptors_dev(s, n, s->U.list));
  return stream_sync(s->st, W);
}

int vo_kfstore_process_new_keyframe(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_process_new_keyframe";
  VO_CHECK(need(s, W, kLayerUpkeep));
  VO_CHECK(need_keyframe(s, W, current));
  // (that `current` has been erased only the device knows: nothing is then listed, and the sticky INVALID is raised)
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  const KfStoreView V = kfstore_view(s);
  VO_CHECK(upkeep_process_enqueue(V, O, s->X, s->M, s->B, s->U, s->normals.as<double>(), connections_view(s->conn).status, current, s->st));
  s->gen++;  // (flags and ids stay: the index does not go stale)
  return connections_update(s->conn, V, O, 1, s->U.head + 2, s->st);  // keyframe_curr_->updateConnections() (:128)
}

int vo_kfstore_add_point_stats_dev(vo_kfstore *s, int n, const int32_t *dev_ids, const int32_t *dev_visible, const int32_t *dev_found) {
  const char *W = "vo_kfstore_add_point_stats_dev";
  VO_CHECK(need(s, W, kLayerUpkeep));
  if (n < 0 || (n > 0 && (!dev_ids || !dev_visible || !dev_found))) return VO_ERR_INVALID;
  s->gen++;
  return upkeep_stats_enqueue(s->U, n, dev_ids, dev_visible, dev_found, s->st);
}

int vo_kfstore_add_point_stats(vo_kfstore *s, int n, const int32_t *ids, const int32_t *visible, const int32_t *found) {
  const char *W = "vo_kfstore_add_point_stats";
  VO_CHECK(need(s, W, kLayerUpkeep));
  if (n < 0 || (n > 0 && (!ids || !visible || !found))) return VO_ERR_INVALID;
  VO_CHECK(up_list_fits(s, W, n));
  for (int i = 0; i < n; i++)
    if (visible[i] < 0 || found[i] < 0) {
      set_error("%s: entry %d: a negative increment (%d visible, %d found)", W, i, visible[i], found[i]);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  // staged as the block's list holds them: ids | visible | found, L entries each; one copy
  const size_t L = (size_t)s->U.L;
  int32_t *h = reinterpret_cast<int32_t *>(s->up_stage.data());
  memset(h, 0xff, L * 4), memset(h + L, 0, L * 8);  // (beyond n: no id, no increment)
  memcpy(h, ids, (size_t)n * 4), memcpy(h + L, visible, (size_t)n * 4), memcpy(h + 2 * L, found, (size_t)n * 4);
  VO_CHECK(copy_h2d(s->U.list, h, L * 12, s->st, W));
  VO_CHECK(vo_kfstore_add_point_stats_dev(s, n, s->U.list, s->U.list + L, s->U.list + 2 * L));
  return stream_sync(s->st, W);
}

int vo_kfstore_cull_map_points(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_cull_map_points";
  VO_CHECK(need(s, W, kLayerUpkeep));
  VO_CHECK(need_keyframe(s, W, current));
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  VO_CHECK(upkeep_cull_enqueue(kfstore_view(s), O, s->X, s->U, current, s->st));
  s->obs_dirty = true, s->gen++;  // (whether anything was erased only the device knows)
  return VO_OK;
}

int vo_kfstore_recent_points(vo_kfstore *s, int32_t *n, int32_t *ids, int32_t *first_kf, int32_t *found, int32_t *visible) {
  const char *W = "vo_kfstore_recent_points";
  VO_CHECK(need(s, W, kLayerUpkeep));
  const size_t R = (size_t)s->U.R;
  std::vector<int32_t> h(4 * R + 4);
  VO_CHECK(copy_d2h(h.data(), s->U.head, 16, s->st, W));
  const int32_t *cols[4] = {s->U.id, s->U.first_kf, s->U.found, s->U.visible};
  for (int c = 0; c < 4; c++) VO_CHECK(copy_d2h(h.data() + 4 + c * R, cols[c], R * 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
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
  VO_CHECK(need(s, W, kLayerUpkeep));
  int32_t rec[kUpRecInts];
  std::vector<int32_t> er((size_t)s->U.R);
  VO_CHECK(copy_d2h(rec, s->U.rec, sizeof(rec), s->st, W));
  if (erased_ids) VO_CHECK(copy_d2h(er.data(), s->U.erased, er.size() * 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  if (record) memcpy(record, rec, sizeof(rec));
  if (erased_ids) {
    const int ne = rec[kUpKind] == VO_KFSTORE_UPKEEP_CULL ? std::min(std::max(rec[kUpNErased], 0), s->U.R) : 0;
    std::sort(er.begin(), er.begin() + ne);
    memcpy(erased_ids, er.data(), (size_t)ne * 4);
  }
  return VO_OK;
}

}  // extern "C"
