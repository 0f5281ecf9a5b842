// loop_sim3.hip -- LoopClosing::computeSim3 (reference src/loopClosing.cpp:178-348) from the key-frame store, walked on the
// device.  The front (searchByBoW over all candidates, match.hip: loop_bow_replay) and the solvers'
// construction are independent of the walk; the walk itself is sequential in the reference -- its order depends on rand() and
// on early returns -- and is sequenced here by one workgroup per step, with the state in device memory between launches:
//   k_loop_begin      the state reset; `current` erased or without a pose: no walk, the sticky VO_KFSTORE_CONNECTIONS_INVALID
//   k_loop_construct  a workgroup per candidate: the discards of :210-222 and Sim3Solver's constructor (sim3Solver.cpp:8-96),
//                     the correspondences compacted in feature order
//   k_loop_walk       ONE workgroup of five wavefronts: the while / for of :236-288 up to the next non-empty iterate().  The
//                     up-to-five trips of an iterate call are evaluated speculatively, a wavefront each (Horn's closed form and
//                     the inlier test of sim3_horn.h), and committed in order by one thread: best count, the > 20 return, the
//                     rand() values consumed.  A return hands inlierMappoints and Scm to the verification.
//   k_loop_search     searchBySim3's two directions (matcher.cpp:715-846), a wavefront per projected map point, the window
//                     read as fuse.hip reads it (kf_area.h)
//   k_loop_gather     the mutual test (:848-861), solveLoopSim3's inputs (optimizer_ceres.cpp:846-881) compacted in feature order
//   (k_sim3, sim3.hip: sim3_solve_dev -- the refinement itself, on the arrays k_loop_gather left)
//   k_loop_verified   the outliers nulled, Scm taken over, the >= 20 decision (:274-285), Scw = Scm * Smw
//   k_loop_mark / k_loop_collect   loopConnectKFMapPoints_ (:298-319): first occurrences by an atomic minimum per id, then an
//                     ordered compaction by one workgroup
//   k_loop_project    searchByProjection (matcher.cpp:356-447): the gates of every loop point in parallel, then the claims in
//                     list order by one workgroup (they depend on one another through matchMapPoints and the :422 index quirk),
//                     and the >= 40 decision (:331)
// Every kernel behind k_loop_construct starts by reading the phase word and returns at once when the step is not due, so
// rounds can be enqueued without knowing how many the walk needs.  No kernel waits on another workgroup; every loop is
// bounded by a count clamped to its array.  Compiled with -ffp-contract=off.
#include "kfstore.h"

#include "ba_math.h"
#include "kf_area.h"
#include "new_points_geom.h"
#include "obs_walk.h"
#include "sim3_horn.h"

#include <cmath>
#include <vector>

namespace {

using namespace vo;

constexpr int kThLow = 50, kThHigh = 100;    // matcher.cpp:11-12
constexpr int kRansacMinInliers = 20, kRansacMaxIterations = 300, kIterateTrips = kLoopTrips;  // loopClosing.cpp:227, :251
constexpr int kWalkThreads = 64 * kLoopTrips;

__device__ __forceinline__ int n_features(const KfStoreView &S, int k) { return min(max(kf_head(S, k)[0], 0), S.NK); }
__device__ __forceinline__ bool kf_usable(const LoopArgs &A, int k) { return k >= 0 && k < A.S.size && !A.X.erased[k]; }

// the OBSERVATION in key-frame k of the id its feature f carries: k's lowest-numbered feature with that id
// and bit 0; -1 when feature f has no point, a negative id or no entry in the index
__device__ int observation_of(const LoopArgs &A, int k, int f) {
  const KfStoreView &S = A.S;
  if (!(kf_sec<uint8_t>(S, k, S.o_flags)[f] & 1)) return -1;
  const int id = kf_sec<int>(S, k, S.o_ids)[f];
  if (id < 0) return -1;
  const unsigned e = (unsigned)k * (unsigned)S.NK + (unsigned)f;
  if ((long long)e >= (long long)A.O.n_keys) return -1;
  const int start = A.O.run[e];
  if (start < 0 || start >= A.O.n_keys || (int)(A.O.keys[start] >> 32) != id) return -1;
  int found = -1;
  obs_run_each(A.O, start, id, [&](unsigned en) {
    const int kk = (int)(en / (unsigned)S.NK);
    if (kk == k) found = (int)(en - (unsigned)kk * (unsigned)S.NK);
    return kk < k;  // entries ascend: the first of k is its lowest feature
  });
  return found;
}

// Tcw * p (SE3 on a point) in the operation order of new_points_geom.h
__device__ __forceinline__ void se3_point(const double *T, const double *p, double out[3]) {
  for (int r = 0; r < 3; r++) out[r] = __dadd_rn(np_dot3(T[3 * r], p[0], T[3 * r + 1], p[1], T[3 * r + 2], p[2]), T[9 + r]);
}
// s R p + t for a Sim3 laid out as R (9) t (3) s
__device__ __forceinline__ void sim3_point(const double *Sm, const double *p, double out[3]) {
  for (int r = 0; r < 3; r++)
    out[r] = __dadd_rn(__dmul_rn(Sm[12], np_dot3(Sm[3 * r], p[0], Sm[3 * r + 1], p[1], Sm[3 * r + 2], p[2])), Sm[9 + r]);
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}

// the exclusive position of `keep` among the workgroup's threads in thread order, and their number (<= 1024 threads)
__device__ __forceinline__ int block_rank(bool keep, int *s_wave /*[16]*/, int &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  const unsigned long long mk = __builtin_amdgcn_ballot_w64(keep);
  const int within = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
  __syncthreads();
  if (lane == 0) s_wave[w] = (int)__popcll(mk);
  __syncthreads();
  int before = 0, all = 0;
  for (int i = 0; i < nw; i++) {
    const int c = s_wave[i];
    if (i < w) before += c;
    all += c;
  }
  total = all;
  return before + within;
}

// ---- a new call
__device__ void loop_begin(const LoopArgs &A, int current, int n_cand, int fix_scale, int n_rand, int rand_max) {
  int *st = A.L.st;
  for (int i = 0; i < kLoopStateInts; i++) st[i] = 0;
  st[kLsMatchPos] = st[kLsMatchKf] = -1;
  st[kLsCurrent] = current, st[kLsNCand] = n_cand, st[kLsFixScale] = fix_scale, st[kLsNRand] = n_rand, st[kLsRandMax] = rand_max;
  st[kLsLive] = -1, st[kLsPending] = -1;
  const bool ok = kf_usable(A, current) && *np_pose_set(A.M, current) != 0;
  st[kLsNCur] = ok ? n_features(A.S, current) : 0;
  st[kLsPhase] = ok ? kLoopWalk : kLoopHalt;
  if (!ok) atomicOr(A.status, VO_KFSTORE_CONNECTIONS_INVALID);
  A.L.off[0] = A.L.off[1] = 0;
  for (int i = 0; i < VO_KFSTORE_LOOP_MAX_CANDIDATES * kLoopPerInts; i++) A.L.per[i] = 0;
  for (int i = 0; i < 13; i++) A.L.Scm[i] = A.L.Scw[i] = 0.0;
}
__global__ void k_loop_begin(LoopArgs A, int current, int n_cand, int fix_scale, int n_rand, int rand_max) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  loop_begin(A, current, n_cand, fix_scale, n_rand, rand_max);
}

// k_loop_begin for a list and a count only the device knows (kfstore.h: loop_compute_counted): the candidates copied into the
// block (-1 beyond the count, as the host form's copy leaves them), their erase locks set (loopClosing.cpp:208), the count
// written.  No list or too long a list: the state of a call that found nothing, and no walk.
__global__ void k_loop_begin_counted(LoopArgs A, int current, const int *go, int go_value, const int *n_src, const int *src, int fix_scale,
                                     int n_rand, int rand_max, int quiet) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool has = go[0] == go_value;
  int n = has ? max(n_src[0], 0) : 0;
  const bool fits = n <= A.L.C;
  if (!fits) n = 0;
  for (int c = 0; c < VO_KFSTORE_LOOP_MAX_CANDIDATES; c++) A.L.cand[c] = c < n ? src[c] : -1;
  loop_begin(A, current, n, fix_scale, n_rand, rand_max);
  if (n == 0) {
    A.L.st[kLsState] = VO_KFSTORE_LOOP_NO_MATCH, A.L.st[kLsPhase] = kLoopDone;
    if (!fits) atomicOr(A.status, VO_KFSTORE_LOOP_CAPACITY);
    else if (!quiet) atomicOr(A.status, VO_KFSTORE_CONNECTIONS_INVALID);
  }
  for (int c = 0; c < n; c++) {
    const int kf = A.L.cand[c];
    if (kf >= 0 && kf < A.S.size) A.X.locked[kf] = 1;
  }
}

// behind k_loop_construct in the counted form: the front ran for max_candidates; the rows beyond the count go back to what
// k_loop_begin left (the walk reads none of them)
__global__ void k_loop_trim(LoopArgs A) {
  const int c = threadIdx.x;
  if (c >= VO_KFSTORE_LOOP_MAX_CANDIDATES || c < min(max(A.L.st[kLsNCand], 0), A.L.C)) return;
  for (int i = 0; i < kLoopPerInts; i++) A.L.per[c * kLoopPerInts + i] = 0;
}

// ---- the discards (:210-222) and Sim3Solver's constructor (sim3Solver.cpp:8-96)
__global__ __launch_bounds__(256) void k_loop_construct(LoopArgs A) {
  __shared__ int s_wave[16];
  const KfLoopView &L = A.L;
  const KfStoreView &S = A.S;
  const int c = blockIdx.x, tid = threadIdx.x, NK = S.NK;
  const int kf = L.cand[c], cur = L.st[kLsCurrent];
  int *per = L.per + c * kLoopPerInts;
  if (L.st[kLsPhase] == kLoopHalt) {
    if (tid == 0) per[kLpKf] = kf;
    return;
  }
  const bool bad = !kf_usable(A, kf) || kf_head(S, kf)[1] != 0;  // :210
  const int nm = bad ? 0 : L.nm[c];
  if (bad || nm < kRansacMinInliers) {  // :218
    if (tid == 0) per[kLpKf] = kf, per[kLpReason] = bad ? 1 : 2, per[kLpBow] = nm;
    return;
  }
  const int nA = n_features(S, cur), nB = n_features(S, kf);
  const int *match = L.match12 + (size_t)c * NK;
  const double *T1 = np_pose(A.M, cur), *T2 = np_pose(A.M, kf);
  const bool pose2 = *np_pose_set(A.M, kf) != 0;  // (a candidate without a pose keeps no correspondence: the solver stops)
  const double fx = (double)A.M.cam[0], fy = (double)A.M.cam[1], cx = (double)A.M.cam[2], cy = (double)A.M.cam[3];
  double *pc1 = L.pc1 + (size_t)c * NK * 3, *pc2 = L.pc2 + (size_t)c * NK * 3, *px1 = L.px1 + (size_t)c * NK * 2, *px2 = L.px2 + (size_t)c * NK * 2;
  int *me1 = L.me1 + (size_t)c * NK, *me2 = L.me2 + (size_t)c * NK, *midx = L.midx + (size_t)c * NK;
  int N = 0;
  for (int base = 0; base < nA; base += 256) {  // (uniform trip count)
    const int i = base + tid;
    int i2 = -1, idx1 = -1, idx2 = -1;
    if (i < nA && pose2) {
      i2 = match[i];
      if (i2 >= 0 && i2 < nB) idx1 = observation_of(A, cur, i), idx2 = observation_of(A, kf, i2);  // :42-46
    }
    const bool keep = idx1 >= 0 && idx2 >= 0;
    int total;
    const int k = N + block_rank(keep, s_wave, total);
    if (keep) {
      const float s1 = A.M.sf[min(max(cull_octave(A.X, cur)[idx1], 0), 15)], s2 = A.M.sf[min(max(cull_octave(A.X, kf)[idx2], 0), 15)];
      me1[k] = (int)(9.210 * (double)s1 * (double)s1), me2[k] = (int)(9.210 * (double)s2 * (double)s2);  // :53-54
      midx[k] = i;
      double a[3], b[3];
      se3_point(T1, kf_sec<double>(S, cur, S.o_points) + 3 * (size_t)i, a);
      se3_point(T2, kf_sec<double>(S, kf, S.o_points) + 3 * (size_t)i2, b);
      for (int r = 0; r < 3; r++) pc1[3 * k + r] = a[r], pc2[3 * k + r] = b[r];
      px1[2 * k] = __dadd_rn(__ddiv_rn(__dmul_rn(fx, a[0]), a[2]), cx), px1[2 * k + 1] = __dadd_rn(__ddiv_rn(__dmul_rn(fy, a[1]), a[2]), cy);
      px2[2 * k] = __dadd_rn(__ddiv_rn(__dmul_rn(fx, b[0]), b[2]), cx), px2[2 * k + 1] = __dadd_rn(__ddiv_rn(__dmul_rn(fy, b[1]), b[2]), cy);
    }
    N += total;
  }
  if (tid == 0) {
    per[kLpKf] = kf, per[kLpReason] = 0, per[kLpBow] = nm, per[kLpN] = N;
    per[kLpMaxIters] = L.iters[min(max(N, 0), NK)];
    per[kLpIters] = per[kLpBest] = per[kLpVerifs] = 0;
  }
}

// randomInt's draws over the shrinking identity list (sim3Solver.cpp:125-141): what position `pos` holds after the swaps
__device__ __forceinline__ int list_at(int pos, int n_swaps, const int *sw_pos, const int *sw_val) {
  int v = pos;
  for (int k = 0; k < n_swaps; k++)
    if (sw_pos[k] == pos) v = sw_val[k];
  return v;
}
__device__ __forceinline__ void draw_triplet(const int *r, int rand_max, int N, int idx[3]) {
  int sw_pos[3], sw_val[3];
  for (int k = 0; k < 3; k++) {
    const int size = N - k;
    int ri = (int)(((double)r[k] / ((double)rand_max + 1.0)) * (double)size);
    ri = min(max(ri, 0), size - 1);  // (a value outside [0, rand_max] cannot index outside the list)
    idx[k] = list_at(ri, k, sw_pos, sw_val);
    sw_pos[k] = ri, sw_val[k] = list_at(size - 1, k, sw_pos, sw_val);  // availableIdxs[randi] = availableIdxs.back(); pop_back()
  }
}

// ---- the walk (:236-288) to the next non-empty iterate() or to its end
__global__ __launch_bounds__(kWalkThreads) void k_loop_walk(LoopArgs A) {
  __shared__ double sT[kIterateTrips][26];
  __shared__ int s_cnt[kIterateTrips];
  __shared__ int s_i, s_live, s_used, s_action, s_c, s_trips, s_ret;
  enum { kEnd = 0, kAgain, kTrips, kVerify, kHalt };
  const KfLoopView &L = A.L;
  int *st = L.st;
  if (st[kLsPhase] != kLoopWalk) return;  // (uniform: the predecessor decided, or halted)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, NK = A.S.NK;
  const int n_cand = min(max(st[kLsNCand], 0), L.C), n_rand = min(max(st[kLsNRand], 0), L.max_rand), rand_max = st[kLsRandMax];
  const int fix_scale = st[kLsFixScale];
  const float fx = A.M.cam[0], fy = A.M.cam[1], cx = A.M.cam[2], cy = A.M.cam[3];
  if (tid == 0) {
    int live = st[kLsLive];
    if (live < 0) {  // the first round: `candidates` of :204-232
      live = 0;
      for (int c = 0; c < n_cand; c++) live += L.per[c * kLoopPerInts + kLpReason] == 0;
    }
    s_i = st[kLsCursor], s_live = live, s_used = st[kLsRandUsed];
    st[kLsRounds]++;
  }
  __syncthreads();
  // (every trip of the loop retires a candidate, commits at least one trip, or leaves: at most n_cand * 301 trips)
  int act = kEnd;  // (s_action read once behind each barrier: thread 0 rewrites it at the top of the next trip)
  for (int guard = 0; guard < VO_KFSTORE_LOOP_MAX_CANDIDATES * (kRansacMaxIterations + 2); guard++) {
    __syncthreads();
    if (tid == 0) {
      int action = kEnd;
      if (s_live > 0) {
        int i = s_i;
        for (int k = 0; k <= n_cand; k++, i++) {  // the for of :238 behind the while of :236
          if (i >= n_cand) i = 0;
          if (L.per[i * kLoopPerInts + kLpReason] == 0) break;
        }
        int *per = L.per + i * kLoopPerInts;
        s_c = i;
        const int N = per[kLpN], left = per[kLpMaxIters] - per[kLpIters];
        if (N < kRansacMinInliers || left <= 0) {  // sim3Solver.cpp:106-112, :171-172: stopFlag without a trip
          per[kLpReason] = 3, s_live--, s_i = i + 1, action = kAgain;
        } else {
          s_trips = min(min(kIterateTrips, left), (n_rand - s_used) / 3);  // (what the values left allow; 0: short at once)
          action = kTrips;
        }
      }
      s_action = action;
    }
    __syncthreads();
    act = s_action;
    if (act == kEnd) break;
    if (act == kAgain) continue;
    const int c = s_c, trips = s_trips;
    const int N = min(max(L.per[c * kLoopPerInts + kLpN], 0), NK);
    const double *pc1 = L.pc1 + (size_t)c * NK * 3, *pc2 = L.pc2 + (size_t)c * NK * 3, *px1 = L.px1 + (size_t)c * NK * 2, *px2 = L.px2 + (size_t)c * NK * 2;
    const int *me1 = L.me1 + (size_t)c * NK, *me2 = L.me2 + (size_t)c * NK;
    if (w < trips) {  // trip w of this iterate call, speculatively: its three values are rand[used + 3 w ..] whatever the others do
      int idx[3];
      draw_triplet(L.rand + s_used + 3 * w, rand_max, N, idx);
      double *T = sT[w];
      if (lane == 0) {
        double P1[9], P2[9], R[9], t[3], s;
        for (int i = 0; i < 3; i++)
          for (int a = 0; a < 3; a++) P1[3 * i + a] = pc1[3 * idx[i] + a], P2[3 * i + a] = pc2[3 * idx[i] + a];
        sim3_horn(P1, P2, fix_scale, R, t, s);
        sim3_with_inverse(R, t, s, T);
      }
      __threadfence_block();
      __builtin_amdgcn_wave_barrier();
      uint8_t *fl = L.tflags + (size_t)w * NK;
      int local = 0;
      for (int i = lane; i < N; i += 64) {
        const bool in = sim3_inlier(T, pc1 + 3 * i, pc2 + 3 * i, px1 + 2 * i, px2 + 2 * i, me1[i], me2[i], fx, fy, cx, cy);
        fl[i] = in ? 1 : 0;
        local += in;
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) local += __shfl_xor(local, o);
      if (lane == 0) s_cnt[w] = local;
    }
    __syncthreads();
    __syncthreads();
    if (tid == 0) {  // the commits, in order (sim3Solver.cpp:120-169)
      int *per = L.per + c * kLoopPerInts;
      const int wanted = min(kIterateTrips, per[kLpMaxIters] - per[kLpIters]);
      int action = kAgain, ret = -1;
      for (int t = 0; t < trips && ret < 0; t++) {
        per[kLpIters]++, s_used += 3;
        if (s_cnt[t] >= per[kLpBest]) {
          per[kLpBest] = s_cnt[t];
          if (s_cnt[t] > kRansacMinInliers) ret = t;
        }
      }
      if (ret >= 0) {
        s_ret = ret, s_i = c + 1, action = kVerify;
      } else if (trips < wanted) {  // the next trip would draw past the caller's values
        action = kHalt;
      } else {
        if (per[kLpIters] >= per[kLpMaxIters]) per[kLpReason] = 3, s_live--;  // :171-172, loopClosing.cpp:253-257
        s_i = c + 1;
      }
      s_action = action;
    }
    __syncthreads();
    act = s_action;
    if (act == kAgain) continue;
    if (act == kHalt) break;
    // a non-empty return: inlierMappoints (:261-267) and matched2 (matcher.cpp:699-710)
    const int kf = L.cand[c], nA = min(max(st[kLsNCur], 0), NK), nB = n_features(A.S, kf);
    const int *match = L.match12 + (size_t)c * NK, *midx = L.midx + (size_t)c * NK;
    const uint8_t *fl = L.tflags + (size_t)s_ret * NK;
    for (int i = tid; i < nA; i += kWalkThreads) L.inl[i] = -1;
    for (int j = tid; j < nB; j += kWalkThreads) L.m2on[j] = 0;
    __threadfence_block();
    __syncthreads();
    for (int k = tid; k < N; k += kWalkThreads)
      if (fl[k]) {
        const int i = min(max(midx[k], 0), nA - 1), i2 = match[i];
        L.inl[i] = i2;
        const int o2 = i2 >= 0 && i2 < nB ? observation_of(A, kf, i2) : -1;
        if (o2 >= 0 && o2 < nB) L.m2on[o2] = 1;
      }
    if (tid < 13) L.Scm[tid] = sT[s_ret][tid];
    break;
  }
  __syncthreads();
  if (tid == 0) {
    st[kLsCursor] = s_i, st[kLsLive] = s_live, st[kLsRandUsed] = s_used;
    if (act == kEnd) {
      st[kLsState] = 1, st[kLsPhase] = kLoopDone;  // :290-296
    } else if (act == kHalt) {
      st[kLsPhase] = kLoopHalt;
      atomicOr(A.status, VO_KFSTORE_LOOP_RAND_SHORT);
    } else if (act == kVerify) {
      st[kLsPending] = s_c, st[kLsPhase] = kLoopVerify;
    }  // (the guard ran out: cannot happen; the phase stays and the next round goes on)
  }
}

// ---- searchBySim3 (matcher.cpp:715-846): the best feature of the other key-frame per projected map point
__global__ __launch_bounds__(256) void k_loop_search(LoopArgs A) {
  const KfLoopView &L = A.L;
  const KfStoreView &S = A.S;
  if (L.st[kLsPhase] != kLoopVerify) return;
  const int lane = threadIdx.x & 63;
  const int c = min(max(L.st[kLsPending], 0), L.C - 1), cur = L.st[kLsCurrent], kf = L.cand[c];
  const int n1 = n_features(S, cur), n2 = n_features(S, kf);
  const float fx = A.M.cam[0], fy = A.M.cam[1], cx = A.M.cam[2], cy = A.M.cam[3];
  const int n_levels = min(max(A.M.n_levels, 1), 16);
  const float log_sf1 = (float)log((double)A.M.sf[1]);
  double S12[13], S21[26];
  for (int a = 0; a < 13; a++) S12[a] = L.Scm[a];
  sim3_with_inverse(S12, S12 + 9, S12[12], S21);  // S21 = S12.inverse() (:697) at S21 + 13
  for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < n1 + n2; q += (int)gridDim.x * 4) {  // (uniform over the wavefront)
    const bool first = q < n1;  // a point of `current` into the candidate, else the reverse
    const int i = first ? q : q - n1, src = first ? cur : kf, dst = first ? kf : cur, nT = first ? n2 : n1;
    int *out = (first ? L.m1 : L.m2) + i;
    if (lane == 0) *out = -1;
    if (!(kf_sec<uint8_t>(S, src, S.o_flags)[i] & 1)) continue;  // :718, :786
    if (first ? L.inl[i] >= 0 : L.m2on[i] != 0) continue;
    double pa[3], pb[3];
    se3_point(np_pose(A.M, src), kf_sec<double>(S, src, S.o_points) + 3 * (size_t)i, pa);
    sim3_point(first ? S21 + 13 : S12, pa, pb);
    const float z = (float)pb[2];
    if (first ? z < 0.0f : z <= 0.0f) continue;  // :729, :794 as written
    const float invz = __fdiv_rn(1.0f, z);
    const float xn = __fmul_rn((float)pb[0], invz), yn = __fmul_rn((float)pb[1], invz);
    const float u = __fadd_rn(__fmul_rn(fx, xn), cx), v = __fadd_rn(__fmul_rn(fy, yn), cy);
    if (!(u >= A.F.xmin && v >= A.F.ymin && u < A.F.xmax && v < A.F.ymax)) continue;
    const float maxd = kf_sec<float>(S, src, S.o_maxd)[i], mind = kf_sec<float>(S, src, S.o_mind)[i];
    const float dist = (float)__dsqrt_rn(np_dot3(pb[0], pb[0], pb[1], pb[1], pb[2], pb[2]));
    if (dist < __fmul_rn(0.8f, mind) || dist > __fmul_rn(1.2f, maxd)) continue;
    const int level = predict_level(maxd, dist, log_sf1, n_levels);
    const float radius = __fmul_rn(7.5f, A.M.sf[level]);  // (loopClosing.cpp:269)
    const AreaWindow W = area_window(A.F, u, v, radius);
    if (!W.any) continue;
    const uint4 *qd = kf_sec<uint4>(S, src, S.o_pdesc) + 2 * (size_t)i;
    const uint4 qa = qd[0], qb = qd[1];
    const float *tx = np_x(A.M, dst), *ty = np_y(A.M, dst);
    const int *toc = cull_octave(A.X, dst);
    unsigned long long best = ~0ull;
    for (int f = lane; f < nT; f += 64) {
      int gx, gy;
      if (!area_holds(A.F, W, tx[f], ty[f], u, v, radius, gx, gy)) continue;
      const int oct = toc[f];
      if (oct < level - 1 || oct > level) continue;
      const uint4 *dd = kf_sec<uint4>(S, dst, S.o_desc) + 2 * (size_t)f;
      const unsigned long long key = area_key(hamming256(qa, qb, dd[0], dd[1]), gx, gy, f);
      best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    if (best != ~0ull && (int)(best >> 44) <= kThHigh && lane == 0) *out = (int)(best & 0xffffffffu);
  }
}

// ---- the mutual test (:848-861) and solveLoopSim3's inputs (optimizer_ceres.cpp:815-881)
__global__ __launch_bounds__(256) void k_loop_gather(LoopArgs A) {
  __shared__ int s_wave[16];
  const KfLoopView &L = A.L;
  const KfStoreView &S = A.S;
  if (L.st[kLsPhase] != kLoopVerify) return;
  const int tid = threadIdx.x;
  const int c = min(max(L.st[kLsPending], 0), L.C - 1), cur = L.st[kLsCurrent], kf = L.cand[c];
  const int n1 = n_features(S, cur), n2 = n_features(S, kf);
  for (int i = tid; i < n1; i += 256) {
    const int i2 = L.m1[i];
    if (i2 >= 0 && i2 < n2 && L.m2[i2] == i) L.inl[i] = i2;  // (inl[i] was null: matched1 kept feature i out otherwise)
  }
  __threadfence_block();
  __syncthreads();
  const double *Tc = np_pose(A.M, cur), *Tm = np_pose(A.M, kf);
  int n = 0;
  for (int base = 0; base < n1; base += 256) {
    const int i = base + tid;
    int i2 = -1, im = -1;
    if (i < n1) {
      i2 = L.inl[i];
      if (i2 >= 0 && i2 < n2 && (kf_sec<uint8_t>(S, cur, S.o_flags)[i] & 1)) im = observation_of(A, kf, i2);  // :849-859
    }
    const bool keep = im >= 0 && im < n2;
    int total;
    const int k = n + block_rank(keep, s_wave, total);
    if (keep) {
      double pm[3], pc[3];
      se3_point(Tm, kf_sec<double>(S, kf, S.o_points) + 3 * (size_t)i2, pm);
      se3_point(Tc, kf_sec<double>(S, cur, S.o_points) + 3 * (size_t)i, pc);
      for (int r = 0; r < 3; r++) L.Pm[3 * k + r] = pm[r], L.Pc[3 * k + r] = pc[r];
      L.pxm[2 * k] = (double)np_x(A.M, kf)[im], L.pxm[2 * k + 1] = (double)np_y(A.M, kf)[im];
      L.pxc[2 * k] = (double)np_x(A.M, cur)[i], L.pxc[2 * k + 1] = (double)np_y(A.M, cur)[i];  // feature i's own pixel (:871)
      L.ism[k] = 1.0 / (double)A.M.sf[min(max(cull_octave(A.X, kf)[im], 0), 15)];
      L.isc[k] = 1.0 / (double)A.M.sf[min(max(cull_octave(A.X, cur)[i], 0), 15)];
      L.sidx[k] = i;
    }
    n += total;
  }
  if (tid == 0) {
    L.off[0] = 0, L.off[1] = n;
    double xi[6];
    const double t0[3] = {0, 0, 0};
    ba::se3_log_from_R(L.Scm, t0, xi);  // the angle-axis vector of Rcm (:826)
    for (int a = 0; a < 3; a++) L.pose[a] = xi[3 + a], L.pose[3 + a] = L.Scm[9 + a];
    L.scale[0] = L.Scm[12];
  }
}

// ---- behind the refinement: the outliers nulled, Scm taken over, the decision of :274-285
__global__ __launch_bounds__(256) void k_loop_verified(LoopArgs A) {
  const KfLoopView &L = A.L;
  int *st = L.st;
  if (st[kLsPhase] != kLoopVerify) return;
  const int tid = threadIdx.x, NK = A.S.NK;
  const int n = min(max(L.off[1], 0), NK), n1 = min(max(st[kLsNCur], 0), NK);
  for (int k = tid; k < n; k += 256)
    if (L.outl[k]) L.inl[min(max(L.sidx[k], 0), n1 - 1)] = -1;
  __syncthreads();
  if (tid != 0) return;
  const int c = min(max(st[kLsPending], 0), L.C - 1), kf = L.cand[c];
  const int inliers = L.ninl[0];
  if (L.sums[0].reserved == 2) {  // both problems ran: Scm = Scm2 (optimizer_ceres.cpp:991-1027); else it is not written (:952-953)
    const double se3[6] = {0, 0, 0, L.pose[0], L.pose[1], L.pose[2]};
    const ba::PoseCache P = ba::pose_cache(se3);  // ceres::AngleAxisToRotationMatrix
    for (int a = 0; a < 9; a++) L.Scm[a] = P.R[a];
    for (int a = 0; a < 3; a++) L.Scm[9 + a] = L.pose[3 + a];
    L.Scm[12] = L.scale[0];
  }
  L.off[0] = L.off[1] = 0;
  st[kLsVerifs]++, L.per[c * kLoopPerInts + kLpVerifs]++;
  st[kLsRefine] = inliers, st[kLsPending] = -1;
  if (inliers >= 20) {  // :274-285: Scw = Scm * Smw, Smw = (Rmw, tmw, 1)
    const double *Tm = np_pose(A.M, kf), *Sc = L.Scm;
    for (int r = 0; r < 3; r++) {
      for (int q = 0; q < 3; q++) L.Scw[3 * r + q] = np_dot3(Sc[3 * r], Tm[q], Sc[3 * r + 1], Tm[3 + q], Sc[3 * r + 2], Tm[6 + q]);
      L.Scw[9 + r] = __dadd_rn(__dmul_rn(Sc[12], np_dot3(Sc[3 * r], Tm[9], Sc[3 * r + 1], Tm[10], Sc[3 * r + 2], Tm[11])), Sc[9 + r]);
    }
    L.Scw[12] = Sc[12];
    st[kLsMatchPos] = c, st[kLsMatchKf] = kf, st[kLsPhase] = kLoopAfter;
  } else if (st[kLsLive] <= 0) {
    st[kLsState] = 1, st[kLsPhase] = kLoopDone;  // the while of :236 ends: no candidate is left
  } else {
    st[kLsPhase] = kLoopWalk;  // the for of :238 goes on behind candidate c
  }
}

// ---- loopConnectKFMapPoints_ (:298-319).  List position g = (place in [ordered list of match ..., match]) * NK + feature.
__device__ __forceinline__ int loop_list_kf(const LoopArgs &A, int mk, int n_ord, int place) {
  return place < n_ord ? A.C.ordered[(size_t)mk * A.C.max_kf + place] : mk;
}
__device__ __forceinline__ int loop_n_ordered(const LoopArgs &A, int mk) { return min(max(A.C.n_ordered[mk], 0), A.C.max_kf); }
// the start of the run of the id feature f of key-frame k carries (bit 0 set), or -1
__device__ __forceinline__ int slot_of_feature(const LoopArgs &A, int k, int f) {
  if (!kf_usable(A, k) || f >= n_features(A.S, k) || !(kf_sec<uint8_t>(A.S, k, A.S.o_flags)[f] & 1)) return -1;
  const int id = kf_sec<int>(A.S, k, A.S.o_ids)[f];
  const unsigned e = (unsigned)k * (unsigned)A.S.NK + (unsigned)f;
  if (id < 0 || (long long)e >= (long long)A.O.n_keys) return -1;
  const int p = A.O.run[e];
  return p >= 0 && p < A.O.n_keys && p < A.L.n_slots && (int)(A.O.keys[p] >> 32) == id ? p : -1;
}

__global__ __launch_bounds__(256) void k_loop_mark(LoopArgs A) {
  const KfLoopView &L = A.L;
  if (L.st[kLsPhase] != kLoopAfter) return;
  const int NK = A.S.NK, mk = L.st[kLsMatchKf], cur = L.st[kLsCurrent];
  if (!kf_usable(A, mk)) return;
  const int n_ord = loop_n_ordered(A, mk);
  const long long total = (long long)(n_ord + 1) * NK;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const int place = (int)(g / NK), f = (int)(g - (long long)place * NK);
    const int p = slot_of_feature(A, loop_list_kf(A, mk, n_ord, place), f);
    if (p >= 0) atomicMin(L.mark + p, (unsigned)g);
  }
  // matchMapPoints_ on entry = inlierMappoints (:283): their ids are searchByProjection's alreadyFound (matcher.cpp:370-371)
  const int n1 = n_features(A.S, cur), c = min(max(L.st[kLsMatchPos], 0), L.C - 1), kf = L.cand[c];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n1; i += (int)gridDim.x * 256) {
    const int i2 = L.inl[i];
    const int p = i2 >= 0 ? slot_of_feature(A, kf, i2) : -1;
    if (p >= 0) L.fnd[p] = 1;
    L.match_ids[i] = p >= 0 ? kf_sec<int>(A.S, kf, A.S.o_ids)[i2] : -1;
  }
}

__global__ __launch_bounds__(1024) void k_loop_collect(LoopArgs A) {
  __shared__ int s_wave[16];
  const KfLoopView &L = A.L;
  int *st = L.st;
  if (st[kLsPhase] != kLoopAfter) return;
  const int NK = A.S.NK, mk = st[kLsMatchKf], tid = threadIdx.x;
  const int n_ord = kf_usable(A, mk) ? loop_n_ordered(A, mk) : -1;
  const long long total = (long long)(n_ord + 1) * NK;
  int n = 0;
  for (long long base = 0; base < total; base += 1024) {
    const long long g = base + tid;
    int id = -1;
    if (g < total) {
      const int place = (int)(g / NK), f = (int)(g - (long long)place * NK), k = loop_list_kf(A, mk, n_ord, place);
      const int p = slot_of_feature(A, k, f);
      if (p >= 0 && L.mark[p] == (unsigned)g) id = kf_sec<int>(A.S, k, A.S.o_ids)[f];  // the first of its id (:312-316)
    }
    int cnt;
    const int q = n + block_rank(id >= 0, s_wave, cnt);
    if (id >= 0 && q < L.P) L.loop_ids[q] = id, L.qg[q] = (int)g;
    n += cnt;
  }
  if (tid == 0) {
    st[kLsNLoop] = n;
    if (n > L.P) {
      st[kLsPhase] = kLoopHalt;
      atomicOr(A.status, VO_KFSTORE_LOOP_CAPACITY);
    }
  }
}

// ---- searchByProjection(current, Scw, loopPoints, matchMapPoints, 10) (matcher.cpp:356-447) and the decision of :331
__global__ __launch_bounds__(256) void k_loop_project(LoopArgs A) {
  extern __shared__ unsigned long long s_list[];  // [NK] the window's features in no order
  __shared__ int s_n;
  __shared__ unsigned long long s_best[4];
  const KfLoopView &L = A.L;
  const KfStoreView &S = A.S;
  int *st = L.st;
  if (st[kLsPhase] != kLoopAfter) return;
  const int NK = S.NK, tid = threadIdx.x, lane = tid & 63, cur = st[kLsCurrent], mk = st[kLsMatchKf];
  if (!kf_usable(A, mk) || !kf_usable(A, cur)) return;  // (a match is a key-frame of the store: checked before anything is indexed by it)
  const int n = min(max(st[kLsNLoop], 0), L.P), n1 = n_features(S, cur);
  const int n_ord = loop_n_ordered(A, mk);
  const float fx = A.M.cam[0], fy = A.M.cam[1], cx = A.M.cam[2], cy = A.M.cam[3];
  const int n_levels = min(max(A.M.n_levels, 1), 16);
  const float log_sf1 = (float)log((double)A.M.sf[1]);
  // Rcw = rotation / scale, tcw = translation / scale, Ow = -Rcw^T tcw (:365-368), as written
  double T[12], Ow[3];
  for (int a = 0; a < 12; a++) T[a] = __ddiv_rn(L.Scw[a], L.Scw[12]);
  np_center(T, Ow);
  // the gates, every loop point on its own
  for (int q = tid; q < n; q += 256) {
    const int g = L.qg[q], place = g / NK, f = g - place * NK, k = loop_list_kf(A, mk, n_ord, place);
    uint8_t ok = 0;
    float u = 0.f, v = 0.f;
    int level = 0;
    const int p = slot_of_feature(A, k, f);
    if (p >= 0 && !L.fnd[p]) {  // :377
      const double *pw = kf_sec<double>(S, k, S.o_points) + 3 * (size_t)f;
      double pc[3];
      se3_point(T, pw, pc);
      const float z = (float)pc[2];
      if (!(z < 0.0f)) {  // :382
        const float invz = __fdiv_rn(1.0f, z);
        const float xn = __fmul_rn((float)pc[0], invz), yn = __fmul_rn((float)pc[1], invz);
        u = __fadd_rn(__fmul_rn(fx, xn), cx), v = __fadd_rn(__fmul_rn(fy, yn), cy);
        if (u >= A.F.xmin && v >= A.F.ymin && u < A.F.xmax && v < A.F.ymax) {
          double line[3];
          for (int a = 0; a < 3; a++) line[a] = __dadd_rn(pw[a], -Ow[a]);
          const float dist = (float)__dsqrt_rn(np_dot3(line[0], line[0], line[1], line[1], line[2], line[2]));
          const float maxd = kf_sec<float>(S, k, S.o_maxd)[f], mind = kf_sec<float>(S, k, S.o_mind)[f];
          const double *pn = A.O.normals + ((size_t)k * NK + f) * 3;
          if (!(dist < __fmul_rn(0.8f, mind) || dist > __fmul_rn(1.2f, maxd)) &&
              !(np_dot3(line[0], pn[0], line[1], pn[1], line[2], pn[2]) < __dmul_rn(0.5, (double)dist))) {  // :400, :404
            level = predict_level(maxd, dist, log_sf1, n_levels);
            ok = 1;
          }
        }
      }
    }
    L.qok[q] = ok, L.qu[q] = u, L.qv[q] = v;
    L.qlv[q] = level;
  }
  __threadfence_block();
  __syncthreads();
  // the claims, in list order
  const float *tx = np_x(A.M, cur), *ty = np_y(A.M, cur);
  const int *toc = cull_octave(A.X, cur);
  for (int q = 0; q < n; q++) {
    if (!L.qok[q]) continue;  // (uniform)
    const int level = L.qlv[q], g = L.qg[q], place = g / NK, f0 = g - place * NK;
    const int k = loop_list_kf(A, mk, n_ord, place);
    const float u = L.qu[q], v = L.qv[q], radius = __fmul_rn(10.0f, A.M.sf[level]);  // (int th = 10, :408)
    const AreaWindow W = area_window(A.F, u, v, radius);
    if (!W.any) continue;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int f = tid; f < n1; f += 256) {
      int gx, gy;
      if (area_holds(A.F, W, tx[f], ty[f], u, v, radius, gx, gy)) s_list[atomicAdd(&s_n, 1)] = area_order(gx, gy, f);
    }
    __syncthreads();
    const int m = min(s_n, n1);
    const uint4 *qd = kf_sec<uint4>(S, k, S.o_pdesc) + 2 * (size_t)f0;
    const uint4 qa = qd[0], qb = qd[1];
    unsigned long long best = ~0ull;
    for (int e = tid; e < m; e += 256) {
      const unsigned long long mine = s_list[e];
      int j = 0;  // the candidate counter of :419: the features of the window visited before this one
      for (int o = 0; o < m; o++) j += s_list[o] < mine;
      if (L.match_ids[j] >= 0) continue;  // `if (matchMapPoints[j])` (:422): indexed by the counter, as written
      const int f = (int)(mine & 0xffffffffu), oct = toc[f];
      if (oct < level - 1 || oct > level) continue;
      const uint4 *dd = kf_sec<uint4>(S, cur, S.o_desc) + 2 * (size_t)f;
      const unsigned long long key = ((unsigned long long)hamming256(qa, qb, dd[0], dd[1]) << 44) | mine;
      best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    if (lane == 0) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < 4; i++) best = s_best[i] < best ? s_best[i] : best;
      if (best != ~0ull && (int)(best >> 44) <= kThLow) L.match_ids[(int)(best & 0xffffffffu)] = L.loop_ids[q];  // :439-441
      __threadfence_block();
    }
    __syncthreads();
  }
  // :324-347
  int cnt = 0;
  for (int i = tid; i < n1; i += 256) cnt += L.match_ids[i] >= 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
  __syncthreads();
  if (lane == 0) s_best[tid >> 6] = (unsigned long long)cnt;
  __syncthreads();
  if (tid == 0) {
    const int total = (int)(s_best[0] + s_best[1] + s_best[2] + s_best[3]);
    st[kLsMatchCnt] = total, st[kLsState] = total >= 40 ? 3 : 2, st[kLsPhase] = kLoopDone;
  }
}

struct Layout {
  uint8_t *block;
  size_t at = 0;
  template <class T>
  void take(T *&field, size_t count) {
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += up16(count * sizeof(T));
  }
};

void loop_lay(Layout &Y, KfLoopView &L, int NK, int C, int P, int max_rand, int n_slots) {
  const size_t nk = (size_t)NK, c = (size_t)C, p = (size_t)P, s = (size_t)n_slots;
  Y.take(L.st, kLoopStateInts), Y.take(L.cand, VO_KFSTORE_LOOP_MAX_CANDIDATES), Y.take(L.rand, (size_t)max_rand), Y.take(L.iters, nk + 1);
  Y.take(L.per, VO_KFSTORE_LOOP_MAX_CANDIDATES * kLoopPerInts);
  Y.take(L.queries, c * nk), Y.take(L.claims, c * nk), Y.take(L.args, c * tri_args_bytes()), Y.take(L.bok, c * nk);
  Y.take(L.match12, c * nk), Y.take(L.nm, c);
  Y.take(L.pc1, c * nk * 3), Y.take(L.pc2, c * nk * 3), Y.take(L.px1, c * nk * 2), Y.take(L.px2, c * nk * 2);
  Y.take(L.me1, c * nk), Y.take(L.me2, c * nk), Y.take(L.midx, c * nk);
  Y.take(L.tflags, (size_t)kLoopTrips * nk);
  Y.take(L.inl, nk), Y.take(L.m1, nk), Y.take(L.m2, nk), Y.take(L.sidx, nk), Y.take(L.off, 2), Y.take(L.ninl, 1);
  Y.take(L.m2on, nk), Y.take(L.outl, nk + 64);
  Y.take(L.Pm, nk * 3), Y.take(L.Pc, nk * 3), Y.take(L.pxc, nk * 2), Y.take(L.pxm, nk * 2), Y.take(L.isc, nk), Y.take(L.ism, nk);
  Y.take(L.pose, 6), Y.take(L.scale, 1), Y.take(L.Scm, 13), Y.take(L.Scw, 13), Y.take(L.cam4, 4), Y.take(L.sums, 2);
  Y.take(L.mark, s), Y.take(L.fnd, s), Y.take(L.qok, p);
  Y.take(L.loop_ids, p), Y.take(L.qlv, p), Y.take(L.qg, p), Y.take(L.match_ids, nk), Y.take(L.qu, p), Y.take(L.qv, p);
  L.NK = NK, L.C = C, L.P = P, L.max_rand = max_rand, L.n_slots = n_slots;
}

}  // namespace

extern "C" int vo_kfstore_loop_ransac_max_iters(int n) {
  if (n <= kRansacMinInliers) return 1;  // :88-89; below 20 iterate() never reaches a trip (:106-112)
  const float epsilon = static_cast<float>(kRansacMinInliers) / static_cast<float>(n);
  const int iterations = (int)std::ceil(std::log(1 - 0.99) / std::log(1 - std::pow(epsilon, 3)));
  return std::max(1, std::min(iterations, kRansacMaxIterations));
}

namespace {

size_t loop_bytes(int NK, int max_cand, int max_pts, int max_rand, int n_slots) {
  Layout Y{nullptr};
  KfLoopView L{};
  loop_lay(Y, L, NK, max_cand, max_pts, max_rand, n_slots);
  return Y.at;
}

KfLoopView loop_layout(void *block, int NK, int max_cand, int max_pts, int max_rand, int n_slots) {
  Layout Y{reinterpret_cast<uint8_t *>(block)};
  KfLoopView L{};
  loop_lay(Y, L, NK, max_cand, max_pts, max_rand, n_slots);
  return L;
}

// the tables and constants of the block, once (ransacMaxIters by N from the host's libm; the camera as doubles)
int loop_init(const KfLoopView &L, const KfMapView &M, size_t bytes, hipStream_t st) {
  VO_HIP_CHECK(hipMemsetAsync(L.st, 0, bytes, st));
  // Sim3Solver::setRansacParameters(0.99, 20, 300) (sim3Solver.cpp:76-96) for every N a key-frame can give, with the host's
  // C library: the device evaluates no log.  N < 20 never iterates (:106-112); its entry is the 1 that max(1, ...) leaves.
  std::vector<int32_t> tab((size_t)L.NK + 1, 1);
  for (int N = 0; N <= L.NK; N++) tab[(size_t)N] = vo_kfstore_loop_ransac_max_iters(N);
  const double cam4[4] = {(double)M.cam[0], (double)M.cam[1], (double)M.cam[2], (double)M.cam[3]};
  VO_HIP_CHECK(hipMemcpyAsync(L.iters, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
  VO_HIP_CHECK(hipMemcpyAsync(L.cam4, cam4, sizeof(cam4), hipMemcpyHostToDevice, st));
  VO_HIP_CHECK(hipStreamSynchronize(st));  // (tab and cam4 are pageable and leave scope)
  return VO_OK;
}

// a new call: the state reset, `current` checked, the front (match.hip: loop_bow_replay) and the solvers' construction
int loop_begin_enqueue(const LoopArgs &A, int current, int n_cand, int fix_scale, int n_rand, int rand_max, hipStream_t st) {
  VO_HIP_CHECK(hipMemsetAsync(A.L.match_ids, 0xff, (size_t)A.L.NK * 4, st));
  hipLaunchKernelGGL(k_loop_begin, dim3(1), dim3(64), 0, st, A, current, n_cand, fix_scale, n_rand, rand_max);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(loop_bow_replay(A, current, n_cand, st));
  hipLaunchKernelGGL(k_loop_construct, dim3((unsigned)n_cand), dim3(256), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// `rounds` rounds (walk to the next verification or to the end, then verify), then the steps behind a match; launches only
int loop_rounds_enqueue(const LoopArgs &A, int rounds, int fix_scale, hipStream_t st) {
  const KfLoopView &L = A.L;
  const unsigned search_grid = (unsigned)std::min((2 * A.S.NK + 3) / 4, 512);
  for (int r = 0; r < rounds; r++) {
    hipLaunchKernelGGL(k_loop_walk, dim3(1), dim3(kWalkThreads), 0, st, A);
    hipLaunchKernelGGL(k_loop_search, dim3(search_grid), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_loop_gather, dim3(1), dim3(256), 0, st, A);
    VO_HIP_CHECK(hipGetLastError());
    // (off = {0, 0} outside a verification: the refinement then runs on no match and writes nothing that is read)
    VO_CHECK(sim3_solve_dev(1, fix_scale, L.off, L.Pm, L.pxc, L.isc, L.Pc, L.pxm, L.ism, L.cam4, L.pose, L.scale, L.outl, L.ninl, L.sums, st));
    hipLaunchKernelGGL(k_loop_verified, dim3(1), dim3(256), 0, st, A);
    VO_HIP_CHECK(hipGetLastError());
  }
  // behind a match (every kernel returns at once otherwise); the marks are per call
  VO_HIP_CHECK(hipMemsetAsync(L.mark, 0xff, (size_t)L.n_slots * 4, st));
  VO_HIP_CHECK(hipMemsetAsync(L.fnd, 0, (size_t)L.n_slots, st));
  hipLaunchKernelGGL(k_loop_mark, dim3(256), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_loop_collect, dim3(1), dim3(1024), 0, st, A);
  hipLaunchKernelGGL(k_loop_project, dim3(1), dim3(256), (size_t)A.S.NK * 8, st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

LoopArgs loop_args(vo_kfstore *s, const KfObsView &O) {
  const KfConnView C = connections_view(s->conn);
  return LoopArgs{kfstore_view(s), O, C, s->X, s->M, s->F, s->L, C.status};
}

// the candidates and the rand() values are in the block already (L.cand, L.rand)
int loop_compute_enqueue(vo_kfstore *s, int current, int n_cand, int fix_scale, int n_rand, int32_t rand_max, int max_rounds) {
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // "who observes p in key-frame j" (launches only, and only when the index is stale)
  const LoopArgs A = loop_args(s, O);
  VO_CHECK(loop_begin_enqueue(A, current, n_cand, fix_scale ? 1 : 0, n_rand, rand_max, s->st));
  s->loop_fix_scale = fix_scale ? 1 : 0, s->loop_called = true;
  return loop_rounds_enqueue(A, max_rounds, s->loop_fix_scale, s->st);
}

int loop_check(vo_kfstore *s, const char *W, int n_cand, const void *cand, int n_rand, const void *rand_values, int32_t rand_max,
               int max_rounds) {
  VO_CHECK(need(s, W, kLayerLoop));
  if (n_cand < 1 || !cand || n_rand < 0 || (n_rand > 0 && !rand_values) || rand_max < 1 || max_rounds < 0) return VO_ERR_INVALID;
  if (n_cand > s->L.C || n_rand > s->L.max_rand) {
    set_error("%s: %d candidates / %d rand() values, the block was enabled for %d / %d", W, n_cand, n_rand, s->L.C, s->L.max_rand);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

}  // namespace

int vo::loop_compute_counted(vo_kfstore *s, int current, const int *dev_go, int go_value, const int *dev_n, const int *dev_src, int fix_scale,
                             int n_rand, int32_t rand_max, int max_rounds, bool quiet) {
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  const LoopArgs A = loop_args(s, O);
  hipStream_t st = s->st;
  VO_HIP_CHECK(hipMemsetAsync(A.L.match_ids, 0xff, (size_t)A.L.NK * 4, st));
  hipLaunchKernelGGL(k_loop_begin_counted, dim3(1), dim3(64), 0, st, A, current, dev_go, go_value, dev_n, dev_src, fix_scale ? 1 : 0, n_rand,
                     rand_max, quiet ? 1 : 0);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(loop_bow_replay(A, current, A.L.C, st));
  hipLaunchKernelGGL(k_loop_construct, dim3((unsigned)A.L.C), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_loop_trim, dim3(1), dim3(64), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  s->loop_fix_scale = fix_scale ? 1 : 0, s->loop_called = true;
  return loop_rounds_enqueue(A, max_rounds, s->loop_fix_scale, st);
}

extern "C" {

int vo_kfstore_enable_loop(vo_kfstore *s, int max_candidates, int max_loop_points, int max_rand) {
  const char *W = "vo_kfstore_enable_loop";
  const bool args_ok = max_candidates >= 1 && max_candidates <= VO_KFSTORE_LOOP_MAX_CANDIDATES && max_loop_points >= 1 && max_rand >= 3;
  if (const int rc = enable_begin(s, W, kLayerFuse, kLayerLoop, args_ok)) return rc < 0 ? rc : VO_OK;
  const size_t bytes = loop_bytes(s->NK, max_candidates, max_loop_points, max_rand, s->okeys_cap);
  VO_CHECK(s->lp.reserve(bytes));
  s->L = loop_layout(s->lp.p, s->NK, max_candidates, max_loop_points, max_rand, s->okeys_cap);
  const size_t down = (size_t)(kLoopStateInts + VO_KFSTORE_LOOP_MAX_CANDIDATES * kLoopPerInts + s->NK + max_loop_points) * 4 + 26 * 8;
  VO_CHECK(s->lp_stage.reserve(std::max(((size_t)VO_KFSTORE_LOOP_MAX_CANDIDATES + (size_t)max_rand) * 4, down)));
  VO_CHECK(loop_init(s->L, s->M, bytes, s->st));  // (synchronises: its tables are host temporaries)
  s->layers |= kLayerLoop;
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
  VO_CHECK(copy_h2d(s->L.cand, up, ((size_t)VO_KFSTORE_LOOP_MAX_CANDIDATES + (size_t)n_rand) * 4, s->st, W));
  VO_CHECK(loop_compute_enqueue(s, current, n_cand, fix_scale, n_rand, rand_max, max_rounds));
  return stream_sync(s->st, W);
}

int vo_kfstore_compute_sim3_continue(vo_kfstore *s, int max_rounds) {
  const char *W = "vo_kfstore_compute_sim3_continue";
  VO_CHECK(need(s, W, kLayerLoop));
  if (max_rounds < 0) return VO_ERR_INVALID;
  if (!s->loop_called) {
    set_error("%s: no vo_kfstore_compute_sim3 has been enqueued on this store", W);
    return VO_ERR_INVALID;
  }
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  return loop_rounds_enqueue(loop_args(s, O), max_rounds, s->loop_fix_scale, s->st);
}

int vo_kfstore_loop_result(vo_kfstore *s, int32_t *record, int32_t *per_cand, double *Scm, double *Scw, int32_t *match_ids,
                           int32_t *n_loop_points, int32_t *loop_point_ids) {
  const char *W = "vo_kfstore_loop_result";
  VO_CHECK(need(s, W, kLayerLoop));
  const KfLoopView &L = s->L;
  int32_t st[kLoopStateInts], per[VO_KFSTORE_LOOP_MAX_CANDIDATES * kLoopPerInts];
  double sims[26];
  VO_CHECK(copy_d2h(st, L.st, sizeof(st), s->st, W));
  VO_CHECK(copy_d2h(per, L.per, sizeof(per), s->st, W));
  VO_CHECK(copy_d2h(sims, L.Scm, 13 * 8, s->st, W));
  VO_CHECK(copy_d2h(sims + 13, L.Scw, 13 * 8, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int n_cur = std::min(std::max(st[kLsNCur], 0), s->NK), n_lp = st[kLsState] >= 2 ? std::min(std::max(st[kLsNLoop], 0), L.P) : 0;
  if (match_ids && n_cur > 0) VO_CHECK(copy_d2h(match_ids, L.match_ids, (size_t)n_cur * 4, s->st, W));
  if (loop_point_ids && n_lp > 0) VO_CHECK(copy_d2h(loop_point_ids, L.loop_ids, (size_t)n_lp * 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  if (record) {
    memset(record, 0, 16 * 4);
    memcpy(record, st, 9 * 4);
  }
  if (per_cand) memcpy(per_cand, per, (size_t)L.C * kLoopPerInts * 4);
  if (Scm) memcpy(Scm, sims, 13 * 8);
  if (Scw) memcpy(Scw, sims + 13, 13 * 8);
  if (n_loop_points) *n_loop_points = n_lp;
  return VO_OK;
}

int vo_kfstore_loop_solver_inputs(vo_kfstore *s, int position, int32_t *n, double *cam1_points, double *cam2_points, double *pixels1,
                                  double *pixels2, int32_t *max_err1, int32_t *max_err2, int32_t *matched_index) {
  const char *W = "vo_kfstore_loop_solver_inputs";
  VO_CHECK(need(s, W, kLayerLoop));
  const KfLoopView &L = s->L;
  if (position < 0 || position >= L.C || !n) return VO_ERR_INVALID;
  int32_t per[kLoopPerInts];
  VO_CHECK(copy_d2h(per, L.per + position * kLoopPerInts, sizeof(per), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const size_t N = (size_t)std::min(std::max(per[kLpN], 0), s->NK), o = (size_t)position * s->NK;
  *n = (int32_t)N;
  if (N == 0) return VO_OK;
  if (cam1_points) VO_CHECK(copy_d2h(cam1_points, L.pc1 + o * 3, N * 24, s->st, W));
  if (cam2_points) VO_CHECK(copy_d2h(cam2_points, L.pc2 + o * 3, N * 24, s->st, W));
  if (pixels1) VO_CHECK(copy_d2h(pixels1, L.px1 + o * 2, N * 16, s->st, W));
  if (pixels2) VO_CHECK(copy_d2h(pixels2, L.px2 + o * 2, N * 16, s->st, W));
  if (max_err1) VO_CHECK(copy_d2h(max_err1, L.me1 + o, N * 4, s->st, W));
  if (max_err2) VO_CHECK(copy_d2h(max_err2, L.me2 + o, N * 4, s->st, W));
  if (matched_index) VO_CHECK(copy_d2h(matched_index, L.midx + o, N * 4, s->st, W));
  return stream_sync(s->st, W);
}

}  // extern "C"
