// fuse.hip -- map-point fusion on the device: LocalMapping::searchInNeighbors
// (localMapping.cpp:363-432), Matcher::fuseMapPoints (matcher.cpp:1012-1133) and MapPoint::replaceMapPoint
// (mappoint.cpp:214-253) over the key-frame store's observation index AS IT STOOD AT THE START OF THE CALL plus an overlay
// (kfstore.h: KfOverlay; obs_walk.h: obs_overlay_wave), so that a call of up to 61 fuse steps never rebuilds the index.
//   k_fuse_begin    the target list from section 4h's ordered lists (one thread) and `current`'s ids (a thread per feature)
//   k_fuse_mark     a thread per list entry: the id's slot (the start of its run), an atomic maximum there decides the first
//                   occurrence of the id in the list without a sort
//   k_fuse_search   a workgroup stages the target's x, y, octave and u_right in LDS; a wavefront per list entry: holders
//                   through the overlay, the gates of a candidate, then lanes over the target's features -- cell rule, radius,
//                   octave and chi-square gates, a descriptor fetched only behind them -- and a wave minimum over (distance,
//                   cell column, cell row, feature).  A match reserves its number in the call's match list.
//   k_fuse_mutate   a wavefront (a workgroup of 64) per CHAIN of matches -- the matches that hit one feature of the target,
//                   or features that carried one id when the step began -- in list order, lanes over carriers: add, or
//                   replace in either direction with the counters and computeDescriptor of the survivor
//   k_fuse_gather   the closing step's list: the targets' ids, a thread per (target, feature)
//   k_fuse_live     `current`'s live ids, each once, for the closing descriptors and refresh
// The carrier collection, replaceMapPoint and computeDescriptor code is in fuse_ops.h, shared with loop_fuse.hip (section 4q).
// No kernel waits on another workgroup; every loop is bounded by a count read once or by an array's size; chains read and
// write disjoint ids and disjoint features, so every byte has one writer per launch.
#include "kfstore.h"

#include "fuse_ops.h"
#include "kf_area.h"
#include "new_points_geom.h"

namespace {

using namespace vo;
using namespace vo::fuse_ops;

constexpr int kMutateGrid = 256, kSearchGrid = 1024;
constexpr int kThLow = 50;
constexpr int kGridCols = kAreaCols, kGridRows = kAreaRows;

__device__ __forceinline__ unsigned first_code(int step, int pos) { return ((unsigned)(step + 1) << 24) | (0xffffffu - (unsigned)pos); }

// ---- the target list (localMapping.cpp:365-386) and current's ids (:390)
__global__ __launch_bounds__(256) void k_fuse_begin(FuseArgs A, int current) {
  const int i = blockIdx.x * 256 + threadIdx.x, NK = A.S.NK;
  const bool ok = target_ready(A, current);
  if (i < NK) {
    int id = -1;
    if (ok && i < n_features(A.S, current) && (kf_sec<uint8_t>(A.S, current, A.S.o_flags)[i] & 1)) id = kf_sec<int>(A.S, current, A.S.o_ids)[i];
    A.F.snap[i] = id;
  }
  if (i != 0) return;
  int n = 0;
  if (!ok) atomicOr(A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  if (ok) {
    const int size = A.S.size, n1 = min(min(max(A.C.n_ordered[current], 0), min(size, A.C.max_kf)), 10);
    const int *l1 = A.C.ordered + (size_t)current * A.C.max_kf;
    int marked[10], n_marked = 0;
    auto is_marked = [&](int k) {
      for (int m = 0; m < n_marked; m++)
        if (marked[m] == k) return true;
      return false;
    };
    for (int a = 0; a < n1; a++) {
      const int kfn = l1[a];
      if (kfn < 0 || kfn >= size || kf_bad(A.S, kfn) || is_marked(kfn)) continue;  // (:371)
      A.F.targets[n++] = kfn, marked[n_marked++] = kfn;
      const int n2 = min(min(max(A.C.n_ordered[kfn], 0), min(size, A.C.max_kf)), 5);
      const int *l2 = A.C.ordered + (size_t)kfn * A.C.max_kf;
      for (int b = 0; b < n2; b++) {
        const int kfs = l2[b];
        if (kfs < 0 || kfs >= size || kf_bad(A.S, kfs) || is_marked(kfs) || kfs == current) continue;  // (:381)
        A.F.targets[n++] = kfs;  // (only first neighbours are marked: a key-frame may come again)
      }
    }
  }
  for (int t = n; t < kFuseFinal; t++) A.F.targets[t] = -1;
  A.F.targets[kFuseFinal] = ok ? current : -1;
  A.F.head[0] = n, A.F.head[2] = current;
}

__global__ void k_fuse_begin_single(KfFuseView F, int target) {
  if (threadIdx.x == 0) F.targets[0] = target, F.targets[kFuseFinal] = -1, F.head[0] = 1, F.head[2] = target;
}

// ---- a step's list: the first occurrence of every id
__global__ __launch_bounds__(256) void k_fuse_mark(FuseArgs A, int step, const int *list, int n_max, const int *n_dev) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  const int T = A.F.targets[step];
  if (pos == 0) {
    int *rec = A.F.rec + step * kFuseRecInts;
    rec[kFuTarget] = T;
    A.F.base[step] = A.F.head[1];
    if (T >= 0 && !target_ready(A, T)) rec[kFuUndone] = 2, atomicOr(A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  }
  if (T < 0) return;
  const int n = n_dev ? min(max(*n_dev, 0), n_max) : n_max;
  if (pos >= n) return;
  const int id = list[pos];
  if (id < 0) return;
  const int p = slot_of(A.O, id);
  if (p >= 0 && p < A.F.V.n_slots) atomicMax(reinterpret_cast<unsigned *>(A.F.first) + p, first_code(step, pos));
}

// ---- the gates of a candidate and its best match
__global__ __launch_bounds__(256) void k_fuse_search(FuseArgs A, int step, const int *list, int n_max, const int *n_dev, float threshold) {
  extern __shared__ float4 s_feat[];  // x, y, u_right, octave (as int bits)
  const int T = A.F.targets[step];
  if (T < 0 || !target_ready(A, T)) return;  // (uniform over the grid)
  const KfStoreView &S = A.S;
  const int NK = S.NK, nT = n_features(S, T), tid = threadIdx.x, lane = tid & 63;
  {
    const float *x = np_x(A.M, T), *y = np_y(A.M, T), *ur = cull_uright(A.X, T);
    const int *oc = cull_octave(A.X, T);
    for (int f = tid; f < nT; f += 256) s_feat[f] = make_float4(x[f], y[f], ur[f], __int_as_float(oc[f]));
  }
  __syncthreads();
  const int n = n_dev ? min(max(*n_dev, 0), n_max) : n_max;
  const float fx = A.M.cam[0], fy = A.M.cam[1], cx = A.M.cam[2], cy = A.M.cam[3], bf = A.M.cam[4];
  const int n_levels = min(max(A.M.n_levels, 1), 16);
  const float log_sf1 = (float)log((double)A.M.sf[1]);
  const double *Tp = np_pose(A.M, T);
  double Ow[3];
  np_center(Tp, Ow);
  int *rec = A.F.rec + step * kFuseRecInts;
  for (int pos = blockIdx.x * 4 + (tid >> 6); pos < n; pos += (int)gridDim.x * 4) {  // (uniform over the wavefront)
    const int id = list[pos];
    if (id < 0) continue;
    const int p = slot_of(A.O, id);
    if (p < 0 || p >= A.F.V.n_slots || (unsigned)A.F.first[p] != first_code(step, pos)) continue;  // a second occurrence is always skipped
    // `mp->isBad() || mp->beObserved(keyframe)` (:1029): the holders through the overlay; the attributes of the first live carrier
    unsigned lowest = ~0u;
    bool in_T = false;
    obs_overlay_wave(A.O, A.F.V, p, [&](bool valid, unsigned e) {
      if (valid && carries(S, e, id)) {
        lowest = min(lowest, e);
        if ((int)(e / (unsigned)NK) == T) in_T = true;
      }
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) lowest = min(lowest, (unsigned)__shfl_xor((int)lowest, o));
    if (lowest == ~0u || __ballot(in_T) != 0ull) continue;
    const int kk = (int)(lowest / (unsigned)NK), ff = (int)(lowest - (unsigned)kk * (unsigned)NK);
    const double *pw = kf_sec<double>(S, kk, S.o_points) + 3 * (size_t)ff;
    double pc[3];
    for (int r = 0; r < 3; r++) pc[r] = __dadd_rn(np_dot3(Tp[3 * r], pw[0], Tp[3 * r + 1], pw[1], Tp[3 * r + 2], pw[2]), Tp[9 + r]);
    const float z = (float)pc[2];
    if (z < 0.0f) continue;  // (:1036)
    const float invz = __fdiv_rn(1.0f, z);
    const float xn = __fmul_rn((float)pc[0], invz), yn = __fmul_rn((float)pc[1], invz);
    const float u = __fadd_rn(__fmul_rn(fx, xn), cx), v = __fadd_rn(__fmul_rn(fy, yn), cy);
    if (!(u >= A.F.xmin && v >= A.F.ymin && u < A.F.xmax && v < A.F.ymax)) continue;  // isInImg (keyframe.cpp:64-67)
    const float ur = __fsub_rn(u, __fmul_rn(bf, invz));
    double line[3];
    for (int c = 0; c < 3; c++) line[c] = __dadd_rn(pw[c], -Ow[c]);
    const float dist = (float)__dsqrt_rn(np_dot3(line[0], line[0], line[1], line[1], line[2], line[2]));
    const float maxd = kf_sec<float>(S, kk, S.o_maxd)[ff], mind = kf_sec<float>(S, kk, S.o_mind)[ff];
    if (dist < __fmul_rn(0.8f, mind) || dist > __fmul_rn(1.2f, maxd)) continue;  // (:1055, mappoint.cpp:391-401)
    const double *pn = A.O.normals + ((size_t)kk * NK + ff) * 3;
    if (np_dot3(line[0], pn[0], line[1], pn[1], line[2], pn[2]) < __dmul_rn(0.5, (double)dist)) continue;  // (:1059)
    const int level = predict_level(maxd, dist, log_sf1, n_levels);  // predictScale (mappoint.cpp:198-212)
    const float radius = __fmul_rn(threshold, A.M.sf[level]);
    if (lane == 0) atomicAdd(rec + kFuPassed, 1);
    const AreaWindow W = area_window(A.F, u, v, radius);  // getFeaturesInArea (keyframe.cpp:268-309), kf_area.h
    if (!W.any) continue;
    const uint4 *qd = reinterpret_cast<const uint4 *>(record_of(S, kk) + S.o_pdesc) + 2 * (size_t)ff;
    const uint4 qa = qd[0], qb = qd[1];
    unsigned long long best = ~0ull;
    for (int f = lane; f < nT; f += 64) {
      const float4 t = s_feat[f];
      int gx, gy;
      if (!area_holds(A.F, W, t.x, t.y, u, v, radius, gx, gy)) continue;
      const int oct = __float_as_int(t.w);
      if (oct < level - 1 || oct > level) continue;  // (:1077)
      const float ex = __fsub_rn(u, t.x), ey = __fsub_rn(v, t.y);
      const float inv = __fdiv_rn(1.0f, A.M.sf[min(max(oct, 0), 15)]);
      float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), th = 5.991f;
      if (t.z >= 0.f) {
        const float er = __fsub_rn(ur, t.z);
        e2 = __fadd_rn(e2, __fmul_rn(er, er)), th = 7.815f;
      }
      if (__fmul_rn(__fmul_rn(e2, inv), inv) > th) continue;  // (:1090, :1097)
      const uint4 *dd = reinterpret_cast<const uint4 *>(kf_sec<uint8_t>(S, T, S.o_desc)) + 2 * (size_t)f;
      const uint4 da = dd[0], db = dd[1];
      const unsigned long long key = area_key(hamming256(qa, qb, da, db), gx, gy, f);
      best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    if (best == ~0ull || (int)(best >> 44) > kThLow) continue;  // (:1109)
    if (lane == 0) {
      const int f = (int)(best & 0xffffffffu);
      atomicAdd(rec + kFuMatches, 1);
      const int m = atomicAdd(A.F.head + 1, 1);
      if (m >= 0 && m < A.F.M) {
        // the chain of the match: the id the feature carries as the step begins, else the feature
        const unsigned eT = (unsigned)T * (unsigned)NK + (unsigned)f;
        const int org = *id_word(S, eT);
        int key = A.O.n_keys + f;
        if ((*flag_byte(S, eT) & 1) && org >= 0) {
          const int po = slot_of(A.O, org);
          if (po >= 0) key = po;
        }
        A.F.mt[m] = make_int4(pos, id, p, f), A.F.key[m] = key;
      }
    }
  }
}

// ---- the mutation (:1109-1127) of one chain per wavefront
__global__ __launch_bounds__(64) void k_fuse_mutate(FuseArgs A, int step) {
  __shared__ MutateLds L;
  const int T = A.F.targets[step];
  if (T < 0 || !target_ready(A, T)) return;
  const int lane = threadIdx.x, NK = A.S.NK;
  const int base = min(max(A.F.base[step], 0), A.F.M), end = A.F.head[1];
  int *rec = A.F.rec + step * kFuseRecInts;
  // more candidates passed the gates than a step takes, or the call's matches do not fit: the step is left undone
  if (rec[kFuPassed] > A.F.M || end > A.F.M) {
    if (blockIdx.x == 0 && lane == 0) atomicOr(A.status, (int)VO_KFSTORE_FUSE_CAPACITY), rec[kFuUndone] = 1;
    return;
  }
  const KfOverlay &V = A.F.V;
  for (int m0 = base + (int)blockIdx.x; m0 < end; m0 += (int)gridDim.x) {
    const int key = A.F.key[m0], pos0 = A.F.mt[m0].x;
    bool later = false;  // the chain's leader is its first match in list order
    for (int o = base + lane; o < end; o += 64) later |= A.F.key[o] == key && A.F.mt[o].x < pos0;
    if (__ballot(later) != 0ull) continue;
    int cur = m0;
    for (int guard = base; cur >= 0 && guard < end; guard++) {
      const int4 mt = A.F.mt[cur];
      const int mp = mt.y, p_mp = mt.z, f = mt.w;
      if (p_mp >= 0 && p_mp < V.n_slots && f >= 0 && f < NK) {
        const unsigned eT = (unsigned)T * (unsigned)NK + (unsigned)f;
        const int nb0 = collect(A, mp, p_mp, L.b);
        bool held = false;
        for (int c = lane; c < min(nb0, kMaxC); c += 64) held |= (int)(L.b[c] / (unsigned)NK) == T;
        const int org = *id_word(A.S, eT);
        const bool occupied = (*flag_byte(A.S, eT) & 1) && org >= 0;
        if (nb0 == 0 || __ballot(held) != 0ull) {
          // (a candidate that passed is not held by the target and has a holder: nothing to do here)
        } else if (!occupied) {  // addObservation + addMapPoint (:1124-1125)
          const unsigned src = lowest_of(L.b, nb0);
          if (lane == 0) {
            const Attr a = attr_of(A, src);
            take(A, eT, mp, a);
            uint8_t *fb = flag_byte(A.S, eT);
            *fb = (uint8_t)(*fb | 1);
            V.node_entry[cur] = (int)eT, V.node_next[cur] = V.a_head[p_mp], V.a_head[p_mp] = cur + 1;
            atomicAdd(rec + kFuAdds, 1);
          }
        } else {
          const int p_org = slot_of(A.O, org);
          const int na0 = p_org >= 0 && p_org < V.n_slots ? collect(A, org, p_org, L.a) : 0;
          if (na0 > kMaxC || nb0 > kMaxC || p_org < 0 || p_org >= V.n_slots) {
            if (lane == 0) atomicOr(A.status, (int)VO_KFSTORE_FUSE_CAPACITY);
          } else {
            const int obs_org = classify(A, L.a, na0, L.ca), obs_mp = classify(A, L.b, nb0, L.cb);
            const bool keep_org = obs_org > obs_mp;  // (:1116)
            if (keep_org) {  // the point that goes is the candidate: its carriers change places with org's, so that A sits in L.a
              for (int c = lane; c < max(na0, nb0); c += 64) {
                const unsigned x = L.a[c];
                const uint8_t y = L.ca[c];
                L.a[c] = L.b[c], L.ca[c] = L.cb[c], L.b[c] = x, L.cb[c] = y;
              }
              __syncthreads();
            }
            const int idA = keep_org ? mp : org, idB = keep_org ? org : mp, pA = keep_org ? p_mp : p_org, pB = keep_org ? p_org : p_mp;
            const int na = keep_org ? nb0 : na0, nb = keep_org ? na0 : nb0;
            int moved, cleared;
            replace_carriers(A, L, idA, idB, pA, pB, na, nb, moved, cleared);  // replaceMapPoint (mappoint.cpp:235-251), fuse_ops.h
            if (lane == 0) {
              atomicAdd(rec + (keep_org ? kFuKeptOrg : kFuKeptCand), 1);
              if (cleared) atomicAdd(rec + kFuCleared, cleared);
            }
          }
        }
      }
      __threadfence_block();
      __syncthreads();
      // the chain's next match in list order
      unsigned long long nxt = ~0ull;
      const int pos_cur = mt.x;
      for (int o = base + lane; o < end; o += 64) {
        const int po = A.F.mt[o].x;
        if (A.F.key[o] == key && po > pos_cur) {
          const unsigned long long k2 = ((unsigned long long)(unsigned)po << 32) | (unsigned)o;
          nxt = k2 < nxt ? k2 : nxt;
        }
      }
      nxt = wave_min_u64(nxt);
      cur = nxt == ~0ull ? -1 : (int)(nxt & 0xffffffffu);
    }
  }
}

// ---- the closing step's candidates (:397-416): the targets' ids, first occurrences decided by k_fuse_mark
__global__ __launch_bounds__(256) void k_fuse_gather(FuseArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x, NK = A.S.NK;
  const int n_t = min(max(A.F.head[0], 0), kFuseFinal);
  if (i == 0) A.F.head[3] = n_t * NK;
  if (i >= n_t * NK) return;
  const int t = i / NK, f = i - t * NK, T = A.F.targets[t];
  int id = -1;
  if (T >= 0 && T < A.S.size && !A.X.erased[T] && f < n_features(A.S, T) && (kf_sec<uint8_t>(A.S, T, A.S.o_flags)[f] & 1))
    id = kf_sec<int>(A.S, T, A.S.o_ids)[f];
  A.F.list[i] = id;
}

// ---- current's live points (:420-429), each id once
__global__ __launch_bounds__(256) void k_fuse_live(FuseArgs A, int current) {
  const int i = blockIdx.x * 256 + threadIdx.x, NK = A.S.NK;
  if (i == 0) A.F.head[2] = current;
  if (i >= NK) return;
  int id = -1;
  if (target_ready(A, current) && i < n_features(A.S, current)) {
    const uint8_t *fl = kf_sec<uint8_t>(A.S, current, A.S.o_flags);
    const int *ids = kf_sec<int>(A.S, current, A.S.o_ids);
    if ((fl[i] & 1) && ids[i] >= 0) {
      id = ids[i];
      for (int o = 0; o < i; o++)
        if ((fl[o] & 1) && ids[o] == id) {
          id = -1;
          break;
        }
    }
  }
  A.F.snap[i] = id;
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

void fuse_lay(Layout &L, KfFuseView &F, int NK, int M, int n_slots) {
  const size_t s = (size_t)n_slots, m = (size_t)M;
  L.take(F.head, 4), L.take(F.base, 64), L.take(F.targets, 64), L.take(F.rec, 64 * kFuseRecInts);
  L.take(F.first, s), L.take(F.V.m_next, s), L.take(F.V.m_tail, s), L.take(F.V.a_head, s);
  F.reset_bytes = L.at;
  L.take(F.V.node_entry, m), L.take(F.V.node_next, m), L.take(F.key, m), L.take(F.mt, m);
  L.take(F.snap, (size_t)NK), L.take(F.list, (size_t)kFuseFinal * NK);
  F.NK = NK, F.M = M, F.list_cap = kFuseFinal * NK, F.V.n_slots = n_slots, F.V.n_nodes = M;
}

int step_enqueue(const FuseArgs &A, int step, const int *list, int n_max, const int *n_dev, float threshold, hipStream_t st) {
  // (an empty list still gets the step's record and the sticky word of a target that is erased or has no pose)
  hipLaunchKernelGGL(k_fuse_mark, dim3((unsigned)std::max((n_max + 255) / 256, 1)), dim3(256), 0, st, A, step, list, std::max(n_max, 0), n_dev);
  if (n_max <= 0) {
    VO_HIP_CHECK(hipGetLastError());
    return VO_OK;
  }
  const int blocks = std::min((n_max + 3) / 4, kSearchGrid);
  hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)blocks), dim3(256), (size_t)A.S.NK * sizeof(float4), st, A, step, list, n_max, n_dev,
                     threshold);
  hipLaunchKernelGGL(k_fuse_mutate, dim3(kMutateGrid), dim3(64), 0, st, A, step);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

size_t fuse_bytes(int NK, int max_matches, int n_slots) {
  Layout L{nullptr};
  KfFuseView F{};
  fuse_lay(L, F, NK, max_matches, n_slots);
  return L.at;
}

KfFuseView fuse_layout(void *block, int NK, int max_matches, int n_slots, const float bounds[4]) {
  Layout L{reinterpret_cast<uint8_t *>(block)};
  KfFuseView F{};
  fuse_lay(L, F, NK, max_matches, n_slots);
  F.xmin = bounds[0], F.xmax = bounds[1], F.ymin = bounds[2], F.ymax = bounds[3];
  F.gpw = (float)kGridCols / (F.xmax - F.xmin), F.gph = (float)kGridRows / (F.ymax - F.ymin);  // (camera.cpp:47-48)
  return F;
}

// one fuse call on its own: reset, then mark / search / mutate for step 0 over the n ids of a device list
int fuse_single_enqueue(const FuseArgs &A, int target, int n, const int *dev_ids, float threshold, hipStream_t st) {
  VO_HIP_CHECK(hipMemsetAsync(A.F.head, 0, A.F.reset_bytes, st));
  hipLaunchKernelGGL(k_fuse_begin_single, dim3(1), dim3(64), 0, st, A.F, target);
  return step_enqueue(A, 0, dev_ids, n, nullptr, threshold, st);
}

// the composed call up to the closing rebuild: reset, target list and snapshot, 60 target steps, the gather, the closing step
int fuse_neighbors_enqueue(const FuseArgs &A, int current, hipStream_t st) {
  const int NK = A.S.NK;
  VO_HIP_CHECK(hipMemsetAsync(A.F.head, 0, A.F.reset_bytes, st));
  hipLaunchKernelGGL(k_fuse_begin, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, st, A, current);
  for (int step = 0; step < kFuseFinal; step++) VO_CHECK(step_enqueue(A, step, A.F.snap, NK, nullptr, 3.0f, st));  // (:389-395)
  hipLaunchKernelGGL(k_fuse_gather, dim3((unsigned)((kFuseFinal * NK + 255) / 256)), dim3(256), 0, st, A);
  return step_enqueue(A, kFuseFinal, A.F.list, kFuseFinal * NK, A.F.head + 3, 3.0f, st);  // (:418)
}

// current's live ids, each once, into F.snap (behind the rebuild: the list of the closing descriptors and refresh)
int fuse_live_list_enqueue(const FuseArgs &A, int current, hipStream_t st) {
  hipLaunchKernelGGL(k_fuse_live, dim3((unsigned)((A.S.NK + 255) / 256)), dim3(256), 0, st, A, current);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

FuseArgs fuse_args(vo_kfstore *s, const KfObsView &O) {
  const KfConnView C = connections_view(s->conn);
  return FuseArgs{kfstore_view(s), O, C, s->X, s->M, s->B, s->U, s->F, s->normals.as<double>(), C.status};
}

// a fuse call's head: the layer, the target, the list (at most F.list_cap ids) and the threshold
int fuse_check(const vo_kfstore *s, const char *W, int target, int n, const int32_t *ids, float threshold) {
  VO_CHECK(need(s, W, kLayerFuse));
  VO_CHECK(need_keyframe(s, W, target));
  if (n < 0 || (n > 0 && !ids) || !(threshold > 0.f)) return VO_ERR_INVALID;
  if (n > s->F.list_cap) {
    set_error("%s: %d ids, the store takes %d (60 * max_features)", W, n, s->F.list_cap);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_fuse(vo_kfstore *s, const float bounds[4], int max_candidates) {
  const char *W = "vo_kfstore_enable_fuse";
  const bool args_ok = bounds && max_candidates >= 1 && bounds[1] > bounds[0] && bounds[3] > bounds[2];
  if (const int rc = enable_begin(s, W, kLayerUpkeep, kLayerFuse, args_ok)) return rc < 0 ? rc : VO_OK;
  if (s->NK > 4096) {
    set_error("%s: %d features per key-frame, the search stages at most 4096", W, s->NK);
    return VO_ERR_CAPACITY;
  }
  const size_t bytes = fuse_bytes(s->NK, max_candidates, s->okeys_cap);
  VO_CHECK(s->fu.reserve(bytes));
  s->F = fuse_layout(s->fu.p, s->NK, max_candidates, s->okeys_cap, bounds);
  VO_CHECK(s->up_stage.reserve((size_t)s->F.list_cap * 4));
  VO_HIP_CHECK(hipMemsetAsync(s->fu.p, 0, bytes, s->st));
  VO_HIP_CHECK(hipMemsetAsync(s->F.targets, 0xff, 64 * 4, s->st));  // (no call yet: no step)
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerFuse;
  return VO_OK;
}

int vo_kfstore_fuse_map_points_dev(vo_kfstore *s, int target, int n, const int32_t *dev_ids, float threshold) {
  const char *W = "vo_kfstore_fuse_map_points_dev";
  VO_CHECK(fuse_check(s, W, target, n, dev_ids, threshold));
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  VO_CHECK(fuse_single_enqueue(fuse_args(s, O), target, n, dev_ids, threshold, s->st));
  s->obs_dirty = true, s->gen++;  // (whether anything matched only the device knows)
  return VO_OK;
}

int vo_kfstore_fuse_map_points(vo_kfstore *s, int target, int n, const int32_t *ids, float threshold) {
  const char *W = "vo_kfstore_fuse_map_points";
  VO_CHECK(fuse_check(s, W, target, n, ids, threshold));
  if (n > 0) {
    memcpy(s->up_stage.data(), ids, (size_t)n * 4);
    VO_CHECK(copy_h2d(s->F.list, s->up_stage.data(), (size_t)n * 4, s->st, W));
  }
  VO_CHECK(vo_kfstore_fuse_map_points_dev(s, target, n, s->F.list, threshold));
  return stream_sync(s->st, W);
}

int vo_kfstore_search_in_neighbors(vo_kfstore *s, int current) {
  const char *W = "vo_kfstore_search_in_neighbors";
  VO_CHECK(need(s, W, kLayerFuse));
  VO_CHECK(need_keyframe(s, W, current));
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // the index the overlay stands on
  VO_CHECK(fuse_neighbors_enqueue(fuse_args(s, O), current, s->st));
  s->obs_dirty = true, s->gen++;
  VO_CHECK(kfstore_obs_view(s, &O));  // the one rebuild behind the fuses, whatever their number
  const FuseArgs A = fuse_args(s, O);
  VO_CHECK(fuse_live_list_enqueue(A, current, s->st));
  VO_CHECK(upkeep_descriptors_enqueue(A.S, O, s->U, A.status, s->NK, s->F.snap, s->st));             // computeDescriptor (:426)
  VO_CHECK(ba_refresh_list_enqueue(A.S, O, s->X, s->M, s->B, A.normals, A.status, s->NK, s->F.snap, s->st));  // (:427)
  return connections_update(s->conn, A.S, O, 1, s->F.head + 2, s->st);  // keyframe_curr_->updateConnections() (:431)
}

int vo_kfstore_fuse_result(vo_kfstore *s, int32_t *record, int32_t *targets, int32_t *per_target) {
  const char *W = "vo_kfstore_fuse_result";
  VO_CHECK(need(s, W, kLayerFuse));
  int32_t head[4], tg[64], rec[64 * kFuseRecInts];
  VO_CHECK(copy_d2h(head, s->F.head, sizeof(head), s->st, W));
  VO_CHECK(copy_d2h(tg, s->F.targets, sizeof(tg), s->st, W));
  VO_CHECK(copy_d2h(rec, s->F.rec, sizeof(rec), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  int32_t out_rec[8] = {0}, out_t[VO_KFSTORE_FUSE_MAX_STEPS], out_p[VO_KFSTORE_FUSE_MAX_STEPS * 6];
  memset(out_t, 0xff, sizeof(out_t)), memset(out_p, 0, sizeof(out_p));
  const int n_t = std::min(std::max(head[0], 0), kFuseFinal);
  int n = 0;
  for (int step = 0; step <= kFuseFinal; step++) {
    if (step < kFuseFinal ? step >= n_t : tg[step] < 0) continue;
    out_t[n] = tg[step];
    for (int c = 0; c < 6; c++) out_p[n * 6 + c] = rec[step * kFuseRecInts + 1 + c], out_rec[1 + c] += out_p[n * 6 + c];
    n++;
  }
  out_rec[0] = n;
  if (record) memcpy(record, out_rec, sizeof(out_rec));
  if (targets) memcpy(targets, out_t, sizeof(out_t));
  if (per_target) memcpy(per_target, out_p, sizeof(out_p));
  return VO_OK;
}

}  // extern "C"
