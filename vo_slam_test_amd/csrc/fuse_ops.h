// fuse_ops.h -- what the fusion kernels (fuse.hip) and the loop fusion (loop_fuse.hip, section 4q) share:
// the live feature words of an entry, the wave reductions, the carriers of an id through the overlay (obs_walk.h), a map
// point's attributes, MapPoint::replaceMapPoint (mappoint.cpp:214-253) over the collected carriers and
// MapPoint::computeDescriptor (mappoint.cpp:118-179) of the survivor.  Every function is called by one WAVEFRONT that is a
// workgroup of 64 (the __syncthreads() below are that wavefront's).
// Include from translation units compiled with -ffp-contract=off only.
#pragma once
#include "kfstore.h"

#include "obs_walk.h"

namespace vo {
namespace fuse_ops {

constexpr int kMaxC = kFuseMaxCarriers;

__device__ __forceinline__ int n_features(const KfStoreView &S, int k) { return min(max(kf_head(S, k)[0], 0), S.NK); }
__device__ __forceinline__ bool kf_bad(const KfStoreView &S, int k) { return kf_head(S, k)[1] != 0; }
__device__ __forceinline__ uint8_t *record_of(const KfStoreView &S, int k) { return const_cast<uint8_t *>(S.base) + (size_t)k * S.rec; }
__device__ __forceinline__ int *id_word(const KfStoreView &S, unsigned e) {
  const unsigned kk = e / (unsigned)S.NK;
  return reinterpret_cast<int *>(record_of(S, (int)kk) + S.o_ids) + (e - kk * (unsigned)S.NK);
}
__device__ __forceinline__ uint8_t *flag_byte(const KfStoreView &S, unsigned e) {
  const unsigned kk = e / (unsigned)S.NK;
  return record_of(S, (int)kk) + S.o_flags + (e - kk * (unsigned)S.NK);
}
// does the live feature word of entry e say "carries id"?
__device__ __forceinline__ bool carries(const KfStoreView &S, unsigned e, int id) {
  if (e / (unsigned)S.NK >= (unsigned)S.size) return false;
  return *id_word(S, e) == id && (*flag_byte(S, e) & 1);
}
__device__ __forceinline__ int slot_of(const KfObsView &O, int id) {
  const int p = obs_lower_bound(O, id);
  return p < O.n_keys && (int)(O.keys[p] >> 32) == id ? p : -1;
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
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ bool target_ready(const FuseArgs &A, int T) {
  return T >= 0 && T < A.S.size && !A.X.erased[T] && *np_pose_set(A.M, T) != 0;
}

// ---- the carriers of id (slot p) through the overlay into `out` (at most kMaxC are stored): their number
__device__ inline int collect(const FuseArgs &A, int id, int p, unsigned *out) {
  const int lane = threadIdx.x & 63;
  int n = 0;
  obs_overlay_wave(A.O, A.F.V, p, [&](bool valid, unsigned e) {
    const bool live = valid && carries(A.S, e, id);
    const unsigned long long m = __ballot(live);
    const int r = n + __popcll(m & ((1ull << lane) - 1ull));
    if (live && r < kMaxC) out[r] = e;
    n += __popcll(m);
  });
  __syncthreads();
  return n;
}

// cls[c] of the n carriers: 0 an entry listed before, 1 its key-frame's observation (the lowest entry), 2 another feature of a
// holder; -> obs(id) (mappoint.cpp:60-63)
__device__ inline int classify(const FuseArgs &A, const unsigned *L, int n, uint8_t *cls) {
  const int lane = threadIdx.x & 63;
  const unsigned NK = (unsigned)A.S.NK;
  int obs = 0;
  for (int c = lane; c < n; c += 64) {
    const unsigned e = L[c], kk = e / NK;
    int k = 1;
    for (int o = 0; o < n && k; o++) {
      const unsigned eo = L[o];
      if (o < c && eo == e) k = 0;
      else if (eo / NK == kk && eo < e) k = 2;
    }
    if (k == 2)
      for (int o = 0; o < c; o++)
        if (L[o] == e) k = 0;
    cls[c] = (uint8_t)k;
    if (k == 1) obs += cull_uright(A.X, (int)kk)[e - kk * NK] >= 0.f ? 2 : 1;
  }
  obs = wave_sum_int(obs);
  __syncthreads();
  return obs;
}

struct Attr {
  double p[3], n[3];
  float mind, maxd;
  int ref;
  uint4 d0, d1;
};
__device__ __forceinline__ Attr attr_of(const FuseArgs &A, unsigned e) {
  const int NK = A.S.NK, kk = (int)(e / (unsigned)NK), f = (int)(e - (unsigned)kk * (unsigned)NK);
  Attr a;
  const double *P = kf_sec<double>(A.S, kk, A.S.o_points) + 3 * (size_t)f, *N = A.normals + ((size_t)kk * NK + f) * 3;
  for (int c = 0; c < 3; c++) a.p[c] = P[c], a.n[c] = N[c];
  a.mind = kf_sec<float>(A.S, kk, A.S.o_mind)[f], a.maxd = kf_sec<float>(A.S, kk, A.S.o_maxd)[f];
  a.ref = A.B.ref_kf[(size_t)kk * NK + f];
  const uint4 *D = reinterpret_cast<const uint4 *>(record_of(A.S, kk) + A.S.o_pdesc) + 2 * (size_t)f;
  a.d0 = D[0], a.d1 = D[1];
  return a;
}
// feature e takes the id and its attributes (bit 0 is the caller's)
__device__ __forceinline__ void take(const FuseArgs &A, unsigned e, int id, const Attr &a) {
  const int NK = A.S.NK, kk = (int)(e / (unsigned)NK), f = (int)(e - (unsigned)kk * (unsigned)NK);
  uint8_t *r = record_of(A.S, kk);
  *id_word(A.S, e) = id;
  double *P = reinterpret_cast<double *>(r + A.S.o_points) + 3 * (size_t)f, *N = A.normals + ((size_t)kk * NK + f) * 3;
  for (int c = 0; c < 3; c++) P[c] = a.p[c], N[c] = a.n[c];
  reinterpret_cast<float *>(r + A.S.o_mind)[f] = a.mind, reinterpret_cast<float *>(r + A.S.o_maxd)[f] = a.maxd;
  A.B.ref_kf[(size_t)kk * NK + f] = a.ref;
  uint4 *D = reinterpret_cast<uint4 *>(r + A.S.o_pdesc) + 2 * (size_t)f;
  D[0] = a.d0, D[1] = a.d1;
}
__device__ __forceinline__ unsigned lowest_of(const unsigned *L, int n) {
  unsigned lo = ~0u;
  for (int c = threadIdx.x & 63; c < min(n, kMaxC); c += 64) lo = min(lo, L[c]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
  return lo;
}

struct MutateLds {
  unsigned a[kMaxC], b[kMaxC], h[kMaxC], t[kMaxC];
  uint8_t ca[kMaxC], cb[kMaxC];
  uint32_t d[kMaxC * 9];
};

// MapPoint::computeDescriptor of B (mappoint.cpp:118-179) from the carriers the replace leaves: B's own (L.b, L.cb) and the
// converted ones of A (L.ca == 3); k_up_desc_over's selection by one wavefront
__device__ inline void descriptor_of(const FuseArgs &A, MutateLds &L, int na, int nb) {
  const int lane = threadIdx.x & 63;
  const unsigned NK = (unsigned)A.S.NK;
  int N = 0;
  for (int pass = 0; pass < 2; pass++) {
    const unsigned *src = pass ? L.a : L.b;
    const uint8_t *cl = pass ? L.ca : L.cb;
    const int want = pass ? 3 : 1, n = pass ? na : nb;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int c = c0 + lane;
      const bool hold = c < n && cl[c] == want && !kf_bad(A.S, (int)(src[c] / NK));  // (:138)
      const unsigned long long m = __ballot(hold);
      const int r = N + __popcll(m & ((1ull << lane) - 1ull));
      if (hold && r < kMaxC) L.h[r] = src[c];
      N += __popcll(m);
    }
  }
  __syncthreads();
  if (N == 0) return;  // `if (desp.empty()) return;`
  if (N > kMaxC) {     // the point keeps its descriptor (section 4l's capacity)
    if (lane == 0) atomicOr(A.status, (int)VO_KFSTORE_UPKEEP_CAPACITY);
    return;
  }
  for (int c = lane; c < N; c += 64) {  // ascending key-frame number: the entries are distinct
    const unsigned e = L.h[c];
    int r = 0;
    for (int o = 0; o < N; o++) r += L.h[o] < e;
    L.t[r] = e;
  }
  __syncthreads();
  for (int i = lane; i < N * 8; i += 64) {
    const unsigned e = L.t[i >> 3], kk = e / NK;
    L.d[(i >> 3) * 9 + (i & 7)] = (kf_sec<uint32_t>(A.S, (int)kk, A.S.o_desc) + 8 * (size_t)(e - kk * NK))[i & 7];
  }
  __syncthreads();
  const int k = (N - 1) / 2;
  constexpr int NC = kMaxC / 64;
  int best_mid = 256, best = 0;
  for (int row = 0; row < N; row++) {
    uint32_t a[8];
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = L.d[row * 9 + j];
    int d[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
      d[c] = 0x7fff;
      const int col = lane + 64 * c;
      if (col < N) {
        int sum = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) sum += __popc(a[j] ^ L.d[col * 9 + j]);
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
    if (lo < best_mid) best_mid = lo, best = row;  // strict: the first row wins (:168)
  }
  const uint32_t *win = L.d + best * 9;
  for (int pass = 0; pass < 2; pass++) {  // every feature that carries B, bad key-frames included
    const unsigned *src = pass ? L.a : L.b;
    const uint8_t *cl = pass ? L.ca : L.cb;
    const int n = pass ? na : nb;
    for (int c = lane; c < n; c += 64) {
      if (pass ? cl[c] != 3 : cl[c] == 0) continue;
      const unsigned e = src[c], kk = e / NK;
      uint32_t *dst = reinterpret_cast<uint32_t *>(record_of(A.S, (int)kk) + A.S.o_pdesc) + 8 * (size_t)(e - kk * NK);
#pragma unroll
      for (int j = 0; j < 8; j++) dst[j] = win[j];
    }
  }
}

// MapPoint::replaceMapPoint(A -> B) (mappoint.cpp:235-251): A's carriers in L.a, classified in L.ca (na of them, slot pA), B's in
// L.b / L.cb (nb >= 1, slot pB), both within kMaxC.  An observation of A whose key-frame does not hold B takes B's id and
// attributes (L.ca becomes 3); every other carrier of A loses bit 0.  addFound / addVisible when both are in the recent list;
// A's runs and added entries go behind B's in the overlay -- unless A had no carrier left (a replace the reference repeats
// on an emptied point: nothing comes over, and a slot is chained behind one root only); computeDescriptor(B).
// -> moved, cleared: the features that took B, the features cleared (uniform over the wavefront)
__device__ inline void replace_carriers(const FuseArgs &A, MutateLds &L, int idA, int idB, int pA, int pB, int na, int nb, int &moved,
                                        int &cleared) {
  const int lane = threadIdx.x & 63, NK = A.S.NK;
  const KfOverlay &V = A.F.V;
  const Attr a = attr_of(A, lowest_of(L.b, nb));
  moved = 0, cleared = 0;
  for (int c = lane; c < na; c += 64) {
    if (L.ca[c] == 0) continue;
    const unsigned e = L.a[c], kk = e / (unsigned)NK;
    bool holds_b = false;
    for (int o = 0; o < nb && !holds_b; o++) holds_b = L.b[o] / (unsigned)NK == kk;
    if (L.ca[c] == 1 && !holds_b) {
      take(A, e, idB, a);
      L.ca[c] = 3;
      moved++;
    } else {  // the holder has B already, or a second feature of a holder
      uint8_t *fb = flag_byte(A.S, e);
      *fb = (uint8_t)(*fb & ~1);
      cleared++;
    }
  }
  cleared = wave_sum_int(cleared), moved = wave_sum_int(moved);
  // addFound / addVisible (:248-249) when both are listed
  int ia = -1, ib = -1;
  const int n_rec = min(max(A.U.head[0], 0), A.U.R);
  for (int j = lane; j < n_rec; j += 64) {
    const int v = A.U.id[j];
    if (v == idA) ia = j;
    if (v == idB) ib = j;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ia = max(ia, __shfl_xor(ia, o)), ib = max(ib, __shfl_xor(ib, o));
  if (lane == 0) {
    if (ia >= 0 && ib >= 0) A.U.found[ib] += A.U.found[ia], A.U.visible[ib] += A.U.visible[ia];
    if (na > 0) {
      const int tail_b = V.m_tail[pB] > 0 ? V.m_tail[pB] - 1 : pB;
      if (tail_b >= 0 && tail_b < V.n_slots) V.m_next[tail_b] = pA + 1;
      V.m_tail[pB] = V.m_tail[pA] > 0 ? V.m_tail[pA] : pA + 1;
    }
  }
  __threadfence_block();
  __syncthreads();
  descriptor_of(A, L, na, nb);
}

}  // namespace fuse_ops
}  // namespace vo
