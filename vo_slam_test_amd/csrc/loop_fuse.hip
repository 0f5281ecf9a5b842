// loop_fuse.hip -- the loop fusion on the device: LoopClosing::searchAndFuse (loopClosing.cpp:496-516),
// Matcher::fuseByPose (matcher.cpp:1135-1238) and the replace loop behind it (:508-513) over the corrected key-frames of a loop,
// one PASS per corrected key-frame, on section 4m's overlay (kfstore.h: KfOverlay), match list and mutate machinery
// (fuse_ops.h): the observation index is rebuilt at most once, in front of the call when it is stale, never between passes.
//   k_lf_begin    the call's head: does it run (the _loop form reads compute_sim3's state), the length of its list, and per
//                 pass the target and whether it is ready (a thread per pass)
//   k_lf_search   a workgroup stages the target's x, y and octave in LDS; a wavefront per loop point: the pose from the
//                 pass's Sim3 (translation NOT divided by the scale, matcher.cpp:1144), holders through the overlay, the gates,
//                 then lanes over the target's features -- cell rule, radius and octave gates, a descriptor fetched only
//                 behind them -- and a wave minimum over (distance, cell column, cell row, feature).  A match reserves its
//                 number in the call's match list
//   k_lf_mutate   a wavefront (a workgroup of 64) per CHAIN of matches -- the matches that hit one empty feature of the
//                 target, or features that carried one id when the pass began -- in list order: the first to hit an empty
//                 feature is added; everybody else replaces the chain's A (the id the features carried, or the point just
//                 added) by itself
// No kernel waits on another workgroup; every loop is bounded by a count read once or by an array's size; every index read
// from device memory is checked against its array; chains read and write disjoint ids and disjoint features.
#include "kfstore.h"

#include "fuse_ops.h"
#include "kf_area.h"
#include "new_points_geom.h"
#include "sim3_compose.h"

namespace {

using namespace vo;
using namespace vo::fuse_ops;

constexpr int kMutateGrid = 256, kSearchGrid = 1024;
constexpr int kThLow = 50;

struct LfArgs {
  FuseArgs A;
  KfLoopFuseView Q;
  const int *corr_kf;    // [n_corr]
  const double *S_corr;  // [n_corr][8]
  const int *list;       // the loop points
};

// the target of a pass, or -1: the call does not run, or the key-frame is outside the store, erased or without a pose
__device__ __forceinline__ int pass_target(const LfArgs &G, int pass) {
  if (G.Q.head[kLfRuns] == 0) return -1;
  const int T = G.corr_kf[pass];
  return target_ready(G.A, T) ? T : -1;
}

__global__ __launch_bounds__(256) void k_lf_begin(LfArgs G, int n_corr, int n_max, const int *loop_state, const int *loop_n) {
  const bool runs = !loop_state || loop_state[kLsState] == VO_KFSTORE_LOOP_ACCEPTED;
  if (threadIdx.x == 0) {
    G.Q.head[kLfPasses] = runs ? n_corr : 0, G.Q.head[kLfRuns] = runs ? 1 : 0;
    G.Q.head[kLfNPoints] = runs ? (loop_n ? min(max(*loop_n, 0), n_max) : n_max) : 0;
    if (!runs) atomicOr(G.A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  }
  if (!runs) return;
  for (int p = threadIdx.x; p < n_corr; p += 256) {
    const int T = G.corr_kf[p];
    int *rec = G.Q.rec + p * kLfRecInts;
    rec[kLfTarget] = T;
    if (!target_ready(G.A, T)) rec[kLfUndone] = 2, atomicOr(G.A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
  }
}

// ---- the gates of a loop point (matcher.cpp:1147-1191) and its best match (:1193-1218)
__global__ __launch_bounds__(256) void k_lf_search(LfArgs G, int pass, int n_max, float threshold) {
  extern __shared__ float4 s_feat[];  // x, y, 0, octave (as int bits)
  const FuseArgs &A = G.A;
  const int T = pass_target(G, pass);
  if (T < 0) return;  // (uniform over the grid)
  const KfStoreView &S = A.S;
  const int NK = S.NK, nT = n_features(S, T), tid = threadIdx.x, lane = tid & 63;
  {
    const float *x = np_x(A.M, T), *y = np_y(A.M, T);
    const int *oc = cull_octave(A.X, T);
    for (int f = tid; f < nT; f += 256) s_feat[f] = make_float4(x[f], y[f], 0.f, __int_as_float(oc[f]));
  }
  __syncthreads();
  const int n = min(max(G.Q.head[kLfNPoints], 0), n_max);
  const float fx = A.M.cam[0], fy = A.M.cam[1], cx = A.M.cam[2], cy = A.M.cam[3];
  const int n_levels = min(max(A.M.n_levels, 1), 16);
  const float log_sf1 = (float)log((double)A.M.sf[1]);
  // Tcw = SE3(R(q), t): the Sim3's translation as it stands (:1144), Ow = -(R^T t)
  double Sm[8], Tp[12], Ow[3];
  s3_load(G.S_corr + 8 * (size_t)pass, Sm);
  s3_matrix(Sm, Tp);
  Tp[9] = Sm[4], Tp[10] = Sm[5], Tp[11] = Sm[6];
  np_center(Tp, Ow);
  int *rec = G.Q.rec + pass * kLfRecInts;
  for (int pos = blockIdx.x * 4 + (tid >> 6); pos < n; pos += (int)gridDim.x * 4) {  // (uniform over the wavefront)
    const int id = G.list[pos];
    if (id < 0) continue;
    const int p = slot_of(A.O, id);
    if (p < 0 || p >= A.F.V.n_slots) continue;  // (no entry when the call began: nobody holds it)
    // `mp->isBad()` and alreadyFound (:1147-1154, :1160): the holders through the overlay; the attributes of the first live carrier
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
    if (z < 0.0f) continue;  // (:1167)
    const float invz = __fdiv_rn(1.0f, z);
    const float xn = __fmul_rn((float)pc[0], invz), yn = __fmul_rn((float)pc[1], invz);
    const float u = __fadd_rn(__fmul_rn(fx, xn), cx), v = __fadd_rn(__fmul_rn(fy, yn), cy);
    if (!(u >= A.F.xmin && v >= A.F.ymin && u < A.F.xmax && v < A.F.ymax)) continue;  // isInImg (:1175)
    double line[3];
    for (int c = 0; c < 3; c++) line[c] = __dadd_rn(pw[c], -Ow[c]);
    const float dist = (float)__dsqrt_rn(np_dot3(line[0], line[0], line[1], line[1], line[2], line[2]));
    const float maxd = kf_sec<float>(S, kk, S.o_maxd)[ff], mind = kf_sec<float>(S, kk, S.o_mind)[ff];
    if (dist < __fmul_rn(0.8f, mind) || dist > __fmul_rn(1.2f, maxd)) continue;  // (:1183)
    const double *pn = A.O.normals + ((size_t)kk * NK + ff) * 3;
    if (np_dot3(line[0], pn[0], line[1], pn[1], line[2], pn[2]) < __dmul_rn(0.5, (double)dist)) continue;  // (:1188)
    const int level = predict_level(maxd, dist, log_sf1, n_levels);  // (:1191)
    const float radius = __fmul_rn(threshold, A.M.sf[level]);
    if (lane == 0) atomicAdd(rec + kLfPassed, 1);
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
      if (oct < level - 1 || oct > level) continue;  // (:1205): no chi-square gate, no u_right
      const uint4 *dd = reinterpret_cast<const uint4 *>(kf_sec<uint8_t>(S, T, S.o_desc)) + 2 * (size_t)f;
      const uint4 da = dd[0], db = dd[1];
      const unsigned long long key = area_key(hamming256(qa, qb, da, db), gx, gy, f);
      best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    if (best == ~0ull || (int)(best >> 44) > kThLow) continue;  // (:1220)
    if (lane == 0) {
      const int f = (int)(best & 0xffffffffu);
      atomicAdd(rec + kLfMatches, 1);
      const int m = atomicAdd(A.F.head + 1, 1);  // (a slot in an unordered list: the chains order it by list position)
      if (m >= 0 && m < A.F.M) {
        // the chain of the match: the id the feature carries as the pass begins, else the feature
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

// ---- the hits of a pass (:1220-1234) and its replaces (loopClosing.cpp:508-513), one chain per wavefront
__global__ __launch_bounds__(64) void k_lf_mutate(LfArgs G, int pass) {
  __shared__ MutateLds L;
  const FuseArgs &A = G.A;
  const int lane = threadIdx.x, NK = A.S.NK;
  const int end = A.F.head[1];
  if (blockIdx.x == 0 && lane == 0) G.Q.base[pass + 1] = end;  // (where the next pass's matches begin)
  const int T = pass_target(G, pass);
  if (T < 0) return;
  const int base = min(max(G.Q.base[pass], 0), A.F.M);
  int *rec = G.Q.rec + pass * kLfRecInts;
  // more candidates passed the gates than a pass takes, or the call's matches do not fit: the pass is left undone
  if (rec[kLfPassed] > A.F.M || end > A.F.M) {
    if (blockIdx.x == 0 && lane == 0) atomicOr(A.status, (int)VO_KFSTORE_FUSE_CAPACITY), rec[kLfUndone] = 1;
    return;
  }
  const KfOverlay &V = A.F.V;
  for (int m0 = base + (int)blockIdx.x; m0 < end; m0 += (int)gridDim.x) {
    const int key = A.F.key[m0], pos0 = A.F.mt[m0].x;
    bool later = false;  // the chain's leader is its first match in list order
    for (int o = base + lane; o < end; o += 64) later |= A.F.key[o] == key && A.F.mt[o].x < pos0;
    if (__ballot(later) != 0ull) continue;
    // the chain's A: what its features carried when the pass began; on an empty feature the leader, once it is added
    int idA = -1, pA = -1;
    bool add_first = false;
    {
      const int f0 = A.F.mt[m0].w;
      if (f0 >= 0 && f0 < NK) {
        const unsigned e0 = (unsigned)T * (unsigned)NK + (unsigned)f0;
        const int org = *id_word(A.S, e0);
        if ((*flag_byte(A.S, e0) & 1) && org >= 0) idA = org, pA = slot_of(A.O, org);
        else add_first = true;
      }
    }
    int cur = m0;
    for (int guard = base; cur >= 0 && guard < end; guard++) {
      const int4 mt = A.F.mt[cur];
      const int mp = mt.y, p_mp = mt.z, f = mt.w;
      if (p_mp >= 0 && p_mp < V.n_slots && f >= 0 && f < NK) {
        const unsigned eT = (unsigned)T * (unsigned)NK + (unsigned)f;
        const int nb0 = collect(A, mp, p_mp, L.b);
        bool held = false;
        for (int c = lane; c < min(nb0, kMaxC); c += 64) held |= (int)(L.b[c] / (unsigned)NK) == T;
        if (nb0 == 0 || __ballot(held) != 0ull) {
          // (a loop point that passed is not held by the target and has a holder: nothing to do here)
        } else if (cur == m0 && add_first) {  // addObservation + addMapPoint at once (:1229-1232)
          const unsigned src = lowest_of(L.b, nb0);
          if (lane == 0) {
            const Attr a = attr_of(A, src);
            take(A, eT, mp, a);
            uint8_t *fb = flag_byte(A.S, eT);
            *fb = (uint8_t)(*fb | 1);
            V.node_entry[cur] = (int)eT, V.node_next[cur] = V.a_head[p_mp], V.a_head[p_mp] = cur + 1;
            atomicAdd(rec + kLfAdds, 1);
          }
          idA = mp, pA = p_mp;
        } else {  // replace[i] = A (:1224-1227), then A->replaceMapPoint(loop point) (loopClosing.cpp:508-513)
          if (lane == 0) atomicAdd(rec + kLfReplaces, 1);
          if (idA != mp) {
            const bool slot_ok = pA >= 0 && pA < V.n_slots;
            const int na0 = slot_ok ? collect(A, idA, pA, L.a) : 0;  // (0: a former replace of the chain emptied A; not skipped)
            if (na0 > kMaxC || nb0 > kMaxC || !slot_ok) {
              if (lane == 0) atomicOr(A.status, (int)VO_KFSTORE_FUSE_CAPACITY);
            } else {
              classify(A, L.a, na0, L.ca), classify(A, L.b, nb0, L.cb);
              int moved, cleared;
              replace_carriers(A, L, idA, mp, pA, p_mp, na0, nb0, moved, cleared);
              if (lane == 0) {
                if (moved) atomicAdd(rec + kLfMoved, 1);
                if (cleared) atomicAdd(rec + kLfCleared, cleared);
              }
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

// head | base [C + 1] | rec [C][8] -- what a call resets -- then `in`: S_corr [C][8] | corr_kf [C] | ids [P]
size_t lf_layout(uint8_t *block, int C, int P, KfLoopFuseView &Q) {
  size_t at = 0;
  auto take = [&](auto *&field, size_t count) {
    using T = std::remove_reference_t<decltype(*field)>;
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += up16(count * sizeof(T));
  };
  take(Q.head, 4), take(Q.base, (size_t)C + 1), take(Q.rec, (size_t)C * kLfRecInts);
  Q.reset_bytes = at;
  const size_t in0 = at;
  take(Q.S_corr, (size_t)C * 8), take(Q.corr_kf, (size_t)C), take(Q.ids, (size_t)P);
  Q.in_bytes = at - in0, Q.C = C, Q.P = P;
  return at;
}

FuseArgs lf_fuse_args(vo_kfstore *s, const KfObsView &O) {
  const KfConnView C = connections_view(s->conn);
  return FuseArgs{kfstore_view(s), O, C, s->X, s->M, s->B, s->U, s->F, s->normals.as<double>(), C.status};
}

// the call: the index rebuilt when stale, three memsets (the call's records, the overlay, the match count), k_lf_begin, then
// two launches per pass.  n_max bounds the list; loop_state / loop_n: the _loop form's words in compute_sim3's block.
int lf_enqueue(vo_kfstore *s, int n_corr, const int *dev_corr_kf, const double *dev_S_corr, int n_max, const int *dev_list,
               const int *loop_state, const int *loop_n, float threshold) {
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // the index the overlay stands on
  const LfArgs G{lf_fuse_args(s, O), s->Q, dev_corr_kf, dev_S_corr, dev_list};
  const KfFuseView &F = s->F;
  hipStream_t st = s->st;
  VO_HIP_CHECK(hipMemsetAsync(s->Q.head, 0, s->Q.reset_bytes, st));
  // the overlay (m_next, m_tail, a_head: side by side up to the end of what a fuse call resets) and the match count; the
  // record of the last fuse call (vo_kfstore_fuse_result) stays
  VO_HIP_CHECK(hipMemsetAsync(F.V.m_next, 0, (size_t)(reinterpret_cast<uint8_t *>(F.head) + F.reset_bytes - reinterpret_cast<uint8_t *>(F.V.m_next)), st));
  VO_HIP_CHECK(hipMemsetAsync(F.head + 1, 0, 4, st));
  hipLaunchKernelGGL(k_lf_begin, dim3(1), dim3(256), 0, st, G, n_corr, n_max, loop_state, loop_n);
  if (n_max > 0) {
    const int blocks = std::min((n_max + 3) / 4, kSearchGrid);
    for (int pass = 0; pass < n_corr; pass++) {
      hipLaunchKernelGGL(k_lf_search, dim3((unsigned)blocks), dim3(256), (size_t)s->NK * sizeof(float4), st, G, pass, n_max, threshold);
      hipLaunchKernelGGL(k_lf_mutate, dim3(kMutateGrid), dim3(64), 0, st, G, pass);
    }
  }
  VO_HIP_CHECK(hipGetLastError());
  s->obs_dirty = true, s->gen++;  // (whether anything matched only the device knows)
  return VO_OK;
}

// a call's head: the layer and the counts against what it was enabled for
int lf_check(const vo_kfstore *s, const char *W, unsigned layers, int n_corr, const void *corr_kf, const void *S_corr, int n_points,
             const void *ids, int max_points, float threshold) {
  VO_CHECK(need(s, W, layers));
  if (n_corr < 0 || n_points < 0 || (n_corr > 0 && (!corr_kf || !S_corr)) || (n_points > 0 && !ids) || !(threshold > 0.f))
    return VO_ERR_INVALID;
  if (n_corr > s->Q.C || n_points > max_points) {
    set_error("%s: %d corrected key-frames, %d loop points; the store was enabled for %d, %d", W, n_corr, n_points, s->Q.C, max_points);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_loop_fuse(vo_kfstore *s, int max_corrected, int max_loop_points) {
  const char *W = "vo_kfstore_enable_loop_fuse";
  if (const int rc = enable_begin(s, W, kLayerFuse, kLayerLoopFuse, max_corrected >= 1 && max_loop_points >= 1)) return rc < 0 ? rc : VO_OK;
  KfLoopFuseView Q{};
  const size_t bytes = lf_layout(nullptr, max_corrected, max_loop_points, Q);
  VO_CHECK(s->lf.reserve(bytes));
  lf_layout(s->lf.as<uint8_t>(), max_corrected, max_loop_points, s->Q);
  VO_CHECK(s->lf_stage.reserve(std::max(s->Q.in_bytes, s->Q.reset_bytes)));
  VO_HIP_CHECK(hipMemsetAsync(s->lf.p, 0, bytes, s->st));
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerLoopFuse;
  return VO_OK;
}

int vo_kfstore_search_and_fuse_dev(vo_kfstore *s, int n_corr, const int32_t *dev_corr_kf, const double *dev_S_corr, int n_points,
                                   const int32_t *dev_ids, float threshold) {
  const char *W = "vo_kfstore_search_and_fuse_dev";
  VO_CHECK(lf_check(s, W, kLayerLoopFuse, n_corr, dev_corr_kf, dev_S_corr, n_points, dev_ids, s ? s->Q.P : 0, threshold));
  return lf_enqueue(s, n_corr, dev_corr_kf, dev_S_corr, n_points, dev_ids, nullptr, nullptr, threshold);
}

int vo_kfstore_search_and_fuse(vo_kfstore *s, int n_corr, const int32_t *corr_kf, const double *S_corr, int n_points, const int32_t *ids,
                               float threshold) {
  const char *W = "vo_kfstore_search_and_fuse";
  VO_CHECK(lf_check(s, W, kLayerLoopFuse, n_corr, corr_kf, S_corr, n_points, ids, s ? s->Q.P : 0, threshold));
  for (int r = 1; r < n_corr; r++)
    if (corr_kf[r - 1] >= corr_kf[r]) {
      set_error("%s: corrected key-frame %d (entry %d) not in ascending order", W, corr_kf[r], r);
      return VO_ERR_INVALID;
    }
  // one copy: S_corr | corr_kf | ids land on the block's `in`, which keeps them side by side
  const KfLoopFuseView &Q = s->Q;
  uint8_t *up = s->lf_stage.data(), *in = reinterpret_cast<uint8_t *>(Q.S_corr);
  const size_t o_kf = (size_t)(reinterpret_cast<uint8_t *>(Q.corr_kf) - in), o_ids = (size_t)(reinterpret_cast<uint8_t *>(Q.ids) - in);
  if (n_corr > 0) memcpy(up, S_corr, (size_t)n_corr * 64), memcpy(up + o_kf, corr_kf, (size_t)n_corr * 4);
  if (n_points > 0) memcpy(up + o_ids, ids, (size_t)n_points * 4);
  VO_CHECK(copy_h2d(in, up, o_ids + (size_t)n_points * 4, s->st, W));
  VO_CHECK(lf_enqueue(s, n_corr, Q.corr_kf, Q.S_corr, n_points, Q.ids, nullptr, nullptr, threshold));
  return stream_sync(s->st, W);
}

int vo_kfstore_search_and_fuse_loop(vo_kfstore *s, int n_corr, const int32_t *dev_corr_kf, const double *dev_S_corr, float threshold) {
  const char *W = "vo_kfstore_search_and_fuse_loop";
  VO_CHECK(lf_check(s, W, kLayerLoopFuse | kLayerLoop, n_corr, dev_corr_kf, dev_S_corr, 0, nullptr, 0, threshold));
  // loopConnectKFMapPoints_ where the last compute_sim3 left it, read in place; its length and the state are the device's
  return lf_enqueue(s, n_corr, dev_corr_kf, dev_S_corr, s->L.P, s->L.loop_ids, s->L.st, s->L.st + kLsNLoop, threshold);
}

int vo_kfstore_loop_fuse_result(vo_kfstore *s, int32_t *record, int32_t *per_pass) {
  const char *W = "vo_kfstore_loop_fuse_result";
  VO_CHECK(need(s, W, kLayerLoopFuse));
  const KfLoopFuseView &Q = s->Q;
  uint8_t *down = s->lf_stage.data();
  VO_CHECK(copy_d2h(down, Q.head, Q.reset_bytes, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int32_t *head = reinterpret_cast<const int32_t *>(down);
  const int32_t *rec = reinterpret_cast<const int32_t *>(down + (reinterpret_cast<uint8_t *>(Q.rec) - reinterpret_cast<uint8_t *>(Q.head)));
  const int n = std::min(std::max(head[kLfPasses], 0), Q.C);
  int32_t out[8] = {n, 0, 0, 0, 0, 0, 0, 0};
  if (per_pass) memset(per_pass, 0, (size_t)Q.C * 6 * 4);
  for (int p = 0; p < n; p++)
    for (int c = 0; c < 6; c++) {
      const int32_t v = rec[p * kLfRecInts + 1 + c];
      out[1 + c] += v;
      if (per_pass) per_pass[p * 6 + c] = v;
    }
  if (record) memcpy(record, out, sizeof(out));
  return VO_OK;
}

}  // extern "C"
