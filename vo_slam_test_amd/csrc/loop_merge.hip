// loop_merge.hip -- the merge of the loop matches on the device: the loop of LoopClosing::correctLoop that
// gives the current key-frame the loop's map points (loopClosing.cpp:439-455) -- MapPoint::replaceMapPoint (mappoint.cpp:214-253)
// where the feature has a point, addObservation + addMapPoint + computeDescriptor (:450-452) where it has none -- driven by a
// feature-to-point list instead of a search, on section 4m's overlay and fuse_ops.h; and the composed vo_kfstore_correct_loop, a
// fixed sequence of the store's entry points with no kernel of its own.
//   k_merge_begin    one thread: does the call run (the _loop form reads compute_sim3's state), `curr`, the number of steps
//   k_merge_plan     ONE workgroup: the id a feature carries as the call begins (A0) next to its match (B); the at most
//                    2 * max_features ids sorted in LDS with their step; a step one of whose ids stands beside the same id of
//                    ANOTHER step is ORDERED, every other step ALONE; the ordered steps' features as an ascending list
//   k_merge_alone    a workgroup of 64 per feature of `curr`; one whose feature has no ALONE step returns at its first load.
//                    An alone step shares no id with any other step, so it finds the state the call began with in everything
//                    it reads, and what it writes nobody else reads (section 4s, the derivation)
//   k_merge_ordered  ONE workgroup of 64 behind it: the ordered steps in feature order, each re-reading its feature, a workgroup
//                    barrier between steps
// Both run merge_step.  No kernel waits on another workgroup; every loop is bounded by a count read once or by an array's size;
// every index read from device memory is checked against its array; both overlay chains are cut after as many links as they
// have entries (obs_walk.h); the atomics are integer sums and the sticky word's bits; every grid is fixed by max_features.
#include "kfstore.h"

#include "block_sort.h"
#include "fuse_ops.h"

#include <algorithm>

namespace {

using namespace vo;
using namespace vo::fuse_ops;

constexpr int kPlanThreads = 1024;

struct MgArgs {
  FuseArgs A;  // (A.F.V: the fusion layer's slots with THIS layer's nodes, one per feature of curr)
  KfLoopMergeView G;
  const int *list;  // match_ids
};

// ---- the head of a call.  loop_state: NULL, or compute_sim3's state words (the _loop form: `curr`, the verdict and the length
// of the list are the device's)
__global__ void k_merge_begin(MgArgs M, int curr, int n, const int *loop_state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool accepted = !loop_state || loop_state[kLsState] == VO_KFSTORE_LOOP_ACCEPTED;
  const int cur = loop_state ? loop_state[kLsCurrent] : curr;
  const int len = loop_state ? loop_state[kLsNCur] : n;
  const bool runs = accepted && cur >= 0 && cur < M.A.S.size && !M.A.X.erased[cur];
  M.G.head[kMgRuns] = runs ? 1 : 0, M.G.head[kMgCurr] = cur;
  M.G.head[kMgN] = runs ? min(max(len, 0), n_features(M.A.S, cur)) : 0;
  M.G.rec[kMgRecCurr] = cur;
  if (!runs) atomicOr(M.A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
}

// exclusive prefix of `flag` over the workgroup in thread order; *total = the workgroup's sum
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

// ---- which steps share an id: keys (id << 32 | step), two per step, sorted; np2 = the power of two >= 2 * max_features
__global__ __launch_bounds__(kPlanThreads) void k_merge_plan(MgArgs M, int np2) {
  extern __shared__ unsigned long long s_keys[];
  __shared__ int s_w[kPlanThreads / 64];
  const KfLoopMergeView &G = M.G;
  const int tid = threadIdx.x, NK = M.A.S.NK;
  const int n = min(max(G.head[kMgN], 0), NK), cur = G.head[kMgCurr];
  if (!G.head[kMgRuns] || n == 0) return;  // (uniform)
  for (int i = tid; 2 * i < np2; i += kPlanThreads) {
    unsigned long long kb = ~0ull, ka = ~0ull;
    if (i < n) {
      const int B = M.list[i];
      if (B >= 0) {
        const unsigned e = (unsigned)cur * (unsigned)NK + (unsigned)i;
        const int A0 = *id_word(M.A.S, e);
        kb = ((unsigned long long)(unsigned)B << 32) | (unsigned)i;
        if ((*flag_byte(M.A.S, e) & 1) && A0 >= 0) ka = ((unsigned long long)(unsigned)A0 << 32) | (unsigned)i;
        G.kind[i] = kMgAlone;
      }
    }
    s_keys[2 * i] = kb, s_keys[2 * i + 1] = ka;
  }
  __threadfence_block();
  block_bitonic_sort(s_keys, np2);
  for (int pos = tid; pos < np2; pos += kPlanThreads) {
    const unsigned long long k = s_keys[pos];
    if (k == ~0ull) continue;
    const unsigned id = (unsigned)(k >> 32), step = (unsigned)k;
    bool shared = false;
    if (pos > 0) {
      const unsigned long long o = s_keys[pos - 1];
      shared |= (unsigned)(o >> 32) == id && (unsigned)o != step;
    }
    if (pos + 1 < np2) {
      const unsigned long long o = s_keys[pos + 1];
      shared |= o != ~0ull && (unsigned)(o >> 32) == id && (unsigned)o != step;
    }
    if (shared && step < (unsigned)n) G.kind[step] = kMgOrdered;  // (every writer writes the same value)
  }
  __threadfence_block();
  __syncthreads();
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += kPlanThreads) {
    const int i = i0 + tid;
    const bool in = i < n && G.kind[i] == kMgOrdered;
    int total;
    const int pos = base + block_rank(in, s_w, &total);
    if (in && pos < NK) G.ordered[pos] = i;
    base += total;
  }
  if (tid == 0) G.head[kMgNOrdered] = base;
}

// ---- one step (loopClosing.cpp:443-454) by one wavefront that is a workgroup; uniform over the wavefront
__device__ void merge_step(const MgArgs &M, MutateLds &L, int i, bool on_ordered_path) {
  const FuseArgs &A = M.A;
  const KfLoopMergeView &G = M.G;
  const KfOverlay &V = A.F.V;
  const int lane = threadIdx.x & 63, NK = A.S.NK;
  const int cur = G.head[kMgCurr];
  if (i < 0 || i >= NK || cur < 0 || cur >= A.S.size) return;
  const int B = M.list[i];
  if (B < 0) return;
  const unsigned eT = (unsigned)cur * (unsigned)NK + (unsigned)i;
  const int idA = *id_word(A.S, eT);
  const bool has = (*flag_byte(A.S, eT) & 1) && idA >= 0;
  int branch;
  if (has && idA == B) {
    branch = kMgBrNoop;  // replaceMapPoint returns at once (mappoint.cpp:216)
  } else {
    const int pB = slot_of(A.O, B);
    const bool b_ok = pB >= 0 && pB < V.n_slots;
    const int nb = b_ok ? collect(A, B, pB, L.b) : 0;
    if (nb == 0) {
      branch = kMgBrDead;  // nobody holds B: it has no attributes to restate
    } else if (has) {      // A->replaceMapPoint(B) (:445-447)
      const int pA = slot_of(A.O, idA);
      const bool a_ok = pA >= 0 && pA < V.n_slots;
      const int na = a_ok ? collect(A, idA, pA, L.a) : 0;
      if (!a_ok || na > kMaxC || nb > kMaxC) {
        branch = kMgBrUndone;
        if (lane == 0) atomicOr(A.status, (int)VO_KFSTORE_FUSE_CAPACITY);
      } else {
        branch = kMgBrReplace;
        classify(A, L.a, na, L.ca), classify(A, L.b, nb, L.cb);
        int moved, cleared;
        replace_carriers(A, L, idA, B, pA, pB, na, nb, moved, cleared);
        if (lane == 0) {
          if (moved) atomicAdd(G.rec + kMgMoved, 1);
          if (cleared) atomicAdd(G.rec + kMgCleared, cleared);
        }
      }
    } else {  // addObservation + addMapPoint (:450-451): B's attributes from its lowest live carrier, the node of this feature
      branch = kMgBrAdd;
      const unsigned src = lowest_of(L.b, nb);
      if (lane == 0) {
        const Attr a = attr_of(A, src);
        take(A, eT, B, a);
        uint8_t *fb = flag_byte(A.S, eT);
        *fb = (uint8_t)(*fb | 1);
        V.node_entry[i] = (int)eT, V.node_next[i] = V.a_head[pB], V.a_head[pB] = i + 1;
      }
      __threadfence_block();
      __syncthreads();
      const int nb1 = collect(A, B, pB, L.b);  // computeDescriptor (:452) over B's carriers with the new one
      if (nb1 > kMaxC) {
        if (lane == 0) atomicOr(A.status, (int)VO_KFSTORE_UPKEEP_CAPACITY);  // (the point keeps its descriptor)
      } else {
        classify(A, L.b, nb1, L.cb);
        descriptor_of(A, L, 0, nb1);
      }
    }
  }
  if (lane == 0) {
    G.branch[i] = branch;
    atomicAdd(G.rec + kMgSteps, 1);
    if (on_ordered_path) atomicAdd(G.rec + kMgOrderedSteps, 1);
    atomicAdd(G.rec + (branch == kMgBrAdd ? kMgAdds : branch == kMgBrNoop ? kMgNoops : branch == kMgBrDead ? kMgDead : kMgReplaces), 1);
    if (branch == kMgBrUndone) atomicAdd(G.rec + kMgUndone, 1);
  }
}

__global__ __launch_bounds__(64) void k_merge_alone(MgArgs M) {
  __shared__ MutateLds L;
  const int i = (int)blockIdx.x;
  if (i >= M.A.S.NK || M.G.kind[i] != kMgAlone) return;
  if (i >= M.G.head[kMgN]) return;
  merge_step(M, L, i, false);
}

__global__ __launch_bounds__(64) void k_merge_ordered(MgArgs M) {
  __shared__ MutateLds L;
  const int n = min(max(M.G.head[kMgNOrdered], 0), M.A.S.NK), n_steps = M.G.head[kMgN];
  for (int t = 0; t < n; t++) {
    const int i = M.G.ordered[t];
    if (i >= 0 && i < n_steps) merge_step(M, L, i, true);
    __threadfence_block();
    __syncthreads();
  }
}

// head | rec | branch -- what a result fetches -- | kind | ordered | node_entry | node_next -- what a call resets -- | ids
size_t mg_layout(uint8_t *block, int NK, KfLoopMergeView &G) {
  size_t at = 0;
  auto take = [&](int *&field, size_t count) {
    field = block ? reinterpret_cast<int *>(block + at) : nullptr;
    at += up16(count * sizeof(int));
  };
  const size_t nk = (size_t)NK;
  take(G.head, 4), take(G.rec, kMgRecInts), take(G.branch, nk), take(G.kind, nk), take(G.ordered, nk), take(G.node_entry, nk), take(G.node_next, nk);
  G.reset_bytes = at;
  take(G.ids, nk);
  G.NK = NK;
  return at;
}

size_t mg_result_bytes(const KfLoopMergeView &G) {
  return (size_t)(reinterpret_cast<uint8_t *>(G.kind) - reinterpret_cast<uint8_t *>(G.head));
}

// the call: the index rebuilt when stale, two memsets (the plan, the overlay), four launches
int mg_enqueue(vo_kfstore *s, int curr, int n, const int *dev_list, const int *loop_state) {
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // the index the overlay stands on
  const KfConnView C = connections_view(s->conn);
  MgArgs M{FuseArgs{kfstore_view(s), O, C, s->X, s->M, s->B, s->U, s->F, s->normals.as<double>(), C.status}, s->G, dev_list};
  KfFuseView &F = M.A.F;
  F.V.node_entry = s->G.node_entry, F.V.node_next = s->G.node_next, F.V.n_nodes = s->NK;
  hipStream_t st = s->st;
  VO_HIP_CHECK(hipMemsetAsync(s->G.head, 0, s->G.reset_bytes, st));
  // the overlay (m_next, m_tail, a_head: side by side up to the end of what a fuse call resets); the match list and the records
  // of the last fuse and search_and_fuse calls stay
  VO_HIP_CHECK(hipMemsetAsync(F.V.m_next, 0, (size_t)(reinterpret_cast<uint8_t *>(F.head) + F.reset_bytes - reinterpret_cast<uint8_t *>(F.V.m_next)), st));
  const int np2 = pow2_ceil(std::max(2 * s->NK, 2));
  hipLaunchKernelGGL(k_merge_begin, dim3(1), dim3(64), 0, st, M, curr, n, loop_state);
  hipLaunchKernelGGL(k_merge_plan, dim3(1), dim3(kPlanThreads), (size_t)np2 * 8, st, M, np2);
  hipLaunchKernelGGL(k_merge_alone, dim3((unsigned)s->NK), dim3(64), 0, st, M);
  hipLaunchKernelGGL(k_merge_ordered, dim3(1), dim3(64), 0, st, M);
  VO_HIP_CHECK(hipGetLastError());
  s->obs_dirty = true, s->gen++;  // (what the steps did only the device knows)
  return VO_OK;
}

int mg_check(const vo_kfstore *s, const char *W, unsigned layers, int n, const void *ids) {
  VO_CHECK(need(s, W, layers));
  if (n < 0 || (n > 0 && !ids)) return VO_ERR_INVALID;
  if (n > s->NK) {
    set_error("%s: %d entries, a key-frame of this store has at most %d features", W, n, s->NK);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

enum { kOk = VO_KFSTORE_BA_WINDOW_OK, kEmpty = VO_KFSTORE_BA_WINDOW_EMPTY, kOverflow = VO_KFSTORE_BA_WINDOW_OVERFLOW };
enum { kClCurr = 0, kClMatch, kClNCorr, kClNCp, kClNLc, kClMergeAdds, kClMergeReplaces, kClFuseAdds, kClFuseReplaces, kClNNodes, kClNEdges,
       kClNMoved, kClStop };

}  // namespace

extern "C" {

int vo_kfstore_enable_loop_merge(vo_kfstore *s) {
  const char *W = "vo_kfstore_enable_loop_merge";
  if (const int rc = enable_begin(s, W, kLayerLoopFuse, kLayerLoopMerge)) return rc < 0 ? rc : VO_OK;
  KfLoopMergeView G{};
  const size_t bytes = mg_layout(nullptr, s->NK, G);
  VO_CHECK(s->lm.reserve(bytes));
  mg_layout(s->lm.as<uint8_t>(), s->NK, s->G);
  // the host form's list going up; a result coming down; the composed call's reads: three records, the sticky word, the fusion's
  VO_CHECK(s->lm_stage.reserve(std::max(mg_result_bytes(s->G), (size_t)288 + s->Q.reset_bytes)));
  VO_HIP_CHECK(hipMemsetAsync(s->lm.p, 0, bytes, s->st));
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerLoopMerge;
  return VO_OK;
}

int vo_kfstore_merge_loop_matches_dev(vo_kfstore *s, int curr, int n, const int32_t *dev_match_ids) {
  const char *W = "vo_kfstore_merge_loop_matches_dev";
  VO_CHECK(mg_check(s, W, kLayerLoopMerge, n, dev_match_ids));
  return mg_enqueue(s, curr, n, dev_match_ids ? dev_match_ids : s->G.ids, nullptr);
}

int vo_kfstore_merge_loop_matches(vo_kfstore *s, int curr, int n, const int32_t *match_ids) {
  const char *W = "vo_kfstore_merge_loop_matches";
  VO_CHECK(mg_check(s, W, kLayerLoopMerge, n, match_ids));
  if (n > 0) {
    memcpy(s->lm_stage.data(), match_ids, (size_t)n * 4);
    VO_CHECK(copy_h2d(s->G.ids, s->lm_stage.data(), (size_t)n * 4, s->st, W));  // the one copy
  }
  VO_CHECK(mg_enqueue(s, curr, n, s->G.ids, nullptr));
  return stream_sync(s->st, W);
}

int vo_kfstore_merge_loop_matches_loop(vo_kfstore *s) {
  const char *W = "vo_kfstore_merge_loop_matches_loop";
  VO_CHECK(need(s, W, kLayerLoopMerge | kLayerLoop));
  // `current`, the verdict, matchMapPoints_ and its length where the last compute_sim3 left them, read in place
  return mg_enqueue(s, -1, s->NK, s->L.match_ids, s->L.st);
}

int vo_kfstore_loop_merge_result(vo_kfstore *s, int32_t *record, int32_t *per_feature) {
  const char *W = "vo_kfstore_loop_merge_result";
  VO_CHECK(need(s, W, kLayerLoopMerge));
  const KfLoopMergeView &G = s->G;
  uint8_t *down = s->lm_stage.data();
  VO_CHECK(copy_d2h(down, G.head, mg_result_bytes(G), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  auto staged = [&](const int *dev) { return reinterpret_cast<const int32_t *>(down + (reinterpret_cast<const uint8_t *>(dev) - reinterpret_cast<const uint8_t *>(G.head))); };
  if (record) memcpy(record, staged(G.rec), kMgRecInts * 4);
  if (per_feature) memcpy(per_feature, staged(G.branch), (size_t)s->NK * 4);
  return VO_OK;
}

// LoopClosing::correctLoop from :364 to :485 on the state the last compute_sim3 left: a fixed sequence of the store's entry
// points (include/vo_hip.h), three small reads between them
int vo_kfstore_correct_loop(vo_kfstore *s, float threshold, int max_iterations, vo_lm_summary *summary, int32_t *record) {
  const char *W = "vo_kfstore_correct_loop";
  VO_CHECK(need(s, W, kLayerLoopMerge | kLayerLoop | kLayerLoopCorrect));
  if (s->size == 0 || !(threshold > 0.f)) return VO_ERR_INVALID;
  int32_t out[16] = {0};
  auto stop = [&](int step, int rc) {
    out[kClStop] = step;
    if (record) memcpy(record, out, sizeof(out));
    return rc;
  };
  const KfLoopCorrectView &R = s->R;
  const int *sticky = connections_view(s->conn).status;
  uint8_t *down = s->lm_stage.data();
  const int32_t *lc = reinterpret_cast<const int32_t *>(down), *mg = lc + 16, *ls = lc + 32, *word = lc + 64, *lf = lc + 68;
  int rc;
  if ((rc = vo_kfstore_propagate_loop_sim3(s)) != VO_OK) return stop(1, rc);      // 1. (:364-437)
  if ((rc = vo_kfstore_merge_loop_matches_loop(s)) != VO_OK) return stop(2, rc);  // 2. (:439-455)
  // 3. the first read: the propagation's record, the merge's, compute_sim3's state words and the sticky word (not cleared)
  VO_CHECK(copy_d2h(down, R.rec, kLcRecInts * 4, s->st, W));
  VO_CHECK(copy_d2h(down + 64, s->G.rec, kMgRecInts * 4, s->st, W));
  VO_CHECK(copy_d2h(down + 128, s->L.st, kLoopStateInts * 4, s->st, W));
  VO_CHECK(copy_d2h(down + 256, sticky, 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int curr = ls[kLsCurrent], match = ls[kLsMatchKf];
  out[kClCurr] = curr, out[kClMatch] = match, out[kClNCorr] = lc[kLcNCorr], out[kClNCp] = lc[kLcNCp];
  out[kClMergeAdds] = mg[kMgAdds], out[kClMergeReplaces] = mg[kMgReplaces];
  if (ls[kLsState] != VO_KFSTORE_LOOP_ACCEPTED) {
    set_error("%s: the last compute_sim3 did not accept a loop", W);
    return stop(1, VO_ERR_INVALID);
  }
  if (lc[kLcStatus] != kOk) {
    set_error("%s: the propagation is %s", W, lc[kLcStatus] == kOverflow ? "overflowed" : "empty");
    return stop(1, lc[kLcStatus] == kOverflow ? VO_ERR_CAPACITY : VO_ERR_INVALID);
  }
  if (word[0] & VO_KFSTORE_FUSE_CAPACITY) {
    set_error("%s: VO_KFSTORE_FUSE_CAPACITY stands after the merge (%d replaces left undone)", W, mg[kMgUndone]);
    return stop(2, VO_ERR_CAPACITY);
  }
  const int n_corr = lc[kLcNCorr], n_cp = lc[kLcNCp];
  if ((rc = vo_kfstore_search_and_fuse_loop(s, n_corr, R.corr_kf, R.S_corr, threshold)) != VO_OK) return stop(4, rc);  // 4. (:458)
  if ((rc = vo_kfstore_loop_connections(s)) != VO_OK) return stop(5, rc);                                               // 5. (:461-479)
  // 6. the second read: the record again, the sticky word, the fusion's per-pass records
  VO_CHECK(copy_d2h(down, R.rec, kLcRecInts * 4, s->st, W));
  VO_CHECK(copy_d2h(down + 256, sticky, 4, s->st, W));
  VO_CHECK(copy_d2h(down + 272, s->Q.head, s->Q.reset_bytes, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  {
    const int32_t *rec = lf + (s->Q.rec - s->Q.head);
    for (int p = 0; p < std::min(std::max(lf[kLfPasses], 0), s->Q.C); p++)
      out[kClFuseAdds] += rec[p * kLfRecInts + kLfAdds], out[kClFuseReplaces] += rec[p * kLfRecInts + kLfReplaces];
  }
  out[kClNLc] = lc[kLcNLc];
  if (word[0] & VO_KFSTORE_FUSE_CAPACITY) {
    set_error("%s: VO_KFSTORE_FUSE_CAPACITY stands after the fusion", W);
    return stop(4, VO_ERR_CAPACITY);
  }
  if (lc[kLcConnStatus] != kOk) {
    set_error("%s: the loop connections are %s", W, lc[kLcConnStatus] == kOverflow ? "overflowed" : "empty");
    return stop(5, lc[kLcConnStatus] == kOverflow ? VO_ERR_CAPACITY : VO_ERR_INVALID);
  }
  const int n_lc = lc[kLcNLc];
  // 7. the window on the layer's device arrays, then vo_kfstore_pose_graph's tail
  if ((rc = vo_kfstore_pose_graph_window_dev(s, curr, match, n_corr, R.corr_kf, R.S_corr, R.S_unc, R.lc_start, n_lc, R.lc_kf, n_cp, R.cp_id,
                                             R.cp_ref)) != VO_OK)
    return stop(7, rc);
  const KfPgView &P = s->P;
  const KfWindow &win = s->pg_win;
  VO_CHECK(s->pg_win.fetch(P.win, P.win_bytes, false, s->st, W));  // the third read: the window
  const int32_t *r = win.rec;
  out[kClNNodes] = r[kPgNNodes], out[kClNEdges] = r[kPgNEdges];
  if (r[kPgStatus] == VO_KFSTORE_BA_WINDOW_OVERFLOW) {
    set_error("%s: %d nodes, %d edges; the solver takes %d nodes and the store was enabled for %d edges", W, r[kPgNNodes], r[kPgNEdges],
              P.max_nodes, P.max_edges);
    return stop(7, VO_ERR_CAPACITY);
  }
  if (r[kPgStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    set_error("%s: the window is empty", W);
    return stop(7, VO_ERR_INVALID);
  }
  const size_t nn = (size_t)r[kPgNNodes];
  memcpy(s->pg_q.data(), win.staged(P.quats, P.win), nn * 32), memcpy(s->pg_t.data(), win.staged(P.trans, P.win), nn * 24);
  // whatever the solver refuses is returned and nothing is written back (section 4o's rule)
  if ((rc = vo_pose_graph_solve((int)nn, s->pg_q.data(), s->pg_t.data(), win.staged(P.scales, P.win), r[kPgFixed], r[kPgNEdges],
                                win.staged(P.e_i, P.win), win.staged(P.e_j, P.win), win.staged(P.q_meas, P.win), win.staged(P.t_meas, P.win),
                                win.staged(P.s_meas, P.win), s->loop_fix_scale, max_iterations, summary)) != VO_OK)
    return stop(7, rc);
  if ((rc = vo_kfstore_pose_graph_apply(s, s->pg_q.data(), s->pg_t.data())) != VO_OK) return stop(7, rc);
  if ((rc = vo_kfstore_add_loop_edge(s, curr, match)) != VO_OK) return stop(8, rc);  // 8. (:484-485)
  if (record) {  // the apply's count: one more small read, for a caller who asks for the record
    VO_CHECK(copy_d2h(down, P.rec, kPgRecInts * 4, s->st, W));
    VO_CHECK(stream_sync(s->st, W));
    out[kClNMoved] = lc[kPgNMoved];
  }
  return stop(0, VO_OK);
}

}  // extern "C"
