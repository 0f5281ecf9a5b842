// detect_loop.hip -- LoopClosing::detectLoop (reference src/loopClosing.cpp:52-175) from the key-frame store and the key-frame
// database, on the device, the erase locks of the loop thread (keyframe.cpp:541-557), and one iteration of
// LoopClosing::run (:17-37) composed from the store's entry points.  Six launches per detect_loop call:
//   k_dl_begin        ONE workgroup: the lock of `current` (:59), the gate (:62), the pair that makes `current`'s row of the
//                     database the query, conn (the ordered list without the bad key-frames, in list order, :72-76) and excl
//                     (the weight row's non-zero entries and `current`, map.cpp:212-215), both compacted with ballots and a
//                     prefix over the workgroup's waves
//   k_dl_neighbors    a thread per key-frame: the store's graph rows into the database's neighbour rows (map.cpp:284)
//   (k_kfdb_min_score, k_kfdb_query<loop>, kfdb.hip: kfdb_query_loop_on -- minScore and Map::detectLoopCandidates, unchanged)
//   k_dl_groups       a wavefront per candidate slot: the candidate's weight row turned into a bitset over key-frames with
//                     __ballot, its own bit set, ANDed against every previous group: one byte consist[c][j] each
//   k_dl_resolve      ONE wavefront: the reference's double loop (:108-163) over those bytes as written -- every lane runs the same
//                     sequence, the lanes share the copy of a pushed group's bitset -- then the counts, the enough list, the record
//                     and the lock release.  A sequence over at most D x G bytes; not meant to be fast.
//   k_dl_release      vo_kfstore_release_loop_locks: computeSim3's releases (:290-296, :331-346) by the state it ended in
// A call that is gated or whose `current` is erased leaves an EMPTY query pair behind: the two database kernels then find
// nothing, and the kernels of this file behind k_dl_begin return at their first load.  Every loop is bounded by a count read once and clamped
// to its array, every key-frame number read from memory is checked against [0, size), no workgroup waits on another, nothing is
// a float atomic, every grid is fixed by a capacity or by the store's size.  Compiled with -ffp-contract=off.
#include "kfstore.h"

#include <algorithm>

namespace {

using namespace vo;

struct DlArgs {
  KfStoreView S;
  KfConnView C;
  KfCullView X;
  KfDetectView V;
  const int *n_ledge;  // [max_kf] the pose-graph layer's loop-edge counts
  const int *graph;    // the store's graph rows
  KfdbDevView B;
  int *status;
};

__device__ __forceinline__ bool dl_keyframe(const DlArgs &A, int k) { return k >= 0 && k < A.S.size; }

// setEraseLoopDetectingKF (keyframe.cpp:547-553) without the erase: the lock comes off unless the key-frame has a loop edge
__device__ __forceinline__ void dl_release(const DlArgs &A, int k) {
  if (A.n_ledge[k] == 0) A.X.locked[k] = 0;
}

// the exclusive position of `keep` among the 256 threads in thread order, behind `base`; base advances by their number
__device__ __forceinline__ int dl_rank(bool keep, int *s_wave /*[4]*/, int &base) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long mk = __ballot(keep);
  __syncthreads();  // (the counts of the previous round have been read)
  if (lane == 0) s_wave[w] = (int)__popcll(mk);
  __syncthreads();
  int pos = base + (int)__popcll(mk & ((1ull << lane) - 1ull));
  for (int i = 0; i < 4; i++) {
    if (i < w) pos += s_wave[i];
    base += s_wave[i];
  }
  return pos;
}

__global__ __launch_bounds__(256) void k_dl_begin(DlArgs A, int current, int last_loop) {
  __shared__ int s_wave[4];
  __shared__ int s_run;
  const KfDetectView &V = A.V;
  const int tid = threadIdx.x, size = A.S.size;
  if (tid == 0) {
    int *rec = V.rec, *head = V.head;
    for (int i = 0; i < kDlRecInts; i++) rec[i] = 0;
    rec[kDlCurrent] = current;
    rec[kDlGroupsBefore] = rec[kDlGroupsAfter] = min(max(head[kDhNGroups], 0), V.G);
    for (int i = kDhNCand; i < kDlHeadInts; i++) head[i] = 0;  // no candidates, three empty pairs, no enough list
    int run = 0;
    if (!dl_keyframe(A, current) || A.X.erased[current]) {
      atomicOr(A.status, VO_KFSTORE_CONNECTIONS_INVALID);
    } else {
      A.X.locked[current] = 1;                                // :59
      if ((long long)current < (long long)last_loop + 10) {  // :62-66
        dl_release(A, current);
        rec[kDlOutcome] = VO_KFSTORE_DETECT_GATED;
        rec[kDlLocked] = A.X.locked[current], rec[kDlPending] = A.X.pending[current];
      } else {
        run = 1;
        if (current < A.B.size) head[kDhQStart] = A.B.kf_start[current], head[kDhQStart + 1] = A.B.kf_start[current + 1];
      }
    }
    head[kDhRun] = run;
    s_run = run;
  }
  __syncthreads();
  if (!s_run) return;  // (uniform)
  // conn: orderedConnectKFs_ without the bad ones, in list order
  const int n_ord = min(max(A.C.n_ordered[current], 0), min(size, A.C.max_kf));
  const int *ordered = A.C.ordered + (size_t)current * A.C.max_kf;
  int n_conn = 0;
  for (int b = 0; b < n_ord; b += 256) {
    const int i = b + tid, k = i < n_ord ? ordered[i] : -1;
    const bool keep = dl_keyframe(A, k) && kf_head(A.S, k)[1] == 0;
    const int pos = dl_rank(keep, s_wave, n_conn);
    if (keep && pos < V.max_kf) V.conn[pos] = k;
  }
  // excl: getConnectKFs() and the key-frame itself
  const int *row = A.C.W + (size_t)current * A.C.max_kf;
  int n_excl = 0;
  for (int b = 0; b < size; b += 256) {
    const int j = b + tid;
    const bool keep = j < size && (j == current || row[j] != 0);
    const int pos = dl_rank(keep, s_wave, n_excl);
    if (keep && pos < V.max_kf) V.excl[pos] = j;
  }
  if (tid == 0) {
    n_conn = min(n_conn, V.max_kf), n_excl = min(n_excl, V.max_kf);
    V.head[kDhExclStart + 1] = n_excl, V.head[kDhConnStart + 1] = n_conn;
    V.rec[kDlNExcl] = n_excl, V.rec[kDlNConn] = n_conn;
  }
}

__global__ __launch_bounds__(256) void k_dl_neighbors(DlArgs A) {
  if (!A.V.head[kDhRun]) return;
  const int k = blockIdx.x * 256 + threadIdx.x, size = min(A.S.size, A.B.size);
  if (k >= size) return;
  const int *g = A.graph + (size_t)k * kKfGraphInts;
  const int n = min(max(g[0], 0), kKfGraphNb);
  A.B.nbr_n[k] = n;
  for (int t = 0; t < kKfGraphNb; t++) {
    const int j = t < n ? g[4 + t] : -1;
    A.B.nbr[k * kKfGraphNb + t] = j >= 0 && j < size ? j : -1;
  }
}

__global__ __launch_bounds__(64) void k_dl_groups(DlArgs A) {
  const KfDetectView &V = A.V;
  const int c = blockIdx.x, lane = threadIdx.x;
  const int n = V.head[kDhNCand];
  if (!V.head[kDhRun] || n > V.D || c >= n) return;
  const int size = A.S.size, words = V.words, kf = V.cand[c];
  const int n_prev = min(max(V.head[kDhNGroups], 0), V.G), half = V.head[kDhHalf] & 1;
  unsigned long long mine = 0;  // word `lane` of the candidate's group
  if (dl_keyframe(A, kf)) {
    const int *row = A.C.W + (size_t)kf * A.C.max_kf;
    for (int w = 0; w < words; w++) {
      const int j = w * 64 + lane;
      const unsigned long long m = __ballot(j < size && (j == kf || row[j] != 0));
      if (lane == w) mine = m;
    }
  }
  if (lane < words) V.cbits[(size_t)c * words + lane] = mine;
  const unsigned long long *prev = V.bits + (size_t)half * V.G * words;
  for (int j = 0; j < n_prev; j++) {
    const bool hit = lane < words && (mine & prev[(size_t)j * words + lane]) != 0;
    const unsigned long long any = __ballot(hit);
    if (lane == 0) V.consist[(size_t)c * V.G + j] = any ? 1 : 0;
  }
}

__global__ __launch_bounds__(64) void k_dl_resolve(DlArgs A) {
  __shared__ uint8_t s_flag[kDlMaxGroups];  // prevConsistentGroupFlags (:98)
  const KfDetectView &V = A.V;
  int *head = V.head, *rec = V.rec;
  if (!head[kDhRun]) return;
  const int lane = threadIdx.x, words = V.words, G = min(V.G, kDlMaxGroups);
  const int current = rec[kDlCurrent], n = head[kDhNCand];
  const int n_prev = min(max(head[kDhNGroups], 0), G), half = head[kDhHalf] & 1;
  int outcome, n_new = 0, n_enough = 0, new_half = half;
  if (n <= 0) {  // :87-93
    outcome = VO_KFSTORE_DETECT_NO_CANDIDATES;
  } else if (n > V.D) {
    outcome = VO_KFSTORE_DETECT_OVERFLOW;
  } else {
    for (int j = lane; j < n_prev; j += 64) s_flag[j] = 0;
    __syncthreads();
    const int *cnt_prev = V.counts + (size_t)half * V.G;
    int *cnt_new = V.counts + (size_t)(half ^ 1) * V.G;
    unsigned long long *bits_new = V.bits + (size_t)(half ^ 1) * V.G * words;
    bool overflow = false;
    // (every lane walks the same sequence; s_flag is written with the same value by all of them)
    auto push = [&](int c, int count) {
      if (n_new >= G) {
        overflow = true;
        return;
      }
      for (int w = lane; w < words; w += 64) bits_new[(size_t)n_new * words + w] = V.cbits[(size_t)c * words + w];
      if (lane == 0) cnt_new[n_new] = count;
      n_new++;
    };
    for (int c = 0; c < n; c++) {  // :108
      bool enough = false, some = false;
      for (int j = 0; j < n_prev; j++) {  // :121
        if (!V.consist[(size_t)c * V.G + j]) continue;
        some = true;
        const int curr_cnt = cnt_prev[j] + 1;  // :139-140
        if (!s_flag[j]) {                      // :142-147
          push(c, curr_cnt);
          s_flag[j] = 1;
        }
        if (curr_cnt >= 3 && !enough) {  // :149-153
          if (lane == 0) V.enough[n_enough] = V.cand[c];
          n_enough++, enough = true;
        }
      }
      if (!some) push(c, 0);  // :158-162
    }
    if (overflow) {
      outcome = VO_KFSTORE_DETECT_OVERFLOW, n_new = 0, n_enough = 0;
    } else {
      outcome = n_enough > 0 ? VO_KFSTORE_DETECT_DETECTED : VO_KFSTORE_DETECT_NOT_CONSISTENT;
      new_half = half ^ 1;  // :165
    }
  }
  if (lane != 0) return;
  if (outcome == VO_KFSTORE_DETECT_OVERFLOW) atomicOr(A.status, VO_KFSTORE_DETECT_CAPACITY);
  head[kDhHalf] = new_half, head[kDhNGroups] = n_new, head[kDhNEnough] = n_enough;
  if (outcome != VO_KFSTORE_DETECT_DETECTED && dl_keyframe(A, current)) dl_release(A, current);  // :91, :169
  rec[kDlOutcome] = outcome, rec[kDlMinScore] = head[kDhMinScore], rec[kDlNCand] = n;
  rec[kDlGroupsAfter] = n_new, rec[kDlNEnough] = n_enough;
  if (dl_keyframe(A, current)) rec[kDlLocked] = A.X.locked[current], rec[kDlPending] = A.X.pending[current];
}

// computeSim3's releases by the state it ended in: `st` is the loop layer's state, `cand` its candidates
__global__ void k_dl_release(DlArgs A, const int *st, const int *cand) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int *lrec = A.V.lrec;
  for (int i = 0; i < kDlLockInts; i++) lrec[i] = i < kDkList ? 0 : -1;
  const int state = st[kLsState], n = min(max(st[kLsNCand], 0), (int)VO_KFSTORE_LOOP_MAX_CANDIDATES);
  const int current = st[kLsCurrent], match = st[kLsMatchKf];
  lrec[kDkState] = state;
  if (state == VO_KFSTORE_LOOP_UNDECIDED) return;
  int released = 0, n_pending = 0;
  for (int c = 0; c <= n; c++) {
    const int k = c < n ? cand[c] : current;
    if (!dl_keyframe(A, k)) continue;
    if (state == VO_KFSTORE_LOOP_ACCEPTED && (c == n || k == match)) continue;  // :333-337: the match and `current` stay locked
    if (!A.X.locked[k]) continue;  // (a key-frame listed twice is released once)
    dl_release(A, k);
    if (A.X.locked[k]) continue;
    released++;
    if (A.X.pending[k]) lrec[kDkList + n_pending++] = k;
  }
  lrec[kDkReleased] = released, lrec[kDkNPending] = n_pending;
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

size_t dl_layout(uint8_t *block, int max_kf, int D, int G, KfDetectView &V) {
  Layout Y{block};
  const size_t d = (size_t)D, g = (size_t)G, k = (size_t)max_kf, w = (size_t)(max_kf + 63) / 64;
  Y.take(V.head, kDlHeadInts), Y.take(V.rec, kDlRecInts), Y.take(V.lrec, kDlLockInts);
  Y.take(V.cand, d), Y.take(V.enough, d), Y.take(V.counts, 2 * g), Y.take(V.excl, k), Y.take(V.conn, k);
  Y.take(V.bits, 2 * g * w), Y.take(V.cbits, d * w), Y.take(V.consist, d * g);
  V.D = D, V.G = G, V.max_kf = max_kf, V.words = (int)w;
  return Y.at;
}

DlArgs dl_args(vo_kfstore *s, const vo_kfdb *db) {
  const KfConnView C = connections_view(s->conn);
  return DlArgs{kfstore_view(s), C, s->X, s->Dv, s->P.n_ledge, s->graph.as<int>(), db ? kfdb_dev_view(db) : KfdbDevView{}, C.status};
}

int dl_sim3_check(vo_kfstore *s, const char *W, int n_rand, const void *rand_values, int32_t rand_max, int max_rounds) {
  VO_CHECK(need(s, W, kLayerDetectLoop));
  if (n_rand < 0 || (n_rand > 0 && !rand_values) || rand_max < 1 || max_rounds < 0) return VO_ERR_INVALID;
  if (n_rand > s->L.max_rand) {
    set_error("%s: %d rand() values, the loop layer was enabled for %d", W, n_rand, s->L.max_rand);
    return VO_ERR_CAPACITY;
  }
  if (s->dl_current < 0) {
    set_error("%s: no vo_kfstore_detect_loop has been enqueued on this store", W);
    return VO_ERR_INVALID;
  }
  return VO_OK;
}

// the enough list and its count read in place, behind the outcome word
int dl_sim3_enqueue(vo_kfstore *s, int fix_scale, int n_rand, int32_t rand_max, int max_rounds, bool quiet = false) {
  const KfDetectView &V = s->Dv;
  return loop_compute_counted(s, s->dl_current, V.rec + kDlOutcome, VO_KFSTORE_DETECT_DETECTED, V.head + kDhNEnough, V.enough, fix_scale, n_rand,
                              rand_max, max_rounds, quiet);
}

// the host form's rand() values: one copy through the loop layer's staging block, not waited for
int dl_sim3_host(vo_kfstore *s, const char *W, int fix_scale, int n_rand, const int32_t *rand_values, int32_t rand_max, int max_rounds,
                 bool quiet = false) {
  VO_CHECK(dl_sim3_check(s, W, n_rand, rand_values, rand_max, max_rounds));
  if (n_rand > 0) {
    memcpy(s->lp_stage.data(), rand_values, (size_t)n_rand * 4);
    VO_CHECK(copy_h2d(s->L.rand, s->lp_stage.data(), (size_t)n_rand * 4, s->st, W));
  }
  return dl_sim3_enqueue(s, fix_scale, n_rand, rand_max, max_rounds, quiet);
}

enum { kStOutcome = 0, kStState, kStCorrect, kStStop, kStNEnough, kStMatch, kStPasses, kStLastLoop };

}  // namespace

extern "C" {

int vo_kfstore_enable_detect_loop(vo_kfstore *s, int max_detect_candidates, int max_groups) {
  const char *W = "vo_kfstore_enable_detect_loop";
  const bool args_ok = max_detect_candidates >= 1 && max_groups >= max_detect_candidates && max_groups <= kDlMaxGroups;
  if (const int rc = enable_begin(s, W, kLayerLoop | kLayerPoseGraph, kLayerDetectLoop, args_ok)) return rc < 0 ? rc : VO_OK;
  if (s->max_kf > VO_KFSTORE_CONNECTIONS_MAX_KEYFRAMES) return VO_ERR_CAPACITY;  // (a wavefront holds a group: 64 words)
  KfDetectView V{};
  const size_t bytes = dl_layout(nullptr, s->max_kf, max_detect_candidates, max_groups, V);
  VO_CHECK(s->dl.reserve(bytes));
  dl_layout(s->dl.as<uint8_t>(), s->max_kf, max_detect_candidates, max_groups, s->Dv);
  // a result coming down: the record and the two lists, or the counters and one half of the bitsets; the composed step's read
  const size_t down = std::max((size_t)(kDlRecInts + 2 * max_detect_candidates) * 4 + 64,
                               (size_t)max_groups * 4 + (size_t)max_groups * s->Dv.words * 8 + 64);
  VO_CHECK(s->dl_stage.reserve(std::max(down, (size_t)(kDlHeadInts + kDlRecInts + kLoopStateInts + kDlLockInts) * 4)));
  VO_HIP_CHECK(hipMemsetAsync(s->dl.p, 0, bytes, s->st));
  VO_CHECK(stream_sync(s->st, W));
  s->dl_current = -1, s->last_loop_kf = 0;
  s->layers |= kLayerDetectLoop;
  return VO_OK;
}

int vo_kfstore_detect_loop(vo_kfstore *s, vo_kfdb *db, int current, int last_loop_keyframe) {
  const char *W = "vo_kfstore_detect_loop";
  VO_CHECK(need(s, W, kLayerDetectLoop));
  if (!db || last_loop_keyframe < 0) return VO_ERR_INVALID;
  VO_CHECK(need_keyframe(s, W, current));
  int db_size = 0;
  kfdb_info(db, &db_size, nullptr);
  if (db_size != s->size) {
    set_error("%s: the database holds %d key-frames, the store %d", W, db_size, s->size);
    return VO_ERR_INVALID;
  }
  const DlArgs A = dl_args(s, db);
  const KfDetectView &V = s->Dv;
  hipStream_t st = s->st;
  VO_CHECK(kfdb_order_before(db, st));  // (k_dl_begin reads the row offsets an insertion has enqueued)
  hipLaunchKernelGGL(k_dl_begin, dim3(1), dim3(256), 0, st, A, current, last_loop_keyframe);
  hipLaunchKernelGGL(k_dl_neighbors, dim3((unsigned)((s->size + 255) / 256)), dim3(256), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(kfdb_query_loop_on(db, st, V.head + kDhQStart, V.head + kDhExclStart, V.excl, V.head + kDhConnStart, V.conn,
                              reinterpret_cast<float *>(V.head + kDhMinScore), V.D, V.head + kDhNCand, V.cand));
  hipLaunchKernelGGL(k_dl_groups, dim3((unsigned)V.D), dim3(64), 0, st, A);
  hipLaunchKernelGGL(k_dl_resolve, dim3(1), dim3(64), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  s->dl_current = current;
  s->gen++;  // (the lock column)
  return VO_OK;
}

int vo_kfstore_detect_loop_result(vo_kfstore *s, int32_t *record, int32_t *candidates, int32_t *enough) {
  const char *W = "vo_kfstore_detect_loop_result";
  VO_CHECK(need(s, W, kLayerDetectLoop));
  const KfDetectView &V = s->Dv;
  int32_t *down = reinterpret_cast<int32_t *>(s->dl_stage.data());
  VO_CHECK(copy_d2h(down, V.rec, kDlRecInts * 4, s->st, W));
  VO_CHECK(copy_d2h(down + kDlRecInts, V.cand, (size_t)V.D * 4, s->st, W));
  VO_CHECK(copy_d2h(down + kDlRecInts + V.D, V.enough, (size_t)V.D * 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  if (record) memcpy(record, down, kDlRecInts * 4);
  const int n = std::min(std::max(down[kDlNCand], 0), V.D), ne = std::min(std::max(down[kDlNEnough], 0), V.D);
  if (candidates && n > 0) memcpy(candidates, down + kDlRecInts, (size_t)n * 4);
  if (enough && ne > 0) memcpy(enough, down + kDlRecInts + V.D, (size_t)ne * 4);
  return VO_OK;
}

int vo_kfstore_detect_loop_groups(vo_kfstore *s, int32_t *n, int32_t *counts, uint8_t *members) {
  const char *W = "vo_kfstore_detect_loop_groups";
  VO_CHECK(need(s, W, kLayerDetectLoop));
  if (!n) return VO_ERR_INVALID;
  const KfDetectView &V = s->Dv;
  int32_t head[kDlHeadInts];
  VO_CHECK(copy_d2h(head, V.head, sizeof(head), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int ng = std::min(std::max(head[kDhNGroups], 0), V.G), half = head[kDhHalf] & 1;
  *n = ng;
  if (ng == 0) return VO_OK;
  int32_t *down = reinterpret_cast<int32_t *>(s->dl_stage.data());
  const unsigned long long *bits = reinterpret_cast<const unsigned long long *>(down + (((size_t)V.G + 3) & ~(size_t)3));  // (8-byte aligned)
  VO_CHECK(copy_d2h(down, V.counts + (size_t)half * V.G, (size_t)ng * 4, s->st, W));
  VO_CHECK(copy_d2h(const_cast<unsigned long long *>(bits), V.bits + (size_t)half * V.G * V.words, (size_t)ng * V.words * 8, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  if (counts) memcpy(counts, down, (size_t)ng * 4);
  if (members)
    for (int g = 0; g < ng; g++)
      for (int j = 0; j < s->size; j++) members[(size_t)g * s->size + j] = (uint8_t)((bits[(size_t)g * V.words + (j >> 6)] >> (j & 63)) & 1);
  return VO_OK;
}

int vo_kfstore_compute_sim3_detected_dev(vo_kfstore *s, int fix_scale, int n_rand, const int32_t *dev_rand_values, int32_t rand_max,
                                         int max_rounds) {
  const char *W = "vo_kfstore_compute_sim3_detected_dev";
  VO_CHECK(dl_sim3_check(s, W, n_rand, dev_rand_values, rand_max, max_rounds));
  if (n_rand > 0) VO_HIP_CHECK(hipMemcpyAsync(s->L.rand, dev_rand_values, (size_t)n_rand * 4, hipMemcpyDeviceToDevice, s->st));
  return dl_sim3_enqueue(s, fix_scale, n_rand, rand_max, max_rounds);
}

int vo_kfstore_compute_sim3_detected(vo_kfstore *s, int fix_scale, int n_rand, const int32_t *rand_values, int32_t rand_max, int max_rounds) {
  const char *W = "vo_kfstore_compute_sim3_detected";
  VO_CHECK(dl_sim3_host(s, W, fix_scale, n_rand, rand_values, rand_max, max_rounds));
  return stream_sync(s->st, W);
}

int vo_kfstore_release_loop_locks(vo_kfstore *s) {
  const char *W = "vo_kfstore_release_loop_locks";
  VO_CHECK(need(s, W, kLayerDetectLoop));
  hipLaunchKernelGGL(k_dl_release, dim3(1), dim3(64), 0, s->st, dl_args(s, nullptr), (const int *)s->L.st, (const int *)s->L.cand);
  VO_HIP_CHECK(hipGetLastError());
  s->gen++;
  return VO_OK;
}

int vo_kfstore_loop_locks_result(vo_kfstore *s, int32_t *n_released, int32_t *n_pending, int32_t *pending) {
  const char *W = "vo_kfstore_loop_locks_result";
  VO_CHECK(need(s, W, kLayerDetectLoop));
  int32_t lrec[kDlLockInts];
  VO_CHECK(copy_d2h(lrec, s->Dv.lrec, sizeof(lrec), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int np = std::min(std::max(lrec[kDkNPending], 0), VO_KFSTORE_LOOP_MAX_CANDIDATES + 1);
  if (n_released) *n_released = lrec[kDkReleased];
  if (n_pending) *n_pending = np;
  if (pending) memcpy(pending, lrec + kDkList, (size_t)np * 4);
  return VO_OK;
}

int vo_kfstore_set_last_loop_keyframe(vo_kfstore *s, int keyframe) {
  VO_CHECK(need(s, "vo_kfstore_set_last_loop_keyframe", kLayerDetectLoop));
  if (keyframe < 0) return VO_ERR_INVALID;
  s->last_loop_kf = keyframe;
  return VO_OK;
}

int vo_kfstore_get_last_loop_keyframe(vo_kfstore *s, int32_t *keyframe) {
  VO_CHECK(need(s, "vo_kfstore_get_last_loop_keyframe", kLayerDetectLoop));
  if (!keyframe) return VO_ERR_INVALID;
  *keyframe = s->last_loop_kf;
  return VO_OK;
}

// One iteration of LoopClosing::run (:17-37): a fixed sequence of the store's entry points, one read behind the first two
int vo_kfstore_loop_closing_step(vo_kfstore *s, vo_kfdb *db, int current, int fix_scale, int n_rand, const int32_t *rand_values,
                                 int32_t rand_max, int max_rounds, float threshold, int max_iterations, vo_lm_summary *summary,
                                 int32_t *record) {
  const char *W = "vo_kfstore_loop_closing_step";
  VO_CHECK(need(s, W, kLayerDetectLoop | kLayerLoopMerge | kLayerLoopCorrect));
  if (!(threshold > 0.f) || n_rand < 0 || (n_rand > 0 && !rand_values) || rand_max < 1 || max_rounds < 0) return VO_ERR_INVALID;
  if (n_rand > s->L.max_rand) {
    set_error("%s: %d rand() values, the loop layer was enabled for %d", W, n_rand, s->L.max_rand);
    return VO_ERR_CAPACITY;
  }
  int32_t out[16] = {0};
  out[kStState] = -1, out[kStCorrect] = 1, out[kStMatch] = -1, out[kStLastLoop] = s->last_loop_kf;
  auto stop = [&](int step, int rc) {
    out[kStStop] = step, out[kStLastLoop] = s->last_loop_kf;
    if (record) memcpy(record, out, sizeof(out));
    return rc;
  };
  int rc;
  if ((rc = vo_kfstore_detect_loop(s, db, current, s->last_loop_kf)) != VO_OK) return stop(1, rc);                        // 1. detectLoop
  if ((rc = dl_sim3_host(s, W, fix_scale, n_rand, rand_values, rand_max, max_rounds, true)) != VO_OK) return stop(2, rc);  // 2. computeSim3
  // 3. the one read: the detect record and compute_sim3's state
  int32_t *down = reinterpret_cast<int32_t *>(s->dl_stage.data());
  const int32_t *rec = down, *ls = down + kDlRecInts;
  VO_CHECK(copy_d2h(down, s->Dv.rec, kDlRecInts * 4, s->st, W));
  VO_CHECK(copy_d2h(down + kDlRecInts, s->L.st, kLoopStateInts * 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  out[kStOutcome] = rec[kDlOutcome], out[kStNEnough] = rec[kDlNEnough];
  if (rec[kDlOutcome] != VO_KFSTORE_DETECT_DETECTED) {
    // (step 2 has walked nothing and raised nothing: a key-frame without a loop is how almost every call ends)
    if (rec[kDlOutcome] == VO_KFSTORE_DETECT_OVERFLOW) {
      set_error("%s: more candidates or groups than the layer was enabled for", W);
      return stop(3, VO_ERR_CAPACITY);
    }
    return stop(rec[kDlOutcome] == VO_KFSTORE_DETECT_NONE ? 3 : 0, rec[kDlOutcome] == VO_KFSTORE_DETECT_NONE ? VO_ERR_INVALID : VO_OK);
  }
  out[kStState] = ls[kLsState];
  // 4. more rounds while the walk is undecided and moves
  while (ls[kLsState] == VO_KFSTORE_LOOP_UNDECIDED && ls[kLsPhase] != kLoopHalt && max_rounds > 0) {
    const int rounds = ls[kLsRounds];
    if ((rc = vo_kfstore_compute_sim3_continue(s, max_rounds)) != VO_OK) return stop(4, rc);
    VO_CHECK(copy_d2h(down + kDlRecInts, s->L.st, kLoopStateInts * 4, s->st, W));
    VO_CHECK(stream_sync(s->st, W));
    out[kStPasses]++, out[kStState] = ls[kLsState];
    if (ls[kLsRounds] == rounds) break;
  }
  if (ls[kLsState] == VO_KFSTORE_LOOP_UNDECIDED) return stop(4, VO_OK);
  if ((rc = vo_kfstore_release_loop_locks(s)) != VO_OK) return stop(5, rc);  // 5. (:290-296, :331-346)
  if (ls[kLsState] != VO_KFSTORE_LOOP_ACCEPTED) return stop(0, VO_OK);
  out[kStMatch] = ls[kLsMatchKf];
  out[kStCorrect] = rc = vo_kfstore_correct_loop(s, threshold, max_iterations, summary, nullptr);  // 6. correctLoop
  if (rc != VO_OK) return stop(6, rc);
  s->last_loop_kf = current;  // :491
  return stop(0, VO_OK);
}

}  // extern "C"
