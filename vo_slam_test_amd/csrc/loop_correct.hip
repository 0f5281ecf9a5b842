// loop_correct.hip -- the loop correction on the device: the propagation of the loop Sim3 over the current
// key-frame's neighbours, the correction of their map points with MapPoint::updateNormalAndDepth (loopClosing.cpp:364-437), and
// the loop connections (:461-479).  It produces, as device arrays, what vo_kfstore_search_and_fuse_loop and
// vo_kfstore_pose_graph_window_dev take: corr_kf, S_corr, S_uncorr, cp_id, cp_ref and the loopConnections CSR.
//   k_lc_begin    one thread: does the call run (the _loop form reads compute_sim3's state), `current` as the one-entry list of
//                 step 1, the loop Sim3 in its 8-double form, the record
//   k_lc_setup    ONE workgroup behind update(current): currConnect = current's ordered list, then current; its checks; every
//                 entry ranked into corr_kf; S_uncorr, S_corr and S_corr^-1 per entry
//   k_lc_count    a thread per key of the observation index: is this key the entry a point is corrected at -- the first key of
//                 its id's run that lies in a corrected key-frame?  Counts per workgroup
//   k_lc_rank     the same grid: those keys ranked in index order, which is ascending id: cp_id, cp_ref, the entry; the capacity
//   k_lc_points   a lane per corrected point: p' from the row of its entry, written to every live feature that carries the id,
//                 and updateNormalAndDepth on the STORED poses: the reference sets a key-frame's pose after that key-frame's
//                 points (:435), and the key-frame a point is corrected through is its lowest corrected holder, so no
//                 holder of the point has its corrected pose yet (section 4r, the mixed-state rule and why it reduces)
//   k_lc_poses    a thread per corrected key-frame: the pose column, behind the points
//   k_lc_csr      ONE workgroup behind the connection update of loop_connections: the rows compacted in corr_kf order
// The connection updates are connections.hip's kernels.  Which key-frame corrects a point is a position in a sorted run, the
// ranks come from counts and a prefix sum, the only atomics are integer sums and the sticky word's bits: nothing depends on
// which thread runs when.  Every index read from device memory is checked against its array before it addresses anything.
// Compiled with -ffp-contract=off: sim3_compose.h and the refresh round every double operation on its own.
#include "kfstore.h"

#include "refresh_point.h"
#include "sim3_compose.h"

#include <algorithm>

namespace {

using namespace vo;

enum { kOk = VO_KFSTORE_BA_WINDOW_OK, kEmpty = VO_KFSTORE_BA_WINDOW_EMPTY, kOverflow = VO_KFSTORE_BA_WINDOW_OVERFLOW };

struct LcArgs {
  KfStoreView S;
  KfObsView O;
  KfConnView C;
  KfCullView X;
  KfMapView M;
  KfLoopCorrectView R;
  int *ref_kf;
  double *normals;
  int *status;
};

// exclusive prefix of `flag` over the workgroup in thread order; *total = the workgroup's sum (local_ba_store.hip's)
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

// ---- the head of a call.  loop_state: NULL, or compute_sim3's state words (the _loop form: `current` and the verdict are the
// device's); scw13: NULL, or compute_sim3's Scw as R, t, s
__global__ void k_lc_begin(KfLoopCorrectView R, int curr, const int *loop_state, const double *scw8, const double *scw13) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool runs = !loop_state || loop_state[kLsState] == VO_KFSTORE_LOOP_ACCEPTED;
  const int cur = loop_state ? loop_state[kLsCurrent] : curr;
  for (int r = 0; r < kLcRecInts; r++) R.rec[r] = 0;
  R.rec[kLcCurr] = cur, R.rec[kLcStatus] = kEmpty, R.rec[kLcConnStatus] = kEmpty;
  R.cur[0] = runs ? cur : -1;  // (k_conn_count skips a negative entry and raises VO_KFSTORE_CONNECTIONS_INVALID)
  if (scw13) {
    double Sn[8];
    s3_from_pose(scw13, Sn);
    Sn[7] = scw13[12];
    for (int c = 0; c < 8; c++) R.scw[c] = Sn[c];
  } else {
    for (int c = 0; c < 8; c++) R.scw[c] = scw8[c];
  }
}

// ---- 2. currConnect and corr_kf (:367-368) and 3. the Sim3s (:378-398)
__global__ __launch_bounds__(256) void k_lc_setup(LcArgs A) {
  const KfLoopCorrectView &R = A.R;
  const int tid = threadIdx.x, size = A.S.size, cur = R.cur[0];
  if (cur < 0 || cur >= size || A.X.erased[cur]) return;  // (uniform; k_conn_count has raised the sticky bit)
  const int n = min(max(A.C.n_ordered[cur], 0), size), nc = n + 1;
  const int *ordered = A.C.ordered + (size_t)cur * A.C.max_kf;
  if (tid == 0) R.rec[kLcNCorr] = nc;
  if (nc > R.C) {  // nothing is truncated: the count is true
    if (tid == 0) R.rec[kLcStatus] = kOverflow, atomicOr(A.status, (int)VO_KFSTORE_CORRECT_LOOP_CAPACITY);
    return;
  }
  auto entry = [&](int i) { return i < n ? ordered[i] : cur; };
  int bad = tid == 0 && !(R.scw[7] > 0.0);  // (step 6 divides by the scale; a NaN fails the test too)
  for (int i = tid; i < nc; i += 256) {
    const int k = entry(i);
    bad |= k < 0 || k >= size || (i < n && k == cur);
    if (!bad) bad |= A.X.erased[k] != 0 || !*np_pose_set(A.M, k);  // (isBad is not tested at :367: a bad key-frame is corrected)
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
    return;
  }
  double Scw[8], Swc[8];
  s3_load(R.scw, Scw);
  {
    double Sc[8];
    s3_from_pose(np_pose(A.M, cur), Sc);
    s3_inv(Sc, Swc);
  }
  for (int i = tid; i < nc; i += 256) {
    const int k = entry(i);
    int rank = 0;
    for (int o = 0; o < nc; o++) rank += entry(o) < k;  // (distinct numbers: a list has no repeats)
    R.list[i] = k, R.corr_kf[rank] = k, R.perm[rank] = i, R.pos_of[k] = rank + 1;
    double Su[8], Sc[8], Si[8];
    s3_from_pose(np_pose(A.M, k), Su);
    if (k == cur) {
      for (int c = 0; c < 8; c++) Sc[c] = Scw[c];
    } else {
      double Sic[8];
      s3_mul(Su, Swc, Sic);
      s3_mul(Sic, Scw, Sc);
    }
    s3_inv(Sc, Si);
    for (int c = 0; c < 8; c++) R.S_unc[8 * (size_t)rank + c] = Su[c], R.S_corr[8 * (size_t)rank + c] = Sc[c], R.S_inv[8 * (size_t)rank + c] = Si[c];
  }
  // kLcSetup is what the two index launches branch on: k_lc_rank writes kLcStatus, and no launch branches on a word it writes
  if (tid == 0) R.rec[kLcStatus] = kOk, R.rec[kLcSetup] = 1;
}

// key s of the index: is it the entry its point is corrected at -- in a corrected key-frame, and no key of the run in front of
// it is (:401-427: key-frames ascending, features ascending, a point once)?  The index is fresh: every key is a live feature.
__device__ __forceinline__ bool lc_first(const LcArgs &A, int s, int &id, unsigned &e, int &kk) {
  if (s >= A.O.n_keys) return false;
  const unsigned long long key = A.O.keys[s];
  if (key == ~0ull) return false;
  const unsigned NK = (unsigned)A.S.NK;
  e = (unsigned)(key & 0xffffffffu), id = (int)(key >> 32), kk = (int)(e / NK);
  if (kk >= A.S.size || A.R.pos_of[kk] == 0) return false;
  for (int t = min(max(A.O.run[e], 0), s); t < s; t++) {
    const int ko = (int)((unsigned)(A.O.keys[t] & 0xffffffffu) / NK);
    if (ko < A.S.size && A.R.pos_of[ko] != 0) return false;
  }
  return true;
}

__global__ __launch_bounds__(256) void k_lc_count(LcArgs A) {
  int cnt = 0;
  if (A.R.rec[kLcSetup]) {  // (uniform: written by k_lc_setup, read-only here)
    int id, kk;
    unsigned e;
    cnt = __syncthreads_count(lc_first(A, blockIdx.x * 256 + threadIdx.x, id, e, kk));
  }
  if (threadIdx.x == 0) A.R.blk[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(256) void k_lc_rank(LcArgs A) {
  __shared__ int s_w[4], s_sum[256];
  const KfLoopCorrectView &R = A.R;
  if (!R.rec[kLcSetup]) return;  // (uniform: written by k_lc_setup, read-only in this launch)
  const int tid = threadIdx.x, b = blockIdx.x;
  int part = 0;
  for (int t = tid; t < b; t += 256) part += R.blk[t];
  s_sum[tid] = part;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) s_sum[tid] += s_sum[tid + w];
    __syncthreads();
  }
  const int base = s_sum[0];
  int id = -1, kk = 0;
  unsigned e = 0;
  const bool first = R.blk[b] > 0 && lc_first(A, b * 256 + tid, id, e, kk);
  int total;
  const int q = base + block_rank(first, s_w, &total);
  if (first && q >= 0 && q < R.P) R.cp_id[q] = id, R.cp_ref[q] = kk, R.cp_ent[q] = (int)e;
  if (b == (int)gridDim.x - 1 && tid == 0) {
    const int n_cp = base + total;
    R.rec[kLcNCp] = n_cp;
    if (n_cp > R.P) R.rec[kLcStatus] = kOverflow, atomicOr(A.status, (int)VO_KFSTORE_CORRECT_LOOP_CAPACITY);
    else R.rec[kLcLive] = R.rec[kLcNCorr], R.rec[kLcValid] = 1;
  }
}

// ---- 4. the point correction (:401-425) and 5. updateNormalAndDepth (:426, mappoint.cpp:66-116): k_ba_refresh's body
// (refresh_point.h, section 4k's operation order) at the position p'.  The poses are the pose column's, which k_lc_poses has
// not touched yet: a corrected holder at a position below the point's own would have its corrected pose here, and there is none -- such a holder
// would have corrected the point itself
__global__ __launch_bounds__(256) void k_lc_points(LcArgs A) {
  const KfLoopCorrectView &R = A.R;
  if (!R.rec[kLcValid]) return;  // (k_lc_rank's verdict: the lists are whole and the points fit)
  const int q = blockIdx.x * 256 + threadIdx.x, NK = A.S.NK, size = A.S.size;
  if (q >= min(R.rec[kLcNCp], R.P)) return;
  const int id = R.cp_id[q], k = R.cp_ref[q];
  const unsigned e0 = (unsigned)R.cp_ent[q];
  if (k < 0 || k >= size || e0 / (unsigned)NK != (unsigned)k) return;  // (written by k_lc_rank: never taken)
  const int j = R.pos_of[k] - 1;
  if (j < 0 || j >= R.C) return;
  double p[3];
  {
    double a[3];
    s3_act(R.S_unc + 8 * (size_t)j, kf_sec<double>(A.S, k, A.S.o_points) + 3 * (size_t)(e0 - (unsigned)k * (unsigned)NK), a);
    s3_act(R.S_inv + 8 * (size_t)j, a, p);
  }
  const int rows = refresh_point(A.S, A.O, A.X, A.M, A.ref_kf, A.normals, A.status, id, p, true);  // (refresh_point.h)
  if (rows) atomicAdd(R.rec + kLcNRows, rows);
}

// ---- 6. the pose columns (:430-435): SE3(s3_matrix(q), t / s), q as step 3 left it
__global__ __launch_bounds__(256) void k_lc_poses(LcArgs A) {
  const KfLoopCorrectView &R = A.R;
  if (!R.rec[kLcValid]) return;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= min(R.rec[kLcNCorr], R.C)) return;
  const int k = R.corr_kf[r];
  if (k < 0 || k >= A.S.size) return;
  const double *Sc = R.S_corr + 8 * (size_t)r;
  double *T = np_pose(A.M, k);
  s3_matrix(Sc, T);
  for (int c = 0; c < 3; c++) T[9 + c] = __ddiv_rn(Sc[4 + c], Sc[7]);
}

// ---- the loop connections (:461-479) as CSR over corr_kf: the row of corr_kf[r] is the one its list position emitted
__global__ __launch_bounds__(1024) void k_lc_csr(LcArgs A) {
  __shared__ int s_w[16];
  const KfLoopCorrectView &R = A.R;
  const int tid = threadIdx.x, size = A.S.size;
  if (!R.rec[kLcValid]) {  // (uniform) no propagate has left its lists
    if (tid == 0) R.rec[kLcConnStatus] = kEmpty, R.rec[kLcNLc] = 0, atomicOr(A.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
    return;
  }
  const int nc = min(max(R.rec[kLcNCorr], 0), R.C);
  int base = 0;
  for (int r = 0; r < nc; r++) {
    const int t = min(max(R.perm[r], 0), R.C - 1);
    const uint8_t *row = R.rows + (size_t)t * R.max_kf;
    if (tid == 0) R.lc_start[r] = base;
    for (int j0 = 0; j0 < size; j0 += 1024) {
      const int j = j0 + tid;
      const bool in = j < size && row[j] != 0;
      int total;
      const int pos = base + block_rank(in, s_w, &total);
      if (in && pos < R.E) R.lc_kf[pos] = j;
      base += total;
    }
  }
  if (tid == 0) {
    R.lc_start[nc] = base, R.rec[kLcNLc] = base;
    if (base > R.E) R.rec[kLcConnStatus] = kOverflow, atomicOr(A.status, (int)VO_KFSTORE_CORRECT_LOOP_CAPACITY);
    else R.rec[kLcConnStatus] = kOk;
  }
}

// everything before the result | the result
size_t lc_layout(uint8_t *block, int max_kf, int n_blk, int C, int P, int E, KfLoopCorrectView &R) {
  size_t at = 0;
  auto take = [&](auto *&field, size_t count) {
    using T = std::remove_reference_t<decltype(*field)>;
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += up16(count * sizeof(T));
  };
  take(R.rec, kLcRecInts), take(R.cur, 4), take(R.scw, 8), take(R.pos_of, (size_t)max_kf), take(R.perm, (size_t)C);
  take(R.S_inv, (size_t)C * 8), take(R.blk, (size_t)n_blk), take(R.cp_ent, (size_t)P);
  take(R.rows, (size_t)C * max_kf);
  const size_t r0 = at;
  take(R.list, (size_t)C), take(R.corr_kf, (size_t)C), take(R.S_corr, (size_t)C * 8), take(R.S_unc, (size_t)C * 8);
  take(R.cp_id, (size_t)P), take(R.cp_ref, (size_t)P), take(R.lc_start, (size_t)C + 1), take(R.lc_kf, (size_t)E);
  R.res = block ? block + r0 : nullptr, R.res_bytes = at - r0;
  R.C = C, R.P = P, R.E = E, R.max_kf = max_kf, R.n_blk = n_blk;
  return at;
}

LcArgs lc_args(vo_kfstore *s, const KfObsView &O) {
  const KfConnView C = connections_view(s->conn);
  return LcArgs{kfstore_view(s), O, C, s->X, s->M, s->R, s->B.ref_kf, s->normals.as<double>(), C.status};
}

// the call: the index rebuilt when stale, k_lc_begin, update(current) (three launches), a memset, five launches, the pose
// columns, update(corr_kf) (three launches).  Every grid is sized by the capacities and the index, which the host knows.
int lc_propagate_enqueue(vo_kfstore *s, int curr, const int *loop_state, const double *scw8, const double *scw13) {
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  const LcArgs A = lc_args(s, O);
  const KfLoopCorrectView &R = s->R;
  hipStream_t st = s->st;
  hipLaunchKernelGGL(k_lc_begin, dim3(1), dim3(64), 0, st, R, curr, loop_state, scw8, scw13);
  VO_CHECK(connections_update_counted(s->conn, A.S, O, 1, R.cur, nullptr, st));  // 1. (:364)
  VO_HIP_CHECK(hipMemsetAsync(R.pos_of, 0, (size_t)R.max_kf * 4, st));
  hipLaunchKernelGGL(k_lc_setup, dim3(1), dim3(256), 0, st, A);
  const unsigned grid = (unsigned)std::min((O.n_keys + 255) / 256, R.n_blk);
  hipLaunchKernelGGL(k_lc_count, dim3(grid), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_lc_rank, dim3(grid), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_lc_points, dim3((unsigned)((R.P + 255) / 256)), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_lc_poses, dim3((unsigned)((R.C + 255) / 256)), dim3(256), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(connections_update_counted(s->conn, A.S, O, R.C, R.corr_kf, R.rec + kLcLive, st));  // 7. (:436)
  s->gen++;  // 8. (no id and no flag changes: the index stays)
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_loop_correct(vo_kfstore *s, int max_corrected, int max_corrected_points, int max_loop_connections) {
  const char *W = "vo_kfstore_enable_loop_correct";
  const bool args_ok = max_corrected >= 1 && max_corrected_points >= 1 && max_loop_connections >= 1;
  if (const int rc = enable_begin(s, W, kLayerPoseGraph, kLayerLoopCorrect, args_ok)) return rc < 0 ? rc : VO_OK;
  const int n_blk = (s->okeys_cap + 255) / 256;
  KfLoopCorrectView R{};
  const size_t bytes = lc_layout(nullptr, s->max_kf, n_blk, max_corrected, max_corrected_points, max_loop_connections, R);
  VO_CHECK(connections_reserve(s->conn, max_corrected, nullptr));  // (the connection scratch of a list of that length: no call grows it)
  VO_CHECK(s->lc.reserve(bytes));
  lc_layout(s->lc.as<uint8_t>(), s->max_kf, n_blk, max_corrected, max_corrected_points, max_loop_connections, s->R);
  VO_CHECK(s->lc_stage.reserve(std::max(s->R.res_bytes, (size_t)64) + kLcRecInts * 4));
  VO_HIP_CHECK(hipMemsetAsync(s->lc.p, 0, bytes, s->st));
  hipLaunchKernelGGL(k_lc_begin, dim3(1), dim3(64), 0, s->st, s->R, -1, (const int *)nullptr, (const double *)s->R.scw, (const double *)nullptr);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerLoopCorrect;
  return VO_OK;
}

int vo_kfstore_propagate_loop_dev(vo_kfstore *s, int curr, const double *dev_Scw) {
  const char *W = "vo_kfstore_propagate_loop_dev";
  VO_CHECK(need(s, W, kLayerLoopCorrect));
  VO_CHECK(need_keyframe(s, W, curr));
  if (!dev_Scw) return VO_ERR_INVALID;
  return lc_propagate_enqueue(s, curr, nullptr, dev_Scw, nullptr);
}

int vo_kfstore_propagate_loop(vo_kfstore *s, int curr, const double *Scw) {
  const char *W = "vo_kfstore_propagate_loop";
  VO_CHECK(need(s, W, kLayerLoopCorrect));
  VO_CHECK(need_keyframe(s, W, curr));
  if (!Scw) return VO_ERR_INVALID;
  memcpy(s->lc_stage.data(), Scw, 64);
  VO_CHECK(copy_h2d(s->R.scw, s->lc_stage.data(), 64, s->st, W));  // (k_lc_begin copies it onto itself)
  VO_CHECK(lc_propagate_enqueue(s, curr, nullptr, s->R.scw, nullptr));
  return stream_sync(s->st, W);
}

int vo_kfstore_propagate_loop_sim3(vo_kfstore *s) {
  const char *W = "vo_kfstore_propagate_loop_sim3";
  VO_CHECK(need(s, W, kLayerLoopCorrect | kLayerLoop));
  if (s->size == 0) return VO_ERR_INVALID;
  // `current`, the verdict and Scw where the last compute_sim3 left them, read in place
  return lc_propagate_enqueue(s, -1, s->L.st, nullptr, s->L.Scw);
}

int vo_kfstore_loop_connections(vo_kfstore *s) {
  const char *W = "vo_kfstore_loop_connections";
  VO_CHECK(need(s, W, kLayerLoopCorrect));
  if (s->size == 0) return VO_ERR_INVALID;
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // (stale behind the caller's search_and_fuse)
  const LcArgs A = lc_args(s, O);
  const KfLoopCorrectView &R = s->R;
  VO_CHECK(connections_update_rows(s->conn, A.S, O, R.C, R.list, R.rec + kLcLive, R.pos_of, R.rows, s->st));
  hipLaunchKernelGGL(k_lc_csr, dim3(1), dim3(1024), 0, s->st, A);
  VO_HIP_CHECK(hipGetLastError());
  s->gen++;
  return VO_OK;
}

int vo_kfstore_loop_correct_result(vo_kfstore *s, int32_t *record, int32_t *list, int32_t *corr_kf, double *S_corr, double *S_uncorr,
                                   int32_t *cp_id, int32_t *cp_ref, int32_t *lc_start, int32_t *lc_kf) {
  const char *W = "vo_kfstore_loop_correct_result";
  VO_CHECK(need(s, W, kLayerLoopCorrect));
  const KfLoopCorrectView &R = s->R;
  uint8_t *down = s->lc_stage.data();
  const bool arrays = list || corr_kf || S_corr || S_uncorr || cp_id || cp_ref || lc_start || lc_kf;
  VO_CHECK(copy_d2h(down, R.rec, kLcRecInts * 4, s->st, W));
  if (arrays) VO_CHECK(copy_d2h(down + kLcRecInts * 4, R.res, R.res_bytes, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int32_t *rec = reinterpret_cast<const int32_t *>(down);
  if (record) {
    memcpy(record, rec, kLcRecInts * 4);
    for (int r = kLcLive; r < kLcRecInts; r++) record[r] = 0;  // (the layer's own words)
  }
  const bool ok = rec[kLcStatus] == kOk, conn_ok = ok && rec[kLcConnStatus] == kOk;
  const size_t nc = ok ? (size_t)std::min(std::max(rec[kLcNCorr], 0), R.C) : 0, np = ok ? (size_t)std::min(std::max(rec[kLcNCp], 0), R.P) : 0;
  const size_t nl = conn_ok ? (size_t)std::min(std::max(rec[kLcNLc], 0), R.E) : 0;
  auto staged = [&](const void *dev) { return down + kLcRecInts * 4 + (reinterpret_cast<const uint8_t *>(dev) - R.res); };
  if (list) memcpy(list, staged(R.list), nc * 4);
  if (corr_kf) memcpy(corr_kf, staged(R.corr_kf), nc * 4);
  if (S_corr) memcpy(S_corr, staged(R.S_corr), nc * 64);
  if (S_uncorr) memcpy(S_uncorr, staged(R.S_unc), nc * 64);
  if (cp_id) memcpy(cp_id, staged(R.cp_id), np * 4);
  if (cp_ref) memcpy(cp_ref, staged(R.cp_ref), np * 4);
  if (lc_start && conn_ok) memcpy(lc_start, staged(R.lc_start), (nc + 1) * 4);
  if (lc_kf) memcpy(lc_kf, staged(R.lc_kf), nl * 4);
  return VO_OK;
}

int vo_kfstore_loop_correct_arrays(vo_kfstore *s, const int32_t **dev_corr_kf, const double **dev_S_corr, const double **dev_S_uncorr,
                                   const int32_t **dev_cp_id, const int32_t **dev_cp_ref, const int32_t **dev_lc_start,
                                   const int32_t **dev_lc_kf) {
  VO_CHECK(need(s, "vo_kfstore_loop_correct_arrays", kLayerLoopCorrect));
  const KfLoopCorrectView &R = s->R;
  if (dev_corr_kf) *dev_corr_kf = R.corr_kf;
  if (dev_S_corr) *dev_S_corr = R.S_corr;
  if (dev_S_uncorr) *dev_S_uncorr = R.S_unc;
  if (dev_cp_id) *dev_cp_id = R.cp_id;
  if (dev_cp_ref) *dev_cp_ref = R.cp_ref;
  if (dev_lc_start) *dev_lc_start = R.lc_start;
  if (dev_lc_kf) *dev_lc_kf = R.lc_kf;
  return VO_OK;
}

}  // extern "C"
