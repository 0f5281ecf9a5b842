// pose_graph_store.hip -- the loop pose graph from the key-frame store: the pose collection and the
// four edge families of Optimizer::solvePoseGraphLoop (optimizer_ceres.cpp:1062-1236) gathered on the device from the
// connection state, the poses and the loop edges, and its write-back (:1264-1301).  The solve in between is
// vo_pose_graph_solve's, unchanged (kfstore.hip).
//   k_pg_nodes     ONE workgroup: the inputs' checks, the non-erased key-frames ranked into nodes, every node's Sim3
//   k_pg_count     a thread per family-A row and per key-frame: the edges it will emit, by the walk that emits them
//   k_pg_layout    ONE workgroup: the exclusive scan of the counts, the capacities
//   k_pg_emit      the same grid and the same walk: every edge written at its offset with its measurement
//   k_pg_poses     a thread per node: Tcw12 into the pose column, S_wr = Sim3(s, R, t)^-1
//   k_pg_reanchor  workgroups striding over the key-frames, a thread per feature: rows staged through LDS in whole
//                  (coalesced both ways), S_rw | S_wr of every node in LDS when they fit, the refresh list
// The order of the edges comes from counts and a scan; the only atomics are integer sums of the record.  Every index read
// from memory is checked against its array before it addresses anything.
// Compiled with -ffp-contract=off: sim3_compose.h rounds every double operation on its own.
#include "kfstore.h"

#include "sim3_compose.h"

namespace {

using namespace vo;

enum { kOk = VO_KFSTORE_BA_WINDOW_OK, kEmpty = VO_KFSTORE_BA_WINDOW_EMPTY, kOverflow = VO_KFSTORE_BA_WINDOW_OVERFLOW };

PgInputs pg_inputs(void *block, int n_corr, int n_lc, int n_cp);  // (behind the kernels)

struct PgLayout {
  uint8_t *block;
  size_t at = 0;
  template <class T>
  void take(T *&field, size_t bytes) {
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += up16(bytes);
  }
};

void pg_layout(PgLayout &L, KfPgView &P, int max_kf, int NK, int E, int MC, int MP) {
  const size_t K = (size_t)max_kf, Nn = (size_t)std::min(max_kf, (int)kPgMaxNodes);
  L.take(P.ledge, K * kPgMaxLoopEdges * 4);
  L.take(P.n_ledge, K * 4);
  L.take(P.node_of, K * 4);
  L.take(P.cnt, ((size_t)MC + K + 1) * 4);
  L.take(P.rl, K * (size_t)NK * 4);
  L.take(P.swr, Nn * 64);
  P.in_bytes = pg_inputs(nullptr, MC, E, MP).bytes;
  L.take(P.in, P.in_bytes);
  const size_t w0 = L.at;
  L.take(P.rec, (size_t)kPgRecInts * 4);
  L.take(P.node_kf, Nn * 4);
  L.take(P.quats, Nn * 32);
  L.take(P.trans, Nn * 24);
  L.take(P.scales, Nn * 8);
  L.take(P.e_i, (size_t)E * 4);
  L.take(P.e_j, (size_t)E * 4);
  L.take(P.q_meas, (size_t)E * 32);
  L.take(P.t_meas, (size_t)E * 24);
  L.take(P.s_meas, (size_t)E * 8);
  P.win = reinterpret_cast<uint8_t *>(P.rec), P.win_bytes = L.at - w0;
  P.sol_bytes = up16(Nn * 56);
  L.take(P.sol, P.sol_bytes);
  P.max_kf = max_kf, P.NK = NK, P.max_nodes = (int)Nn, P.max_edges = E, P.max_corr = MC, P.max_cp = MP;
}

__device__ __forceinline__ int n_features(const KfStoreView &S, int k) { return min(max(kf_head(S, k)[0], 0), S.NK); }
__device__ __forceinline__ bool kf_bad(const KfStoreView &S, int k) { return kf_head(S, k)[1] != 0; }

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

// position of v in the strictly ascending a[0 .. n), or -1
__device__ __forceinline__ int find_sorted(const int *a, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == v ? lo : -1;
}

struct PgArgs {
  KfStoreView S;
  KfConnView C;
  KfCullView X;
  KfMapView M;
  KfPgView P;
  PgInputs I;
  int curr, match;
};

__device__ __forceinline__ int weight(const PgArgs &A, int a, int b) { return A.C.W[(size_t)a * A.C.max_kf + b]; }
__device__ __forceinline__ bool is_node(const PgArgs &A, int k) { return k >= 0 && k < A.S.size && A.P.node_of[k] >= 0; }

// ---- 1. nodes and 2. their Sim3s (:1062-1083)
__global__ __launch_bounds__(1024) void k_pg_nodes(PgArgs A) {
  __shared__ int s_w[16];
  const int tid = threadIdx.x, size = A.S.size;
  const KfPgView &P = A.P;
  const PgInputs &I = A.I;
  if (tid < kPgRecInts) P.rec[tid] = tid == kPgCurr ? A.curr : tid == kPgMatch ? A.match : tid == kPgFixed ? -1 : 0;
  // what only the device sees of a device form's inputs: the orders and ranges the host form validates
  int bad = 0;
  for (int r = tid; r < I.n_corr; r += 1024) {
    const int k = I.corr_kf[r], a = I.lc_start[r], b = I.lc_start[r + 1];
    bad |= k < 0 || k >= size || (r > 0 && I.corr_kf[r - 1] >= k) || a < 0 || b < a || b > I.n_lc || (r == 0 && a != 0);
  }
  if (tid == 0 && I.n_corr > 0) bad |= I.lc_start[I.n_corr] != I.n_lc;
  if (tid == 0 && I.n_corr == 0) bad |= I.n_lc != 0;
  for (int e = tid; e < I.n_lc; e += 1024) bad |= I.lc_kf[e] < 0 || I.lc_kf[e] >= size;
  for (int e = tid; e < I.n_cp; e += 1024)
    bad |= I.cp_id[e] < 0 || (e > 0 && I.cp_id[e - 1] >= I.cp_id[e]) || I.cp_ref[e] < 0 || I.cp_ref[e] >= size;
  bad = __syncthreads_or(bad);
  if (!bad) {  // (the row bounds are known to be sound now) every row strictly ascending
    for (int r = tid; r < I.n_corr; r += 1024)
      for (int e = I.lc_start[r] + 1; e < I.lc_start[r + 1]; e++) bad |= I.lc_kf[e - 1] >= I.lc_kf[e];
    bad = __syncthreads_or(bad);
  }
  if (bad || A.X.erased[A.curr] || A.X.erased[A.match]) {  // (uniform)
    if (tid == 0) P.rec[kPgStatus] = kEmpty, atomicOr(A.C.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
    return;
  }
  int base = 0, no_pose = 0;
  for (int k0 = 0; k0 < size; k0 += 1024) {
    const int k = k0 + tid;
    const bool f = k < size && !A.X.erased[k];
    int total;
    const int pos = base + block_rank(f, s_w, &total);
    if (k < size) P.node_of[k] = f ? pos : -1;
    if (f) {
      if (pos < P.max_nodes) P.node_kf[pos] = k;
      if (!*np_pose_set(A.M, k)) no_pose = 1;
    }
    base += total;
  }
  if (__syncthreads_or(no_pose)) {
    if (tid == 0) P.rec[kPgStatus] = kEmpty, atomicOr(A.C.status, (int)VO_KFSTORE_CONNECTIONS_INVALID);
    return;
  }
  if (tid == 0) P.rec[kPgNNodes] = base, P.rec[kPgFixed] = P.node_of[A.match];  // (written by this workgroup above the barrier)
  for (int i = tid; i < min(base, P.max_nodes); i += 1024) {
    const int k = P.node_kf[i], r = find_sorted(I.corr_kf, I.n_corr, k);
    double Sn[8];
    if (r >= 0) s3_load(I.S_corr + 8 * (size_t)r, Sn);
    else s3_from_pose(np_pose(A.M, k), Sn);
    for (int c = 0; c < 4; c++) P.quats[4 * (size_t)i + c] = Sn[c];
    for (int c = 0; c < 3; c++) P.trans[3 * (size_t)i + c] = Sn[4 + c];
    P.scales[i] = Sn[7];
  }
}

// ---- the walk both the count and the emit make.  Family A (:1094-1125): row r of the loop connections
template <class Sink>
__device__ __forceinline__ void walk_row(const PgArgs &A, int r, Sink sink) {
  const int k = A.I.corr_kf[r];
  if (!is_node(A, k)) return;
  for (int e = A.I.lc_start[r]; e < A.I.lc_start[r + 1]; e++) {
    const int j = A.I.lc_kf[e];
    // Q-B5: the curr / match exemption never acts, only the weight gate (:1105)
    if (j != k && is_node(A, j) && weight(A, k, j) >= kPgMinWeight) sink(0, k, j);
  }
}

// does family A emit a -> b?  (the pair is then in insertedLoopEdges)
__device__ __forceinline__ bool row_emits(const PgArgs &A, int a, int b) {
  const int r = find_sorted(A.I.corr_kf, A.I.n_corr, a);
  if (r < 0) return false;
  const int s = A.I.lc_start[r];
  return find_sorted(A.I.lc_kf + s, A.I.lc_start[r + 1] - s, b) >= 0 && is_node(A, a) && is_node(A, b) && weight(A, a, b) >= kPgMinWeight;
}

// families B, C, D of node key-frame k (:1128-1236)
template <class Sink>
__device__ __forceinline__ void walk_keyframe(const PgArgs &A, int k, Sink sink) {
  const int size = A.S.size;
  const int parent = A.C.parent[k];
  if (parent != k && is_node(A, parent)) sink(1, k, parent);  // spanning tree (:1141-1166)
  const int *le = A.P.ledge + (size_t)k * kPgMaxLoopEdges;
  const int nle = min(max(A.P.n_ledge[k], 0), (int)kPgMaxLoopEdges);
  for (int t = 0; t < nle; t++)  // loop edges found before this closure (:1168-1198)
    if (le[t] < A.curr && le[t] != k && is_node(A, le[t])) sink(2, k, le[t]);
  const int *list = A.C.ordered + (size_t)k * A.C.max_kf;
  const int n = min(max(A.C.n_ordered[k], 0), size);
  for (int t = 0; t < n; t++) {  // getCovisiblesByWeight(100): the prefix of the ordered list (:1200-1236)
    const int w = list[t];
    if (w < 0 || w >= size || w == k) continue;
    if (weight(A, k, w) < kPgMinWeight) break;
    if (w == parent || (A.C.parent[w] == k && !A.X.erased[w])) continue;  // the parent, a child
    bool loop = false;
    for (int u = 0; u < nle; u++) loop |= le[u] == w;
    if (loop || kf_bad(A.S, w) || w >= k || !is_node(A, w)) continue;
    if (row_emits(A, k, w) || row_emits(A, w, k)) continue;  // insertedLoopEdges
    sink(3, k, w);
  }
}

template <class Sink>
__device__ __forceinline__ void walk(const PgArgs &A, int t, Sink sink) {
  if (t < A.I.n_corr) walk_row(A, t, sink);
  else if (t - A.I.n_corr < A.S.size && A.P.node_of[t - A.I.n_corr] >= 0) walk_keyframe(A, t - A.I.n_corr, sink);
}

__global__ __launch_bounds__(256) void k_pg_count(PgArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (A.P.rec[kPgStatus] != kOk || t >= A.I.n_corr + A.S.size) return;
  int n[4] = {0, 0, 0, 0};
  walk(A, t, [&](int family, int, int) { n[family]++; });
  A.P.cnt[t] = ((n[0] + n[1]) + n[2]) + n[3];
  for (int f = 0; f < 4; f++)
    if (n[f]) atomicAdd(A.P.rec + kPgNA + f, n[f]);
}

// counts -> exclusive offsets, the total, the capacities
__global__ __launch_bounds__(1024) void k_pg_layout(PgArgs A) {
  __shared__ int s_scan[1024];
  const KfPgView &P = A.P;
  if (P.rec[kPgStatus] != kOk) return;  // (uniform)
  const int tid = threadIdx.x, n = A.I.n_corr + A.S.size;
  int carry = 0;
  for (int p0 = 0; p0 < n; p0 += 1024) {
    const int p = p0 + tid, v = p < n ? P.cnt[p] : 0;
    s_scan[tid] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int add = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    if (p < n) P.cnt[p] = carry + s_scan[tid] - v;
    carry += s_scan[1023];
    __syncthreads();
  }
  if (tid == 0) {
    P.cnt[n] = carry, P.rec[kPgNEdges] = carry;
    if (P.rec[kPgNNodes] > P.max_nodes || carry > P.max_edges)  // nothing is truncated: the counts are true
      P.rec[kPgStatus] = kOverflow, atomicOr(A.C.status, (int)VO_KFSTORE_POSE_GRAPH_CAPACITY);
  }
}

// S_uncorr[x] where listed, else x's node Sim3 (:1130-1139)
__device__ __forceinline__ void node_sim3(const PgArgs &A, int x, double *Sn) {
  const size_t i = (size_t)A.P.node_of[x];
  for (int c = 0; c < 4; c++) Sn[c] = A.P.quats[4 * i + c];
  for (int c = 0; c < 3; c++) Sn[4 + c] = A.P.trans[3 * i + c];
  Sn[7] = A.P.scales[i];
}
__device__ __forceinline__ void uncorrected(const PgArgs &A, int x, double *Sn) {
  const int r = find_sorted(A.I.corr_kf, A.I.n_corr, x);
  if (r >= 0) s3_load(A.I.S_unc + 8 * (size_t)r, Sn);
  else node_sim3(A, x, Sn);
}

__global__ __launch_bounds__(256) void k_pg_emit(PgArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const KfPgView &P = A.P;
  if (P.rec[kPgStatus] != kOk || t >= A.I.n_corr + A.S.size) return;
  int at = P.cnt[t];
  const int end = P.cnt[t + 1];
  walk(A, t, [&](int family, int k, int j) {
    if (at >= end || at >= P.max_edges) return;  // (the counts came from this walk: never taken)
    double Sk[8], Sj[8], Swi[8], Sji[8];
    if (family == 0) node_sim3(A, k, Sk), node_sim3(A, j, Sj);  // corrected poses (:1100, :1119)
    else uncorrected(A, k, Sk), uncorrected(A, j, Sj);
    s3_inv(Sk, Swi);
    s3_mul(Sj, Swi, Sji);
    const size_t d = (size_t)at++;
    P.e_i[d] = P.node_of[k], P.e_j[d] = P.node_of[j];
    for (int c = 0; c < 4; c++) P.q_meas[4 * d + c] = Sji[c];
    for (int c = 0; c < 3; c++) P.t_meas[3 * d + c] = Sji[4 + c];
    P.s_meas[d] = Sji[7];
  });
}

struct PgApplyArgs {
  KfStoreView S;
  KfObsView O;
  KfCullView X;
  KfMapView M;
  KfPgView P;
  PgInputs I;
  const int *ref_kf;
  int n_nodes, table_in_lds;
};

// ---- a. poses (:1264-1278): Tiw = SE3(normalised uq, t / s), Swr = Sim3(s, R(Tiw), t)^-1
__global__ __launch_bounds__(256) void k_pg_poses(PgApplyArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const KfPgView &P = A.P;
  if (i == 0) P.rec[kPgNMoved] = 0, P.rec[kPgNUnanchored] = 0;
  if (i >= A.n_nodes) return;
  const double *q = reinterpret_cast<const double *>(P.sol) + 4 * (size_t)i;
  const double *t = reinterpret_cast<const double *>(P.sol) + 4 * (size_t)A.n_nodes + 3 * (size_t)i;
  double Siw[8], R[9];
  for (int c = 0; c < 4; c++) Siw[c] = q[c];
  s3_normalize(Siw);
  Siw[4] = t[0], Siw[5] = t[1], Siw[6] = t[2], Siw[7] = P.scales[i];
  s3_matrix(Siw, R);
  double *T = np_pose(A.M, P.node_kf[i]);
  for (int c = 0; c < 9; c++) T[c] = R[c];
  for (int c = 0; c < 3; c++) T[9 + c] = __ddiv_rn(Siw[4 + c], Siw[7]);
  s3_inv(Siw, P.swr + 8 * (size_t)i);
}

// ---- b. re-anchoring (:1281-1301) and the list the refresh walks
constexpr int kPgTableDoubles = 16;  // S_rw | S_wr per node
constexpr int kPgLdsNodes = 448;     // 56 KB of table beside the 6 KB stage
__global__ __launch_bounds__(256) void k_pg_reanchor(PgApplyArgs A) {
  extern __shared__ double s_table[];
  __shared__ double s_p[768];
  const KfPgView &P = A.P;
  const int tid = threadIdx.x, NK = A.S.NK, size = A.S.size, nn = A.n_nodes;
  if (A.table_in_lds) {
    for (int x = tid; x < nn * kPgTableDoubles; x += 256) {
      const int i = x >> 4, c = x & 15;
      s_table[x] = c < 4 ? P.quats[4 * (size_t)i + c] : c < 7 ? P.trans[3 * (size_t)i + c - 4] : c == 7 ? P.scales[i] : P.swr[8 * (size_t)i + c - 8];
    }
    __syncthreads();
  }
  int moved = 0, unanchored = 0;
  for (int k = blockIdx.x; k < size; k += gridDim.x) {  // (uniform per workgroup)
    const bool erased = A.X.erased[k] != 0;
    const int n = erased ? 0 : n_features(A.S, k);
    double *rows = const_cast<double *>(kf_sec<double>(A.S, k, A.S.o_points));
    const uint8_t *flags = kf_sec<uint8_t>(A.S, k, A.S.o_flags);
    const int *ids = kf_sec<int>(A.S, k, A.S.o_ids);
    for (int f0 = 0; f0 < NK; f0 += 256) {
      const int left = 3 * (min(n, f0 + 256) - f0);  // doubles of this chunk that belong to features of k
      for (int x = tid; x < left; x += 256) s_p[x] = rows[3 * (size_t)f0 + x];
      __syncthreads();
      const int f = f0 + tid;
      int listed = -1;
      if (f < n && (flags[f] & 1)) {
        const int id = ids[f];
        const unsigned e = (unsigned)k * (unsigned)NK + (unsigned)f;
        const int pos = A.O.run[e];
        if (id >= 0 && pos >= 0 && pos < A.O.n_keys && A.O.keys[pos] == (((unsigned long long)(unsigned)id << 32) | e)) listed = id;
        const int c = id >= 0 ? find_sorted(A.I.cp_id, A.I.n_cp, id) : -1;
        const int idm = c >= 0 ? A.I.cp_ref[c] : A.ref_kf[(size_t)k * NK + f];
        const int node = idm >= 0 && idm < size ? P.node_of[idm] : -1;
        if (node >= 0 && node < nn) {
          double Srw[8], Swr[8], a[3], b[3];
          if (A.table_in_lds) {
            for (int c2 = 0; c2 < 8; c2++) Srw[c2] = s_table[node * kPgTableDoubles + c2], Swr[c2] = s_table[node * kPgTableDoubles + 8 + c2];
          } else {
            for (int c2 = 0; c2 < 4; c2++) Srw[c2] = P.quats[4 * (size_t)node + c2];
            for (int c2 = 0; c2 < 3; c2++) Srw[4 + c2] = P.trans[3 * (size_t)node + c2];
            Srw[7] = P.scales[node];
            for (int c2 = 0; c2 < 8; c2++) Swr[c2] = P.swr[8 * (size_t)node + c2];
          }
          s3_act(Srw, s_p + 3 * tid, a);
          s3_act(Swr, a, b);
          s_p[3 * tid] = b[0], s_p[3 * tid + 1] = b[1], s_p[3 * tid + 2] = b[2];
          moved++;
        } else {
          unanchored++;  // the reference reads a default-constructed Sim3 here: the row keeps its bytes
        }
      }
      if (f < NK) P.rl[(size_t)k * NK + f] = listed;
      __syncthreads();
      for (int x = tid; x < left; x += 256) rows[3 * (size_t)f0 + x] = s_p[x];
      __syncthreads();
    }
  }
  __syncthreads();  // (s_p is reused for the two sums)
  int *s_sum = reinterpret_cast<int *>(s_p);
  s_sum[tid] = moved, s_sum[256 + tid] = unanchored;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) s_sum[tid] += s_sum[tid + w], s_sum[256 + tid] += s_sum[256 + tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    if (s_sum[0]) atomicAdd(P.rec + kPgNMoved, s_sum[0]);
    if (s_sum[256]) atomicAdd(P.rec + kPgNUnanchored, s_sum[256]);
  }
}

__global__ void k_pg_init(KfPgView P) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < kPgRecInts) P.rec[t] = t == kPgStatus ? (int)kEmpty : t == kPgFixed ? -1 : 0;
  if (t < P.max_kf) P.n_ledge[t] = 0, P.node_of[t] = -1;
  if (t < P.max_kf * kPgMaxLoopEdges) P.ledge[t] = -1;
}

// KeyFrame::addLoopEdge both ways (keyframe.cpp:528-533); the host has checked the capacities and that the edge is new
__global__ void k_pg_add_edge(KfPgView P, KfCullView X, int a, int b) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int side = 0; side < 2; side++) {
    const int k = side ? b : a, v = side ? a : b;
    int *row = P.ledge + (size_t)k * kPgMaxLoopEdges;
    int n = min(max(P.n_ledge[k], 0), (int)kPgMaxLoopEdges);
    bool have = false;
    for (int t = 0; t < n; t++) have |= row[t] == v;
    if (!have && n < kPgMaxLoopEdges) {
      int t = n;
      for (; t > 0 && row[t - 1] > v; t--) row[t] = row[t - 1];
      row[t] = v, P.n_ledge[k] = n + 1;
    }
    X.locked[k] = 1;  // notEraseLoopDetecting_ = true
  }
}

PgInputs pg_inputs(void *block, int n_corr, int n_lc, int n_cp) {
  PgLayout L{reinterpret_cast<uint8_t *>(block)};
  PgInputs I{};
  I.n_corr = n_corr, I.n_lc = n_lc, I.n_cp = n_cp;
  L.take(I.S_corr, (size_t)n_corr * 64);
  L.take(I.S_unc, (size_t)n_corr * 64);
  L.take(I.corr_kf, (size_t)n_corr * 4);
  L.take(I.lc_start, ((size_t)n_corr + 1) * 4);
  L.take(I.lc_kf, (size_t)n_lc * 4);
  L.take(I.cp_id, (size_t)n_cp * 4);
  L.take(I.cp_ref, (size_t)n_cp * 4);
  I.bytes = L.at;
  return I;
}

size_t pg_store_bytes(int max_kf, int NK, int max_edges, int max_corr, int max_cp) {
  PgLayout L{nullptr};
  KfPgView P{};
  pg_layout(L, P, max_kf, NK, max_edges, max_corr, max_cp);
  return L.at;
}

KfPgView pg_store_layout(void *block, int max_kf, int NK, int max_edges, int max_corr, int max_cp) {
  PgLayout L{reinterpret_cast<uint8_t *>(block)};
  KfPgView P{};
  pg_layout(L, P, max_kf, NK, max_edges, max_corr, max_cp);
  return P;
}

int pg_store_init(const KfPgView &P, hipStream_t st) {
  const int n = std::max(P.max_kf * kPgMaxLoopEdges, (int)kPgRecInts);
  hipLaunchKernelGGL(k_pg_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// addLoopEdge both ways and both erase locks; one launch
int pg_add_loop_edge(const KfPgView &P, const KfCullView &X, int a, int b, hipStream_t st) {
  hipLaunchKernelGGL(k_pg_add_edge, dim3(1), dim3(64), 0, st, P, X, a, b);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// four launches: nodes (with the inputs' checks and the node Sim3s), counts, layout, emit
int pg_window_enqueue(const KfStoreView &S, const KfConnView &C, const KfCullView &X, const KfMapView &M, const KfPgView &P,
                      const PgInputs &I, int curr, int match, hipStream_t st) {
  PgArgs A{S, C, X, M, P, I, curr, match};
  const unsigned grid = (unsigned)((I.n_corr + S.size + 255) / 256);
  hipLaunchKernelGGL(k_pg_nodes, dim3(1), dim3(1024), 0, st, A);
  hipLaunchKernelGGL(k_pg_count, dim3(grid), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_pg_layout, dim3(1), dim3(1024), 0, st, A);
  hipLaunchKernelGGL(k_pg_emit, dim3(grid), dim3(256), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// two launches on the solver's result in P.sol: poses and S_wr, then the re-anchoring with the refresh list
int pg_apply_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                     const KfPgView &P, const PgInputs &I, int n_nodes, hipStream_t st) {
  const int in_lds = n_nodes <= kPgLdsNodes ? 1 : 0;
  PgApplyArgs A{S, O, X, M, P, I, B.ref_kf, n_nodes, in_lds};
  hipLaunchKernelGGL(k_pg_poses, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, st, A);
  const size_t lds = in_lds ? (size_t)n_nodes * kPgTableDoubles * 8 : 0;
  hipLaunchKernelGGL(k_pg_reanchor, dim3((unsigned)std::min(S.size, 256)), dim3(256), lds, st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int pg_check_counts(const vo_kfstore *s, const char *W, int curr, int match, int n_corr, int n_lc, int n_cp) {
  VO_CHECK(need_keyframe(s, W, curr));
  VO_CHECK(need_keyframe(s, W, match));
  if (n_corr < 0 || n_lc < 0 || n_cp < 0) return VO_ERR_INVALID;
  if (n_corr > s->P.max_corr || n_lc > s->P.max_edges || n_cp > s->P.max_cp) {
    set_error("%s: %d corrected key-frames, %d loop connections, %d corrected points; the store was enabled for %d, %d, %d", W, n_corr,
              n_lc, n_cp, s->P.max_corr, s->P.max_edges, s->P.max_cp);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

int pg_enqueue_window(vo_kfstore *s, int curr, int match, int n_corr, int n_lc, int n_cp) {
  const PgInputs I = pg_inputs(s->P.in, n_corr, n_lc, n_cp);
  VO_CHECK(pg_window_enqueue(kfstore_view(s), connections_view(s->conn), s->X, s->M, s->P, I, curr, match, s->st));
  s->pg_counts[0] = n_corr, s->pg_counts[1] = n_lc, s->pg_counts[2] = n_cp;
  s->pg_win.begin(s->gen);
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_pose_graph(vo_kfstore *s, int max_edges, int max_corrected, int max_corrected_points) {
  const char *W = "vo_kfstore_enable_pose_graph";
  const bool args_ok = max_edges >= 1 && max_corrected >= 1 && max_corrected_points >= 1;
  if (const int rc = enable_begin(s, W, kLayerLocalBa, kLayerPoseGraph, args_ok)) return rc < 0 ? rc : VO_OK;
  VO_CHECK(s->pg.reserve(pg_store_bytes(s->max_kf, s->NK, max_edges, max_corrected, max_corrected_points)));
  s->P = pg_store_layout(s->pg.p, s->max_kf, s->NK, max_edges, max_corrected, max_corrected_points);
  VO_CHECK(s->pg_win.stage.reserve(std::max(s->P.win_bytes, std::max(s->P.in_bytes, s->P.sol_bytes))));
  s->pg_ledge.assign((size_t)s->max_kf * (1 + VO_KFSTORE_MAX_LOOP_EDGES), 0);
  s->pg_q.resize((size_t)s->P.max_nodes * 4), s->pg_t.resize((size_t)s->P.max_nodes * 3);
  VO_CHECK(pg_store_init(s->P, s->st));
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerPoseGraph;
  return VO_OK;
}

int vo_kfstore_add_loop_edge(vo_kfstore *s, int a, int b) {
  const char *W = "vo_kfstore_add_loop_edge";
  VO_CHECK(need(s, W, kLayerPoseGraph));
  VO_CHECK(need_keyframe(s, W, a));
  VO_CHECK(need_keyframe(s, W, b));
  if (a == b) {
    set_error("%s: key-frame %d cannot be its own loop edge", W, a);
    return VO_ERR_INVALID;
  }
  const int stride = 1 + VO_KFSTORE_MAX_LOOP_EDGES;
  int32_t *ra = s->pg_ledge.data() + (size_t)a * stride, *rb = s->pg_ledge.data() + (size_t)b * stride;
  const bool a_has = std::find(ra + 1, ra + 1 + ra[0], b) != ra + 1 + ra[0], b_has = std::find(rb + 1, rb + 1 + rb[0], a) != rb + 1 + rb[0];
  if ((!a_has && ra[0] >= VO_KFSTORE_MAX_LOOP_EDGES) || (!b_has && rb[0] >= VO_KFSTORE_MAX_LOOP_EDGES)) {
    set_error("%s: key-frame %d or %d holds %d loop edges already", W, a, b, VO_KFSTORE_MAX_LOOP_EDGES);
    return VO_ERR_CAPACITY;
  }
  if (!a_has) ra[1 + ra[0]++] = b;
  if (!b_has) rb[1 + rb[0]++] = a;
  s->gen++;
  return pg_add_loop_edge(s->P, s->X, a, b, s->st);  // (a repeat still sets both locks, as addLoopEdge does)
}

int vo_kfstore_get_loop_edges(vo_kfstore *s, int keyframe, int32_t *n, int32_t *edges) {
  const char *W = "vo_kfstore_get_loop_edges";
  VO_CHECK(need(s, W, kLayerPoseGraph));
  VO_CHECK(need_keyframe(s, W, keyframe));
  int32_t h[1 + VO_KFSTORE_MAX_LOOP_EDGES];
  VO_CHECK(copy_d2h(h, s->P.n_ledge + keyframe, 4, s->st, W));
  VO_CHECK(copy_d2h(h + 1, s->P.ledge + (size_t)keyframe * VO_KFSTORE_MAX_LOOP_EDGES, VO_KFSTORE_MAX_LOOP_EDGES * 4, s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int cnt = std::min(std::max(h[0], 0), VO_KFSTORE_MAX_LOOP_EDGES);
  if (n) *n = cnt;
  if (edges) memcpy(edges, h + 1, (size_t)cnt * 4);
  return VO_OK;
}

int vo_kfstore_pose_graph_window(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *corr_kf, const double *S_corr,
                                 const double *S_uncorr, const int32_t *lc_start, const int32_t *lc_kf, int n_cp, const int32_t *cp_id,
                                 const int32_t *cp_ref) {
  const char *W = "vo_kfstore_pose_graph_window";
  VO_CHECK(need(s, W, kLayerPoseGraph));
  if (n_corr < 0 || n_cp < 0 || !lc_start || (n_corr > 0 && (!corr_kf || !S_corr || !S_uncorr)) || (n_cp > 0 && (!cp_id || !cp_ref)))
    return VO_ERR_INVALID;
  if (lc_start[0] != 0 || lc_start[n_corr] < 0 || (lc_start[n_corr] > 0 && !lc_kf)) {
    set_error("%s: the loop connections do not start at 0, or end at %d without a list", W, lc_start[n_corr]);
    return VO_ERR_INVALID;
  }
  const int n_lc = lc_start[n_corr];
  VO_CHECK(pg_check_counts(s, W, curr, match, n_corr, n_lc, n_cp));
  for (int r = 0; r < n_corr; r++) {
    if (corr_kf[r] < 0 || corr_kf[r] >= s->size || (r > 0 && corr_kf[r - 1] >= corr_kf[r])) {
      set_error("%s: corrected key-frame %d (entry %d) outside [0, %d) or not in ascending order", W, corr_kf[r], r, s->size);
      return VO_ERR_INVALID;
    }
    if (lc_start[r + 1] < lc_start[r] || lc_start[r + 1] > n_lc) {
      set_error("%s: the loop connections of entry %d run from %d to %d of %d", W, r, lc_start[r], lc_start[r + 1], n_lc);
      return VO_ERR_INVALID;
    }
    for (int e = lc_start[r]; e < lc_start[r + 1]; e++)
      if (lc_kf[e] < 0 || lc_kf[e] >= s->size || (e > lc_start[r] && lc_kf[e - 1] >= lc_kf[e])) {
        set_error("%s: loop connection %d of key-frame %d outside [0, %d) or not in ascending order", W, lc_kf[e], corr_kf[r], s->size);
        return VO_ERR_INVALID;
      }
  }
  for (int e = 0; e < n_cp; e++)
    if (cp_id[e] < 0 || (e > 0 && cp_id[e - 1] >= cp_id[e]) || cp_ref[e] < 0 || cp_ref[e] >= s->size) {
      set_error("%s: corrected point %d (entry %d) negative or not in ascending order, or its reference %d outside [0, %d)", W, cp_id[e], e,
                cp_ref[e], s->size);
      return VO_ERR_INVALID;
    }
  uint8_t *h = s->pg_win.stage.data();
  const PgInputs H = pg_inputs(h, n_corr, n_lc, n_cp);
  memcpy(H.S_corr, S_corr, (size_t)n_corr * 64), memcpy(H.S_unc, S_uncorr, (size_t)n_corr * 64);
  memcpy(H.corr_kf, corr_kf, (size_t)n_corr * 4), memcpy(H.lc_start, lc_start, ((size_t)n_corr + 1) * 4);
  memcpy(H.lc_kf, lc_kf, (size_t)n_lc * 4), memcpy(H.cp_id, cp_id, (size_t)n_cp * 4), memcpy(H.cp_ref, cp_ref, (size_t)n_cp * 4);
  VO_CHECK(copy_h2d(s->P.in, h, H.bytes, s->st, W));  // the one copy
  VO_CHECK(pg_enqueue_window(s, curr, match, n_corr, n_lc, n_cp));
  return stream_sync(s->st, W);  // (the staging block is free again)
}

int vo_kfstore_pose_graph_window_dev(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *dev_corr_kf, const double *dev_S_corr,
                                     const double *dev_S_uncorr, const int32_t *dev_lc_start, int n_lc, const int32_t *dev_lc_kf, int n_cp,
                                     const int32_t *dev_cp_id, const int32_t *dev_cp_ref) {
  const char *W = "vo_kfstore_pose_graph_window_dev";
  VO_CHECK(need(s, W, kLayerPoseGraph));
  if (!dev_lc_start || (n_corr > 0 && (!dev_corr_kf || !dev_S_corr || !dev_S_uncorr)) || (n_lc > 0 && !dev_lc_kf) ||
      (n_cp > 0 && (!dev_cp_id || !dev_cp_ref)))
    return VO_ERR_INVALID;
  VO_CHECK(pg_check_counts(s, W, curr, match, n_corr, n_lc, n_cp));
  const PgInputs I = pg_inputs(s->P.in, n_corr, n_lc, n_cp);
  auto d2d = [&](void *dst, const void *src, size_t bytes) {
    return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->st) == hipSuccess;
  };
  if (!d2d(I.S_corr, dev_S_corr, (size_t)n_corr * 64) || !d2d(I.S_unc, dev_S_uncorr, (size_t)n_corr * 64) ||
      !d2d(I.corr_kf, dev_corr_kf, (size_t)n_corr * 4) || !d2d(I.lc_start, dev_lc_start, ((size_t)n_corr + 1) * 4) ||
      !d2d(I.lc_kf, dev_lc_kf, (size_t)n_lc * 4) || !d2d(I.cp_id, dev_cp_id, (size_t)n_cp * 4) || !d2d(I.cp_ref, dev_cp_ref, (size_t)n_cp * 4)) {
    set_error("%s: hipMemcpyAsync failed", W);
    return VO_ERR_HIP;
  }
  return pg_enqueue_window(s, curr, match, n_corr, n_lc, n_cp);
}

int vo_kfstore_pose_graph_window_result(vo_kfstore *s, int32_t *record, int32_t *node_kf, double *quats, double *trans, double *scales,
                                        int32_t *edge_i, int32_t *edge_j, double *q_meas, double *t_meas, double *s_meas) {
  const char *W = "vo_kfstore_pose_graph_window_result";
  VO_CHECK(need(s, W, kLayerPoseGraph));
  const KfPgView &P = s->P;
  const KfWindow &win = s->pg_win;
  VO_CHECK(s->pg_win.fetch(P.win, P.win_bytes, false, s->st, W));
  const int32_t *r = win.rec;
  if (record) memcpy(record, r, sizeof(win.rec));
  if (r[kPgStatus] != VO_KFSTORE_BA_WINDOW_OK) return VO_OK;
  const size_t nn = (size_t)r[kPgNNodes], ne = (size_t)r[kPgNEdges];
  if (node_kf) memcpy(node_kf, win.staged(P.node_kf, P.win), nn * 4);
  if (quats) memcpy(quats, win.staged(P.quats, P.win), nn * 32);
  if (trans) memcpy(trans, win.staged(P.trans, P.win), nn * 24);
  if (scales) memcpy(scales, win.staged(P.scales, P.win), nn * 8);
  if (edge_i) memcpy(edge_i, win.staged(P.e_i, P.win), ne * 4);
  if (edge_j) memcpy(edge_j, win.staged(P.e_j, P.win), ne * 4);
  if (q_meas) memcpy(q_meas, win.staged(P.q_meas, P.win), ne * 32);
  if (t_meas) memcpy(t_meas, win.staged(P.t_meas, P.win), ne * 24);
  if (s_meas) memcpy(s_meas, win.staged(P.s_meas, P.win), ne * 8);
  return VO_OK;
}

int vo_kfstore_pose_graph_apply(vo_kfstore *s, const double *quats, const double *trans) {
  const char *W = "vo_kfstore_pose_graph_apply";
  VO_CHECK(need(s, W, kLayerPoseGraph));
  VO_CHECK(s->pg_win.check_apply(W, s->gen, s->P.win, s->st));
  if (!quats || !trans) return VO_ERR_INVALID;
  const size_t nn = (size_t)s->pg_win.rec[kPgNNodes];
  uint8_t *h = s->pg_win.stage.data();
  memcpy(h, quats, nn * 32), memcpy(h + nn * 32, trans, nn * 24);  // staged as k_pg_poses reads it: quats | trans
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));  // (rebuilt when stale: the refresh list is read off it)
  VO_CHECK(copy_h2d(s->P.sol, h, nn * 56, s->st, W));
  const PgInputs I = pg_inputs(s->P.in, s->pg_counts[0], s->pg_counts[1], s->pg_counts[2]);
  const KfStoreView V = kfstore_view(s);
  VO_CHECK(pg_apply_enqueue(V, O, s->X, s->M, s->B, s->P, I, (int)nn, s->st));
  VO_CHECK(ba_refresh_list_enqueue(V, O, s->X, s->M, s->B, s->normals.as<double>(), connections_view(s->conn).status, s->size * s->NK,
                                   s->P.rl, s->st));  // updateNormalAndDepth of every live point (:1299)
  s->obs_dirty = true, s->gen++;
  return stream_sync(s->st, W);  // (the staging block is free again)
}

int vo_kfstore_pose_graph(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *corr_kf, const double *S_corr, const double *S_uncorr,
                          const int32_t *lc_start, const int32_t *lc_kf, int n_cp, const int32_t *cp_id, const int32_t *cp_ref,
                          int max_iterations, vo_lm_summary *summary) {
  const char *W = "vo_kfstore_pose_graph";
  VO_CHECK(need(s, W, kLayerPoseGraph));
  VO_CHECK(vo_kfstore_pose_graph_window(s, curr, match, n_corr, corr_kf, S_corr, S_uncorr, lc_start, lc_kf, n_cp, cp_id, cp_ref));
  const KfPgView &P = s->P;
  const KfWindow &win = s->pg_win;
  VO_CHECK(s->pg_win.fetch(P.win, P.win_bytes, false, s->st, W));  // the ONE device-to-host copy
  const int32_t *r = win.rec;
  if (r[kPgStatus] == VO_KFSTORE_BA_WINDOW_OVERFLOW) {
    set_error("%s: %d nodes, %d edges; the solver takes %d nodes and the store was enabled for %d edges", W, r[kPgNNodes], r[kPgNEdges],
              P.max_nodes, P.max_edges);
    return VO_ERR_CAPACITY;
  }
  if (r[kPgStatus] != VO_KFSTORE_BA_WINDOW_OK) {
    set_error("%s: the window is empty (curr or match erased, a key-frame without a pose, or lists only the device could refuse)", W);
    return VO_ERR_INVALID;
  }
  const size_t nn = (size_t)r[kPgNNodes];
  memcpy(s->pg_q.data(), win.staged(P.quats, P.win), nn * 32), memcpy(s->pg_t.data(), win.staged(P.trans, P.win), nn * 24);
  // whatever the solver refuses is returned and nothing is written back (the shim's rule, optimizer_hip.inl:280-287)
  VO_CHECK(vo_pose_graph_solve((int)nn, s->pg_q.data(), s->pg_t.data(), win.staged(P.scales, P.win), r[kPgFixed], r[kPgNEdges],
                               win.staged(P.e_i, P.win), win.staged(P.e_j, P.win), win.staged(P.q_meas, P.win),
                               win.staged(P.t_meas, P.win), win.staged(P.s_meas, P.win), 1, max_iterations, summary));
  return vo_kfstore_pose_graph_apply(s, s->pg_q.data(), s->pg_t.data());
}

}  // extern "C"
