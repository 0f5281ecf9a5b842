// connections.hip -- the covisibility graph and the spanning tree of the key-frame store, maintained on the device (DESIGN.md
// section 4h): KeyFrame::updateConnections, addConnection and updateBestCovisibles (keyframe.cpp:69-198) for a list of
// key-frames, applied in list order.  Three launches per call:
//   k_conn_count  a workgroup per list entry: the entry's flagged features walk their ids' runs of the observation index
//                 into an LDS histogram over key-frames (:80-93); the row, its threshold count, its first strictly largest
//                 entry and the front of its sorted list go to scratch.  The rows depend on the index alone.
//   k_conn_apply  ONE workgroup walks the list in order (:105-150): the weights, the mode bit of every key-frame it touches
//                 (thresholded / whole map) and the parent on first connection.  Threads are parallel over the other
//                 key-frame inside a step, a barrier separates the steps.  Nothing is sorted here.
//   k_conn_order  a workgroup per touched key-frame: its ordered list from its weight row and mode bit (:127-134, :176-198),
//                 its children from the parent column, its graph row for k_lm_keyframes.
// k_conn_apply_rows is k_conn_apply for the loop correction: the same sequence, which also emits per step
// the row of the loop connections, from the list membership as the step finds it.
// As in local_map.hip nothing depends on which thread runs when: the counts are integer sums, a step of the sequence
// writes every word from one thread, and the order comes from a fixed sorting network over distinct keys.
#include "kfstore.h"

#include "block_sort.h"
#include "obs_walk.h"

#include <algorithm>
#include <new>

namespace vo {

struct KfConnections {
  int max_kf = 0;
  OwnedDevBuf state, scratch;
  int n_cap = 0;  // list entries the scratch holds
  // views into `state`
  int *W = nullptr, *ordered = nullptr;                                                          // [max_kf][max_kf]
  int *n_ordered = nullptr, *mode = nullptr, *first = nullptr, *parent = nullptr, *touched = nullptr;  // [max_kf]
  int *status = nullptr;                                                                         // the sticky word
  int *graph = nullptr;                                                                          // the store's graph rows
  const int *erased = nullptr;  // [max_kf] of a store with culling, else NULL: nothing is erased
  // views into `scratch`
  int *rows = nullptr, *list = nullptr;
  int4 *meta = nullptr;
};

}  // namespace vo

namespace {

using namespace vo;

constexpr int kMaxKf = VO_KFSTORE_CONNECTIONS_MAX_KEYFRAMES;
constexpr int kThreshold = 15;  // `int threshold = 15;` (keyframe.cpp:100)
enum { kConnInvalid = VO_KFSTORE_CONNECTIONS_INVALID, kConnCapacity = VO_KFSTORE_CONNECTIONS_CAPACITY };

// k_conn_apply is ONE workgroup: its hand-offs through global memory stay inside it, so the accesses and the fence are
// workgroup-scope (a device-scope fence writes the XCD's L2 back on every step of the sequence: measured, 4.2 us a step)
__device__ __forceinline__ int load_wg(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void store_wg(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// (weight, number) packed so that the larger key wins: `first strictly largest in ascending number` / `largest number`
__device__ __forceinline__ unsigned long long key_lowest(int w, int j) {
  return ((unsigned long long)(unsigned)w << 32) | (unsigned)(0x7fffffff - j);
}
__device__ __forceinline__ unsigned long long key_highest(int w, int j) { return ((unsigned long long)(unsigned)w << 32) | (unsigned)j; }

// the workgroup's (sum of n, max of a, max of b) in every thread; s_*: 256 entries each.  Two barriers.
__device__ __forceinline__ void block_reduce(int &n, unsigned long long &a, unsigned long long &b, int *s_n, unsigned long long *s_a,
                                             unsigned long long *s_b) {
  const int tid = threadIdx.x;
  __syncthreads();  // (the arrays of the previous round have been read)
  s_n[tid] = n, s_a[tid] = a, s_b[tid] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s_n[tid] += s_n[tid + w];
      s_a[tid] = s_a[tid + w] > s_a[tid] ? s_a[tid + w] : s_a[tid];
      s_b[tid] = s_b[tid + w] > s_b[tid] ? s_b[tid + w] : s_b[tid];
    }
    __syncthreads();
  }
  n = s_n[0], a = s_a[0], b = s_b[0];
}

// meta[t] = (key-frame or -1: skipped, entries >= 15, kfmax or -1: no connection, front of the sorted list)
// n_live: NULL, or the device word that says how many entries of the list count; those beyond it are skipped silently
__global__ __launch_bounds__(256) void k_conn_count(KfStoreView S, KfObsView O, const int *list, const int *erased, int *rows, int4 *meta,
                                                    int *status, const int *n_live) {
  __shared__ int hist[kMaxKf];
  __shared__ int s_n[256];
  __shared__ unsigned long long s_a[256], s_b[256];
  const int t = blockIdx.x, tid = threadIdx.x, size = S.size, NK = S.NK;
  if (n_live && t >= *n_live) {  // (uniform over the workgroup)
    if (tid == 0) meta[t] = make_int4(-1, 0, -1, -1);
    return;
  }
  const int k = list[t];
  if (k < 0 || k >= size || (erased && erased[k])) {  // (uniform over the workgroup; an erased key-frame is never updated)
    if (tid == 0) atomicOr(status, (int)kConnInvalid), meta[t] = make_int4(-1, 0, -1, -1);
    return;
  }
  for (int j = tid; j < size; j += 256) hist[j] = 0;
  __syncthreads();
  const int n = min(max(kf_head(S, k)[0], 0), NK);
  const uint8_t *flags = kf_sec<uint8_t>(S, k, S.o_flags);
  const int *ids = kf_sec<int>(S, k, S.o_ids);
  for (int i = tid; i < n; i += 256) {
    if (!(flags[i] & 1)) continue;
    const int id = ids[i];
    if (id < 0) continue;
    obs_run_holders(O, NK, size, O.run[(size_t)k * NK + i], id, [](int, unsigned) { return true; }, [&](int kk, int) {
      if (kk != k) atomicAdd(&hist[kk], 1);  // `if (itf->first->id_ == id_) continue;` (:89)
      return true;
    });
  }
  __syncthreads();
  int *row = rows + (size_t)t * S.max_kf;
  int nt = 0;
  unsigned long long best = 0, front = 0;
  for (int j = tid; j < size; j += 256) {
    const int c = hist[j];
    row[j] = c;
    if (c > 0) best = max(best, key_lowest(c, j));
    if (c >= kThreshold) nt++, front = max(front, key_highest(c, j));
  }
  block_reduce(nt, best, front, s_n, s_a, s_b);
  if (tid == 0) {
    const int kfmax = best ? 0x7fffffff - (int)(best & 0xffffffffu) : -1;
    meta[t] = make_int4(k, nt, kfmax, nt > 0 ? (int)(front & 0xffffffffu) : kfmax);
  }
}

// (a word of W, mode, touched, first or parent is written by one thread of a step and read by another thread of a later
//  step: workgroup-scope accesses, a workgroup-scope fence in front of the barrier that ends the step; the next launch
//  sees the result through the kernel boundary.  The scratch rows and meta
//  words do not depend on the sequence: those of step t + 1 (meta: t + 2) are fetched while step t waits for its weights.)
__global__ __launch_bounds__(1024) void k_conn_apply(int size, int max_kf, int n, const int *rows, const int4 *meta, int *W, int *mode,
                                                     int *first, int *parent, int *touched) {
  constexpr int kPer = kMaxKf / 1024;  // key-frames per thread
  const int tid = threadIdx.x;
  const int4 none = make_int4(-1, 0, -1, -1);
  int4 m1 = n > 0 ? meta[0] : none, m2 = n > 1 ? meta[1] : none;
  int c1[kPer];
  for (int r = 0; r < kPer; r++) {
    const int j = tid + r * 1024;
    c1[r] = n > 0 && j < size ? rows[j] : 0;
  }
  for (int t = 0; t < n; t++) {
    const int4 m = m1;
    const int k = m.x;
    const bool live = k >= 0 && m.z >= 0;  // not skipped, and not `if (connections.empty()) return;` (:95); uniform
    int c[kPer], w[kPer];
    bool in[kPer];
    for (int r = 0; r < kPer; r++) {
      const int j = tid + r * 1024;
      c[r] = c1[r];
      in[r] = live && j < size && (m.y > 0 ? c[r] >= kThreshold : j == m.z);  // addConnection(this, c) on key-frame j (:115, :123)
      w[r] = in[r] ? load_wg(W + (size_t)j * max_kf + k) : c[r];
    }
    m1 = m2, m2 = t + 2 < n ? meta[t + 2] : none;
    for (int r = 0; r < kPer; r++) {
      const int j = tid + r * 1024;
      c1[r] = t + 1 < n && j < size ? rows[(size_t)(t + 1) * max_kf + j] : 0;
    }
    if (!live) continue;
    for (int r = 0; r < kPer; r++) {
      const int j = tid + r * 1024;
      if (j >= size) continue;
      if (in[r] && w[r] != c[r])  // absent or different (:162-170): set, and j's list becomes its whole map
        store_wg(W + (size_t)j * max_kf + k, c[r]), store_wg(mode + j, 1), store_wg(touched + j, 1);
      store_wg(W + (size_t)k * max_kf + j, c[r]);  // `connectedKFWts_ = connections;` (:140)
    }
    if (tid == 0) {
      store_wg(mode + k, 0), store_wg(touched + k, 1);
      if (k != 0 && load_wg(first + k)) {  // (:145-150)
        store_wg(parent + k, m.w), store_wg(first + k, 0), store_wg(touched + m.w, 1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
  }
}

// k_conn_apply's sequence, and per step the ROW of the loop connections (loopClosing.cpp:461-479):
// out[t][j] = 1 iff key-frame j is in k's weight map as the step leaves it (`getConnectKFs`: the whole map, and the old one when
// the update finds no connection), was NOT a member of k's ordered list as the step found it, and is not listed.  The
// membership is the function of the weight row and the mode bit k_conn_order sorts by: the whole map, or the entries >= 15,
// or -- when there is none -- the first strictly largest one.  It is taken from the state of the SEQUENCE: an earlier step that
// changed a weight of k has switched k to its whole map.  No prefetch here: a step is one row, the list is short.
__global__ __launch_bounds__(1024) void k_conn_apply_rows(int size, int max_kf, int n, const int *rows, const int4 *meta, int *W, int *mode,
                                                          int *first, int *parent, int *touched, const int *listed, uint8_t *out) {
  constexpr int kPer = kMaxKf / 1024;
  __shared__ int s_n[1024];
  __shared__ unsigned long long s_a[1024];
  const int tid = threadIdx.x;
  for (int t = 0; t < n; t++) {
    const int4 m = meta[t];
    const int k = m.x;
    uint8_t *row = out + (size_t)t * max_kf;
    if (k < 0) {  // skipped, or beyond the list (uniform): an empty row
      for (int j = tid; j < size; j += 1024) row[j] = 0;
      continue;
    }
    const bool live = m.z >= 0;
    const bool whole = load_wg(mode + k) != 0;
    int w0[kPer], nt = 0;
    unsigned long long best = 0;
    for (int r = 0; r < kPer; r++) {
      const int j = tid + r * 1024;
      w0[r] = j < size ? load_wg(W + (size_t)k * max_kf + j) : 0;
      if (w0[r] > 0) best = max(best, key_lowest(w0[r], j));
      if (w0[r] >= kThreshold) nt++;
    }
    __syncthreads();  // (the arrays of the previous step have been read)
    s_n[tid] = nt, s_a[tid] = best;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
      if (tid < w) s_n[tid] += s_n[tid + w], s_a[tid] = s_a[tid + w] > s_a[tid] ? s_a[tid + w] : s_a[tid];
      __syncthreads();
    }
    nt = s_n[0], best = s_a[0];
    const int kfmax0 = best ? 0x7fffffff - (int)(best & 0xffffffffu) : -1;
    for (int r = 0; r < kPer; r++) {
      const int j = tid + r * 1024;
      if (j >= size) continue;
      const bool old = whole ? w0[r] > 0 : (nt > 0 ? w0[r] >= kThreshold : j == kfmax0);
      int c = w0[r];  // `new` without a connection: the row as it stands (:95)
      if (live) {
        c = rows[(size_t)t * max_kf + j];
        const bool in = m.y > 0 ? c >= kThreshold : j == m.z;
        if (in && load_wg(W + (size_t)j * max_kf + k) != c)
          store_wg(W + (size_t)j * max_kf + k, c), store_wg(mode + j, 1), store_wg(touched + j, 1);
        store_wg(W + (size_t)k * max_kf + j, c);
      }
      row[j] = (c != 0 && !old && !listed[j]) ? 1 : 0;
    }
    if (live && tid == 0) {
      store_wg(mode + k, 0), store_wg(touched + k, 1);
      if (k != 0 && load_wg(first + k)) {
        store_wg(parent + k, m.w), store_wg(first + k, 0), store_wg(touched + m.w, 1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_conn_order(int size, int max_kf, const int *W, const int *mode, const int *parent,
                                                    const int *erased, int *touched, int *ordered, int *n_ordered, int *graph,
                                                    int *status) {
  __shared__ unsigned long long keys[kMaxKf];
  __shared__ int s_n[256];
  __shared__ unsigned long long s_a[256], s_b[256];
  __shared__ int s_w[4];
  const int a = blockIdx.x, tid = threadIdx.x;
  if (!touched[a]) return;  // (uniform over the workgroup)
  const int *row = W + (size_t)a * max_kf;
  const bool whole = mode[a] != 0;
  int nt = 0;
  unsigned long long best = 0, unused = 0;
  for (int j = tid; j < size; j += 256) {
    const int w = row[j];
    if (w > 0) best = max(best, key_lowest(w, j));
    if (whole ? w > 0 : w >= kThreshold) nt++;
  }
  block_reduce(nt, best, unused, s_n, s_a, s_b);
  const int kfmax = best ? 0x7fffffff - (int)(best & 0xffffffffu) : -1;
  const int m = nt > 0 ? nt : (!whole && kfmax >= 0 ? 1 : 0);
  // weight descending, ties in descending number: ascending on the complement of (weight, number)
  const int np2 = pow2_ceil(max(size, 2));
  for (int j = tid; j < np2; j += 256) {
    const int w = j < size ? row[j] : 0;
    const bool in = whole ? w > 0 : (nt > 0 ? w >= kThreshold : j == kfmax);
    keys[j] = in ? ~key_highest(w, j) : ~0ull;
  }
  block_bitonic_sort(keys, np2);
  int *out = ordered + (size_t)a * max_kf;
  for (int i = tid; i < m; i += 256) out[i] = (int)(~keys[i] & 0xffffffffu);
  int *g = graph + (size_t)a * kKfGraphInts;
  for (int i = tid; i < kKfGraphNb + 2; i += 256) g[4 + i] = i < min(m, kKfGraphNb) ? (int)(~keys[i] & 0xffffffffu) : -1;
  // children: the key-frames whose parent this one is, ascending, the lowest kKfGraphCh of them; an erased key-frame keeps
  // its parent but has left the children (eraseChild, keyframe.cpp:485)
  int base = 0;
  for (int j0 = 0; j0 < size; j0 += 256) {
    const int j = j0 + tid, lane = tid & 63, wv = tid >> 6;
    const bool c = j < size && parent[j] == a && !(erased && erased[j]);
    const unsigned long long bal = __ballot(c);
    __syncthreads();
    if (lane == 0) s_w[wv] = __popcll(bal);
    __syncthreads();
    int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    for (int i = 0; i < 4; i++) {
      if (i < wv) pos += s_w[i];
      base += s_w[i];
    }
    if (c && pos < kKfGraphCh) g[16 + pos] = j;
  }
  for (int i = min(base, kKfGraphCh) + tid; i < kKfGraphCh; i += 256) g[16 + i] = -1;
  if (tid == 0) {
    n_ordered[a] = m;
    g[0] = min(m, kKfGraphNb), g[1] = min(base, kKfGraphCh), g[2] = parent[a], g[3] = 0;
    if (base > kKfGraphCh) atomicOr(status, (int)kConnCapacity);
    touched[a] = 0;
  }
}

__global__ void k_conn_init(int max_kf, int *n_ordered, int *mode, int *first, int *parent, int *touched, int *status) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) status[0] = 0;
  if (k >= max_kf) return;
  // no list, the whole (empty) map, firstConnect_ = true, no parent
  n_ordered[k] = 0, mode[k] = 1, first[k] = 1, parent[k] = -1, touched[k] = 0;
}

}  // namespace

namespace {

size_t connections_bytes(int max_kf) { return ((size_t)2 * max_kf * max_kf + (size_t)5 * max_kf + 4) * 4; }

int connections_create(KfConnections **out, int max_kf, int *graph, hipStream_t st) {
  if (max_kf > kMaxKf) {
    set_error("vo_kfstore_enable_connections: %d key-frames, the connection state holds %d (a dense weight row per key-frame)", max_kf,
              kMaxKf);
    return VO_ERR_CAPACITY;
  }
  KfConnections *c = new (std::nothrow) KfConnections();
  if (!c) return VO_ERR_HIP;
  c->max_kf = max_kf, c->graph = graph;
  const size_t sq = (size_t)max_kf * max_kf, K = (size_t)max_kf;
  int rc = c->state.reserve(connections_bytes(max_kf));
  if (rc == VO_OK) {
    int *p = c->state.as<int>();
    c->W = p, c->ordered = p + sq, p += 2 * sq;
    c->n_ordered = p, c->mode = p + K, c->first = p + 2 * K, c->parent = p + 3 * K, c->touched = p + 4 * K, c->status = p + 5 * K;
    if (hipMemsetAsync(c->W, 0, sq * 4, st) != hipSuccess || hipMemsetAsync(c->ordered, 0xff, sq * 4, st) != hipSuccess) rc = VO_ERR_HIP;
  }
  if (rc == VO_OK) {
    hipLaunchKernelGGL(k_conn_init, dim3((max_kf + 255) / 256), dim3(256), 0, st, max_kf, c->n_ordered, c->mode, c->first, c->parent,
                       c->touched, c->status);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = VO_ERR_HIP;
  }
  if (rc != VO_OK) {
    set_error("vo_kfstore_enable_connections: allocating or initialising %zu bytes failed", connections_bytes(max_kf));
    delete c;
    return rc;
  }
  *out = c;
  return VO_OK;
}

}  // namespace

namespace vo {

void connections_destroy(KfConnections *c) { delete c; }

int connections_reserve(KfConnections *c, int n, int **dev_list) {
  if (n > c->n_cap) {
    const size_t rows = (size_t)n * c->max_kf * 4, meta = (size_t)n * sizeof(int4), list = (size_t)n * 4;
    c->n_cap = 0;
    VO_CHECK(c->scratch.reserve(meta + rows + list));
    uint8_t *p = c->scratch.as<uint8_t>();
    c->meta = reinterpret_cast<int4 *>(p), c->rows = reinterpret_cast<int *>(p + meta), c->list = reinterpret_cast<int *>(p + meta + rows);
    c->n_cap = n;
  }
  if (dev_list) *dev_list = c->list;
  return VO_OK;
}

int connections_update(KfConnections *c, const KfStoreView &S, const KfObsView &O, int n, const int *dev_list, hipStream_t st) {
  if (n <= 0 || S.size <= 0) return VO_OK;
  VO_CHECK(connections_reserve(c, n, nullptr));
  hipLaunchKernelGGL(k_conn_count, dim3(n), dim3(256), 0, st, S, O, dev_list, c->erased, c->rows, c->meta, c->status, (const int *)nullptr);
  hipLaunchKernelGGL(k_conn_apply, dim3(1), dim3(1024), 0, st, S.size, c->max_kf, n, (const int *)c->rows, (const int4 *)c->meta, c->W,
                     c->mode, c->first, c->parent, c->touched);
  return connections_order(c, S.size, st);
}

// (the scratch for n_max entries was reserved when the caller's layer was enabled: nothing is allocated here)
int connections_update_counted(KfConnections *c, const KfStoreView &S, const KfObsView &O, int n_max, const int *dev_list, const int *dev_n,
                               hipStream_t st) {
  if (n_max <= 0 || S.size <= 0) return VO_OK;
  if (n_max > c->n_cap) return VO_ERR_CAPACITY;
  hipLaunchKernelGGL(k_conn_count, dim3(n_max), dim3(256), 0, st, S, O, dev_list, c->erased, c->rows, c->meta, c->status, dev_n);
  hipLaunchKernelGGL(k_conn_apply, dim3(1), dim3(1024), 0, st, S.size, c->max_kf, n_max, (const int *)c->rows, (const int4 *)c->meta, c->W,
                     c->mode, c->first, c->parent, c->touched);
  return connections_order(c, S.size, st);
}

int connections_update_rows(KfConnections *c, const KfStoreView &S, const KfObsView &O, int n_max, const int *dev_list, const int *dev_n,
                            const int *listed, uint8_t *out, hipStream_t st) {
  if (n_max <= 0 || S.size <= 0) return VO_OK;
  if (n_max > c->n_cap) return VO_ERR_CAPACITY;
  hipLaunchKernelGGL(k_conn_count, dim3(n_max), dim3(256), 0, st, S, O, dev_list, c->erased, c->rows, c->meta, c->status, dev_n);
  hipLaunchKernelGGL(k_conn_apply_rows, dim3(1), dim3(1024), 0, st, S.size, c->max_kf, n_max, (const int *)c->rows, (const int4 *)c->meta,
                     c->W, c->mode, c->first, c->parent, c->touched, listed, out);
  return connections_order(c, S.size, st);
}

int connections_order(KfConnections *c, int size, hipStream_t st) {
  hipLaunchKernelGGL(k_conn_order, dim3(size), dim3(256), 0, st, size, c->max_kf, (const int *)c->W, (const int *)c->mode,
                     (const int *)c->parent, c->erased, c->touched, c->ordered, c->n_ordered, c->graph, c->status);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

KfConnView connections_view(const KfConnections *c) {
  return KfConnView{c->max_kf, c->W, c->ordered, c->n_ordered, c->mode, c->parent, c->touched, c->status};
}

void connections_set_erased(KfConnections *c, const int *erased) { c->erased = erased; }

}  // namespace vo

namespace {

int connections_status(KfConnections *c, hipStream_t st, int *word) {
  const char *W = "vo_kfstore_connections_status";
  int w = 0;
  VO_CHECK(copy_d2h(&w, c->status, 4, st, W));
  VO_HIP_CHECK(hipMemsetAsync(c->status, 0, 4, st));
  VO_CHECK(stream_sync(st, W));
  *word = w;
  return VO_OK;
}

int connections_get(KfConnections *c, int size, int k, hipStream_t st, int32_t *n_connected, int32_t *weights, int32_t *n_ordered,
                    int32_t *ordered, int32_t *ordered_weights, int32_t *parent, int32_t *n_children, int32_t *children) {
  const char *Wh = "vo_kfstore_get_connections";
  std::vector<int32_t> w((size_t)size), o((size_t)size);
  int32_t no = 0, g[kKfGraphInts];
  VO_CHECK(copy_d2h(w.data(), c->W + (size_t)k * c->max_kf, (size_t)size * 4, st, Wh));
  VO_CHECK(copy_d2h(o.data(), c->ordered + (size_t)k * c->max_kf, (size_t)size * 4, st, Wh));
  VO_CHECK(copy_d2h(&no, c->n_ordered + k, 4, st, Wh));
  VO_CHECK(copy_d2h(g, c->graph + (size_t)k * kKfGraphInts, sizeof(g), st, Wh));
  VO_CHECK(stream_sync(st, Wh));
  no = std::min(std::max(no, 0), size);
  int nc = 0;
  for (int j = 0; j < size; j++) nc += w[(size_t)j] > 0;
  if (n_connected) *n_connected = nc;
  if (weights) memcpy(weights, w.data(), (size_t)size * 4);
  if (n_ordered) *n_ordered = no;
  for (int i = 0; i < size; i++) {
    const int j = i < no ? o[(size_t)i] : -1;
    if (ordered) ordered[i] = j;
    if (ordered_weights) ordered_weights[i] = j >= 0 && j < size ? w[(size_t)j] : 0;
  }
  if (parent) *parent = g[2];
  if (n_children) *n_children = g[1];
  if (children) memcpy(children, g + 16, kKfGraphCh * 4);
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_connections(vo_kfstore *s) {
  if (const int rc = enable_begin(s, "vo_kfstore_enable_connections", 0, kLayerConnections)) return rc < 0 ? rc : VO_OK;
  VO_CHECK(connections_create(&s->conn, s->max_kf, s->graph.as<int>(), s->st));
  s->layers |= kLayerConnections;
  return VO_OK;
}

int vo_kfstore_update_connections_dev(vo_kfstore *s, int n, const int32_t *dev_keyframes) {
  VO_CHECK(need(s, "vo_kfstore_update_connections_dev", kLayerConnections));
  if (n < 0 || (n > 0 && !dev_keyframes)) return VO_ERR_INVALID;
  if (n == 0 || s->size == 0) return VO_OK;
  VO_CHECK(connections_reserve(s->conn, n, nullptr));  // (before the index: nothing is enqueued when it fails)
  KfObsView O;
  VO_CHECK(kfstore_obs_view(s, &O));
  s->gen++;  // (the ordered lists are what a window starts from)
  return connections_update(s->conn, kfstore_view(s), O, n, dev_keyframes, s->st);
}

int vo_kfstore_update_connections(vo_kfstore *s, int n, const int32_t *keyframes) {
  const char *W = "vo_kfstore_update_connections";
  VO_CHECK(need(s, W, kLayerConnections));
  if (n < 0 || (n > 0 && !keyframes)) return VO_ERR_INVALID;
  for (int i = 0; i < n; i++)
    if (keyframes[i] < 0 || keyframes[i] >= s->size) {
      set_error("%s: entry %d: key-frame %d outside [0, %d)", W, i, keyframes[i], s->size);
      return VO_ERR_INVALID;
    }
  if (n == 0) return VO_OK;
  int *dev_list = nullptr;
  VO_CHECK(connections_reserve(s->conn, n, &dev_list));
  VO_CHECK(copy_h2d(dev_list, keyframes, (size_t)n * 4, s->st, W));
  VO_CHECK(vo_kfstore_update_connections_dev(s, n, dev_list));
  return stream_sync(s->st, W);  // (the caller's list is free on return)
}

int vo_kfstore_connections_status(vo_kfstore *s, int32_t *word) {
  VO_CHECK(need(s, "vo_kfstore_connections_status", kLayerConnections));
  if (!word) return VO_ERR_INVALID;
  int w = 0;
  VO_CHECK(connections_status(s->conn, s->st, &w));
  *word = w;
  return VO_OK;
}

int vo_kfstore_get_connections(vo_kfstore *s, int keyframe, int32_t *n_connected, int32_t *weights, int32_t *n_ordered,
                               int32_t *ordered, int32_t *ordered_weights, int32_t *parent, int32_t *n_children, int32_t *children) {
  VO_CHECK(need(s, "vo_kfstore_get_connections", kLayerConnections));
  if (keyframe < 0 || keyframe >= s->size) return VO_ERR_INVALID;
  return connections_get(s->conn, s->size, keyframe, s->st, n_connected, weights, n_ordered, ordered, ordered_weights, parent,
                         n_children, children);
}

}  // extern "C"
