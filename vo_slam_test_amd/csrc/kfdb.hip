// kfdb.hip -- the key-frame database on the device:
//   k_bow_vector      DBoW3::Vocabulary::transform's BoW vector (the (word -> summed weight) map and its L1 normalisation,
//                     frame_hip.inl's host loop) for a ragged batch of frames, one workgroup per frame
//   k_post_*          the inverted index of Map::insertKeyFrame (src/map.cpp:9-22) as a CSR over words, rebuilt from the
//                     key-frames' vectors before the first query that follows an insertion
//   k_kfdb_query      Map::detectRelocalizationCandidates (:101-208) and Map::detectLoopCandidates (:210-333, with the
//                     minScore loop of LoopClosing::detectLoop, loopClosing.cpp:71-83), one workgroup per query
// Every result is integer arithmetic or IEEE operations in a fixed order: no float atomics, and every unordered step
// (atomic compaction, posting fill) is followed by a sort on a total key.  Compiled with -ffp-contract=off.
#include "vo_common.h"

#include <climits>
#include <new>

namespace {

constexpr int kMaxNbr = 10;         // KeyFrame::getBestCovisibleKFs(10)
constexpr int kLdsKeyframes = 16384;  // count + first shared word, 8 B per key-frame: 128 KiB of the CU's 160 KiB

__global__ void k_set_int(int *p, int v) { *p = v; }

struct NbrRow {
  int n, id[kMaxNbr];
};
__global__ void k_set_nbr(int *nbr_n, int *nbr, int kf, NbrRow r) {
  if (threadIdx.x == 0) nbr_n[kf] = r.n;
  if (threadIdx.x < kMaxNbr) nbr[kf * kMaxNbr + threadIdx.x] = threadIdx.x < (unsigned)r.n ? r.id[threadIdx.x] : -1;
}

// exclusive scan of in[0..n) into out[0..n] (out[n] = total) and, when given, out2[0..n); one workgroup of 1024
__global__ __launch_bounds__(1024) void k_excl_scan(const int *in, int n, int *out, int *out2) {
  __shared__ int part[1024];
  const int t = threadIdx.x, per = (n + 1023) / 1024;
  const int b = min(t * per, n), e = min(b + per, n);
  int s = 0;
  for (int i = b; i < e; i++) s += in[i];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int i = b; i < e; i++) {
    const int v = in[i];  // (in may alias out: read before the write of the same index)
    out[i] = run;
    if (out2) out2[i] = run;
    run += v;
  }
  if (t == 1023) out[n] = part[1023];
}

// ---------------------------------------------------------------------------------------------------- BoW vector
// One workgroup per frame.  Feature i leads its word when no earlier feature with weight > 0 carries it; the leader adds the
// word's weights in feature order (FP64), its slot is the number of smaller leading words.  The L1 norm is one lane's
// sequential sum over the slots (ascending words).  Algorithmic bytes: 12 B read and at most 12 B written per feature
// (24 MB per batch of 1024 x 1000) -- nothing next to the ~ 1.5 n^2 LDS word reads per frame of the three passes.  Measured
// 1434 us per batch (profiles/kfdb_kernel_stats_summary.txt) = 1.1 x 10^12 LDS reads/s, ~ 5 % of the LDS peak: uniform-address
// reads in loops with a data-dependent exit, bound by LDS latency per iteration.  A sort-based form would be n log^2 n.
// Frames of more than kBowLds features keep the same three arrays in global scratch instead of LDS.
constexpr int kBowLds = 2048;
__global__ __launch_bounds__(256) void k_bow_vector(const int *f_start, const int *word, const double *weight, int *n_out,
                                                    int *tkey, double *tsum, int *tw, double *tv) {
  __shared__ int s_key[kBowLds];
  __shared__ double s_sum[kBowLds], s_val[kBowLds];
  __shared__ int s_n;
  __shared__ double s_norm;
  const int f = blockIdx.x, tid = threadIdx.x, b = f_start[f], n = f_start[f + 1] - b;
  if (n <= 0) {
    if (tid == 0) n_out[f] = 0;
    return;
  }
  const bool lds = n <= kBowLds;
  int *key = lds ? s_key : tkey + b;       // the feature's word, -1 when it is skipped (weight <= 0)
  double *sum = lds ? s_sum : tsum + b;    // a leader's summed weight (> 0), -1 for every other feature
  double *val = lds ? s_val : tv + b;      // the sums in ascending word order
  for (int i = tid; i < n; i += 256) key[i] = weight[b + i] > 0 ? word[b + i] : -1;
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int w = key[i];
    bool lead = w >= 0;
    for (int j = 0; lead && j < i; j++) lead = key[j] != w;
    double s = -1.0;
    if (lead) {
      s = 0;
      for (int j = i; j < n; j++)
        if (key[j] == w) s += weight[b + j];
    }
    sum[i] = s;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const double s = sum[i];
    if (!(s >= 0)) continue;
    const int w = key[i];
    int slot = 0;
    for (int j = 0; j < n; j++) slot += sum[j] >= 0 && key[j] < w;
    tw[b + slot] = w;
    val[slot] = s;
    atomicAdd(&s_n, 1);
  }
  __syncthreads();
  const int m = s_n;
  if (tid == 0) {
    double norm = 0;
    for (int i = 0; i < m; i++) norm += fabs(val[i]);
    s_norm = norm;
    n_out[f] = m;
  }
  __syncthreads();
  const double norm = s_norm;
  for (int i = tid; i < m; i += 256) {
    const double v = val[i];
    tv[b + i] = norm > 0.0 ? v / norm : v;
  }
}

__global__ __launch_bounds__(256) void k_bow_compact(const int *f_start, const int *out_start, const int *tw, const double *tv,
                                                     int *ow, double *ov) {
  const int f = blockIdx.x, b = f_start[f], o = out_start[f], m = out_start[f + 1] - o;
  for (int i = threadIdx.x; i < m; i += 256) ow[o + i] = tw[b + i], ov[o + i] = tv[b + i];
}

// ---------------------------------------------------------------------------------------------------- inverted index
__global__ __launch_bounds__(256) void k_post_hist(int total, const int *kf_words, int n_words, int *cnt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int w = kf_words[e];
  if (w >= 0 && w < n_words) atomicAdd(&cnt[w], 1);
}
__device__ __forceinline__ int kf_of_entry(const int *kf_start, int size, int e) {  // last k with kf_start[k] <= e
  int lo = 0, hi = size;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (kf_start[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_post_fill(int total, const int *kf_words, const int *kf_start, int size, int n_words,
                                                   int *cursor, int *post_tmp) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int w = kf_words[e];
  if (w < 0 || w >= n_words) return;
  const int pos = atomicAdd(&cursor[w], 1);
  if (pos < total) post_tmp[pos] = kf_of_entry(kf_start, size, e);
}
// the fill's order within a word is the atomics': put each list in insertion order (a key-frame holds a word once, so the
// rank of an entry is the number of smaller key-frame indices in its word's list)
// L reads per entry of a list of length L (L^2 per word): 402 us for 3.43 M entries at a mean L of 34, the largest of the
// rebuild's four launches (131 + 222 + 280 + 402 us = 1.04 ms per rebuild at 4096 key-frames)
__global__ __launch_bounds__(256) void k_post_order(int total, const int *kf_words, const int *kf_start, int size, int n_words,
                                                    const int *post_start, const int *post_tmp, int *post_kf) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int w = kf_words[e];
  if (w < 0 || w >= n_words) return;
  const int k = kf_of_entry(kf_start, size, e), b = post_start[w], n = post_start[w + 1] - b;
  int rank = 0;
  for (int i = 0; i < n; i++) rank += post_tmp[b + i] < k;
  post_kf[b + rank] = k;
}

// ---------------------------------------------------------------------------------------------------- queries
struct QueryArgs {
  int size, n_words, max_out, stride;  // stride: key-frames per row of the work slabs (max_keyframes)
  const int *post_start, *post_kf, *kf_start, *kf_words;
  const double *kf_vals;
  const int *nbr_n, *nbr;
  const int *q_start, *q_words;
  const double *q_values;
  const float *stale;  // reloc: [size] or NULL
  const int *excl_start, *excl, *conn_start, *conn;  // loop
  const float *min_score;                            // loop: [nq] or NULL
  int *n_cand, *cand;
  float *score;  // [nq][size]
  unsigned long long *keys;  // slabs [max_batch][stride]
  int *order, *grep, *g_cnt, *g_first;
  float *gsc;
  int *err;
};

// Map::score of the query (qw, qv, nq) against one key-frame's vector, by one whole wave: every lane looks its query word up in
// the key-frame's ascending words; the matched terms are added one by one in ascending word order (all lanes carry the
// same sum), which is the order of the reference's merge and of k_bow_score.
__device__ double wave_score(const int *qw, const double *qv, int nq, const int *cw, const double *cv, int nc) {
  const int lane = threadIdx.x & 63;
  double s = 0;
  for (int base = 0; base < nq; base += 64) {
    const int i = base + lane;
    bool m = false;
    double term = 0;
    if (i < nq && nc > 0) {
      const int a = qw[i];
      int lo = 0, hi = nc;  // first index with cw >= a
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cw[mid] < a) lo = mid + 1;
        else hi = mid;
      }
      if (lo < nc && cw[lo] == a) {
        const double vi = qv[i], wi = cv[lo];
        m = true;
        term = fabs(vi - wi) - fabs(vi) - fabs(wi);
      }
    }
    unsigned long long mask = __ballot(m);
    while (mask) {
      const int bit = __ffsll((long long)mask) - 1;
      s += __shfl(term, bit, 64);
      mask &= mask - 1;
    }
  }
  return -s / 2.0;
}

// One workgroup per query.  Algorithmic bytes per query: 4 B per posting entry of the query's words (34 entries per word x
// 840 words = 115 KB at 4096 key-frames, 10^5 vocabulary words), ~ 10 KB per scored key-frame, 8 B of LDS per key-frame for
// the counters: ~ 0.15 GB per batch of 1024.  Measured 314 us per launch (profiles/kfdb_kernel_stats_summary.txt) = 0.5 TB/s,
// 6 % of the HBM peak: not bandwidth-bound.  Four rounds of workgroups per CU at ~ 78 us each, spent in the dependent chain
// count -> sort -> ordered FP64 sums -> groups.  The rank sort is S^2 over the scored set (S ~ 1-10 behind the 0.8 gate;
// thousands only if thousands of key-frames tie on the common-word count).
template <bool LOOP, bool LDS>
__global__ __launch_bounds__(256) void k_kfdb_query(QueryArgs a) {
  extern __shared__ int dyn[];
  __shared__ int s_max, s_ns, s_run, s_wcnt[4];
  __shared__ float s_minscore, s_wmax[4], s_best;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.size;
  const long long row = (long long)q * a.stride;
  int *cnt = LDS ? dyn : a.g_cnt + row;
  int *first = LDS ? dyn + N : a.g_first + row;
  unsigned long long *keys = a.keys + row;
  int *order = a.order + row, *grep = a.grep + row;
  float *gsc = a.gsc + row, *sc = a.score + (long long)q * N;
  const int qb = a.q_start[q], nq = max(a.q_start[q + 1] - qb, 0);
  const int *qw = a.q_words + qb;
  const double *qv = a.q_values + qb;

  for (int k = tid; k < N; k += 256) {
    cnt[k] = 0, first[k] = INT_MAX;
    sc[k] = LOOP ? -1.0f : (a.stale ? a.stale[k] : 0.0f);
  }
  if (tid == 0) s_max = 0, s_ns = 0, s_run = 0;
  __syncthreads();
  // the walk over the inverted index: a wave per query word, its lanes over the posting list
  for (int i = wave; i < nq; i += 4) {
    const int w = qw[i];
    if (w < 0 || w >= a.n_words) {
      if (lane == 0) atomicOr(a.err, 1);
      continue;
    }
    const int pb = a.post_start[w], pe = a.post_start[w + 1];
    for (int p = pb + lane; p < pe; p += 64) {
      const int k = a.post_kf[p];
      if (k >= 0 && k < N) atomicAdd(&cnt[k], 1), atomicMin(&first[k], w);
    }
  }
  __syncthreads();
  if (LOOP) {  // getConnectKFs() and the key-frame itself never enter the sharing list
    const int eb = a.excl_start[q], ee = a.excl_start[q + 1];
    for (int p = eb + tid; p < ee; p += 256) {
      const int k = a.excl[p];
      if (k >= 0 && k < N) cnt[k] = 0;
      else atomicOr(a.err, 1);
    }
    __syncthreads();
  }
  int mx = 0;
  for (int k = tid; k < N; k += 256) mx = max(mx, cnt[k]);
  if (mx) atomicMax(&s_max, mx);
  __syncthreads();
  const int max_common = s_max;
  if (max_common == 0) {  // sharingWordKFs.empty()
    if (tid == 0) a.n_cand[q] = 0;
    return;
  }
  const int min_common = LOOP ? (int)(0.8f * (float)max_common) : (int)(0.8 * (double)max_common);
  // the scored set, then its place in the sharing list: ascending (smallest shared word, insertion number)
  for (int k = tid; k < N; k += 256)
    if (cnt[k] > min_common) keys[atomicAdd(&s_ns, 1)] = ((unsigned long long)(unsigned)first[k] << 32) | (unsigned)k;
  __syncthreads();
  const int S = s_ns;
  for (int i = tid; i < S; i += 256) {
    const unsigned long long key = keys[i];
    int rank = 0;
    for (int j = 0; j < S; j++) rank += keys[j] < key;
    order[rank] = (int)(key & 0xffffffffu);
  }
  if (LOOP) {  // minScore: given, or the float minimum over the connected key-frames (loopClosing.cpp:71-83)
    if (a.min_score) {
      if (tid == 0) s_minscore = a.min_score[q];
    } else {
      const int cb = a.conn_start[q], nc = min(max(a.conn_start[q + 1] - cb, 0), a.stride);
      if (a.conn_start[q + 1] - cb > a.stride && tid == 0) atomicOr(a.err, 1);
      for (int c = wave; c < nc; c += 4) {
        const int k = a.conn[cb + c];
        float v = 1.0f;  // (an id out of range is reported and leaves the minimum alone)
        if (k >= 0 && k < N) {
          const int kb = a.kf_start[k];
          v = (float)wave_score(qw, qv, nq, a.kf_words + kb, a.kf_vals + kb, a.kf_start[k + 1] - kb);
        } else if (lane == 0) {
          atomicOr(a.err, 1);
        }
        if (lane == 0) gsc[c] = v;
      }
      __syncthreads();
      if (tid == 0) {
        float m = 1.0f;
        for (int c = 0; c < nc; c++)
          if (gsc[c] < m) m = gsc[c];
        s_minscore = m;
      }
    }
  }
  __syncthreads();
  for (int i = wave; i < S; i += 4) {
    const int k = order[i], kb = a.kf_start[k];
    const float v = (float)wave_score(qw, qv, nq, a.kf_words + kb, a.kf_vals + kb, a.kf_start[k + 1] - kb);
    if (lane == 0) sc[k] = v;
  }
  __syncthreads();
  const float min_score = LOOP ? s_minscore : 0.0f;
  // covisibility groups, one lane per scored key-frame (each lane adds its neighbours in the given order)
  float lbest = min_score;
  for (int i = tid; i < S; i += 256) {
    const int k = order[i];
    const float own = sc[k];
    const bool enter = LOOP ? own >= min_score : true;
    float group = own, best = own;
    int rep = k;
    const int nn = min(a.nbr_n[k], kMaxNbr);
    for (int t = 0; t < nn; t++) {
      const int n = a.nbr[k * kMaxNbr + t];
      if (n < 0 || n >= N) continue;
      if (LOOP ? cnt[n] > min_common : cnt[n] > 0) {
        const float s = sc[n];
        group += s;
        if (s > best) best = s, rep = n;
      }
    }
    gsc[i] = group;
    grep[i] = enter ? rep : -1;
    if (enter && group > lbest) lbest = group;
  }
  for (int d = 32; d; d >>= 1) {
    const float o = __shfl_xor(lbest, d, 64);
    if (o > lbest) lbest = o;
  }
  if (lane == 0) s_wmax[wave] = lbest;
  __syncthreads();
  if (tid == 0) {
    float b = min_score;
    for (int w = 0; w < 4; w++)
      if (s_wmax[w] > b) b = s_wmax[w];
    s_best = b;
  }
  __syncthreads();
  const float keep = 0.75f * s_best;
  // representatives that pass, first occurrence only: `first` becomes the table of the earliest passing position
  for (int i = tid; i < S; i += 256)
    if (grep[i] >= 0 && gsc[i] > keep) first[grep[i]] = INT_MAX;
  __syncthreads();
  for (int i = tid; i < S; i += 256)
    if (grep[i] >= 0 && gsc[i] > keep) atomicMin(&first[grep[i]], i);
  __syncthreads();
  for (int base = 0; base < S; base += 256) {  // ordered compaction
    const int i = base + tid;
    const bool kept = i < S && grep[i] >= 0 && gsc[i] > keep && first[grep[i]] == i;
    const unsigned long long m = __ballot(kept);
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int pos = s_run + __popcll(m & ((1ull << lane) - 1));
    for (int w = 0; w < wave; w++) pos += s_wcnt[w];
    if (kept && pos < a.max_out) a.cand[(long long)q * a.max_out + pos] = grep[i];
    __syncthreads();
    if (tid == 0) s_run += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    __syncthreads();
  }
  if (tid == 0) a.n_cand[q] = s_run;  // the true count, also beyond max_out
}

// LoopClosing::detectLoop's minScore (loopClosing.cpp:71-83) for ONE query whose vector is a row of the database: the float minimum
// of wave_score over the connected key-frames, 1.0f for an empty list -- what k_kfdb_query<true> computes from `conn` when no
// min_score is given (a minimum does not depend on the order it is taken in).  One workgroup, a wave per connected key-frame.
__global__ __launch_bounds__(256) void k_kfdb_min_score(int size, int stride, const int *kf_start, const int *kf_words, const double *kf_vals,
                                                        const int *q_start, const int *conn_start, const int *conn, float *out) {
  __shared__ float s_m[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qb = q_start[0], nq = max(q_start[1] - qb, 0);
  const int cb = conn_start[0], nc = min(max(conn_start[1] - cb, 0), stride);
  float m = 1.0f;
  for (int c = wave; c < nc; c += 4) {
    const int k = conn[cb + c];
    if (k < 0 || k >= size) continue;  // (uniform in the wave)
    const int kb = kf_start[k];
    const float v = (float)wave_score(kf_words + qb, kf_vals + qb, nq, kf_words + kb, kf_vals + kb, kf_start[k + 1] - kb);
    if (v < m) m = v;
  }
  if (lane == 0) s_m[wave] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; w++)
      if (s_m[w] < m) m = s_m[w];
    out[0] = m;
  }
}

}  // namespace

struct vo_kfdb {
  int n_words = 0, max_kf = 0, max_wpk = 0, max_batch = 0;
  int size = 0;
  long long total = 0, cap_total = 0;  // entries of the key-frames' vectors
  bool dirty = false;
  int lds_kf = kLdsKeyframes;
  bool lds_attr = false;
  hipStream_t st = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;  // a query on a caller's stream (kfdb_query_reloc_on), created on first use
  // the database
  vo::OwnedDevBuf kf_start, kf_words, kf_vals, nbr_n, nbr, post_cnt, post_start, post_tmp, post_kf;
  // per-query work slabs [max_batch][max_kf]
  vo::OwnedDevBuf keys, order, grep, gsc, g_cnt, g_first, score, err;
  // staging of the host forms (grow-only)
  vo::OwnedDevBuf h_qs, h_qw, h_qv, h_stale, h_es, h_ex, h_ms, h_cs, h_cn, h_nc, h_cand;
};

namespace {

int kfdb_rebuild(vo_kfdb *db) {
  if (!db->dirty) return VO_OK;
  hipStream_t st = db->st;
  const int total = (int)db->total, nw = db->n_words;
  VO_HIP_CHECK(hipMemsetAsync(db->post_cnt.p, 0, (size_t)(nw + 1) * 4, st));
  if (total > 0) {
    hipLaunchKernelGGL(k_post_hist, dim3((total + 255) / 256), dim3(256), 0, st, total, db->kf_words.as<int>(), nw, db->post_cnt.as<int>());
  }
  hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(1024), 0, st, db->post_cnt.as<int>(), nw, db->post_start.as<int>(), db->post_cnt.as<int>());
  if (total > 0) {
    hipLaunchKernelGGL(k_post_fill, dim3((total + 255) / 256), dim3(256), 0, st, total, db->kf_words.as<int>(), db->kf_start.as<int>(),
                       db->size, nw, db->post_cnt.as<int>(), db->post_tmp.as<int>());
    hipLaunchKernelGGL(k_post_order, dim3((total + 255) / 256), dim3(256), 0, st, total, db->kf_words.as<int>(), db->kf_start.as<int>(),
                       db->size, nw, db->post_start.as<int>(), db->post_tmp.as<int>(), db->post_kf.as<int>());
  }
  VO_HIP_CHECK(hipGetLastError());
  db->dirty = false;
  return VO_OK;
}

template <bool LOOP>
int kfdb_launch(vo_kfdb *db, int nq, const QueryArgs &a) {
  const bool lds = db->size <= db->lds_kf;
  const size_t dyn = lds ? (size_t)db->size * 8 : 0;
  if (lds && dyn > 48 * 1024 && !db->lds_attr) {
    const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kfdb_query<false, true>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsKeyframes * 8);
    const hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kfdb_query<true, true>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsKeyframes * 8);
    if (e1 != hipSuccess || e2 != hipSuccess) {
      (void)hipGetLastError();
      db->lds_kf = std::min(db->lds_kf, 48 * 1024 / 8);  // what every launch may ask for; beyond it, the global slab
      return kfdb_launch<LOOP>(db, nq, a);
    }
    db->lds_attr = true;
  }
  if (lds) hipLaunchKernelGGL((k_kfdb_query<LOOP, true>), dim3(nq), dim3(256), dyn, db->st, a);
  else hipLaunchKernelGGL((k_kfdb_query<LOOP, false>), dim3(nq), dim3(256), 0, db->st, a);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// the device form of both queries: rebuild when an insertion is pending, one query launch
int kfdb_query_dev(vo_kfdb *db, bool loop, int nq, const int *q_start, const int *q_words, const double *q_values, const float *stale,
                   const int *excl_start, const int *excl, const float *min_score, const int *conn_start, const int *conn, int max_out,
                   int *n_cand, int *cand, float *score_out, const char *W) {
  if (!db || nq < 0 || max_out < 0) return VO_ERR_INVALID;
  if (nq == 0) return VO_OK;
  if (!q_start || !n_cand || (max_out > 0 && !cand)) return VO_ERR_INVALID;
  if (loop && (!excl_start || (!min_score && !conn_start))) return VO_ERR_INVALID;
  if (nq > db->max_batch) {
    vo::set_error("%s: %d queries, the database was created for batches of %d", W, nq, db->max_batch);
    return VO_ERR_CAPACITY;
  }
  VO_CHECK(kfdb_rebuild(db));
  if (db->size == 0) {  // nothing inserted: every query finds nothing (no kernel to size)
    VO_HIP_CHECK(hipMemsetAsync(n_cand, 0, (size_t)nq * 4, db->st));
    return VO_OK;
  }
  QueryArgs a{};
  a.size = db->size, a.n_words = db->n_words, a.max_out = max_out, a.stride = db->max_kf;
  a.post_start = db->post_start.as<int>(), a.post_kf = db->post_kf.as<int>();
  a.kf_start = db->kf_start.as<int>(), a.kf_words = db->kf_words.as<int>(), a.kf_vals = db->kf_vals.as<double>();
  a.nbr_n = db->nbr_n.as<int>(), a.nbr = db->nbr.as<int>();
  a.q_start = q_start, a.q_words = q_words, a.q_values = q_values;
  a.stale = stale, a.excl_start = excl_start, a.excl = excl, a.min_score = min_score, a.conn_start = conn_start, a.conn = conn;
  a.n_cand = n_cand, a.cand = cand, a.score = score_out ? score_out : db->score.as<float>();
  a.keys = db->keys.as<unsigned long long>(), a.order = db->order.as<int>(), a.grep = db->grep.as<int>(), a.gsc = db->gsc.as<float>();
  a.g_cnt = db->g_cnt.as<int>(), a.g_first = db->g_first.as<int>(), a.err = db->err.as<int>();
  return loop ? kfdb_launch<true>(db, nq, a) : kfdb_launch<false>(db, nq, a);
}

// checks of a host CSR: offsets start at 0 and ascend; returns the total or -1
long long csr_total(const int32_t *start, int n) {
  if (start[0] != 0) return -1;
  for (int i = 0; i < n; i++)
    if (start[i + 1] < start[i]) return -1;
  return start[n];
}

int kfdb_query_host(vo_kfdb *db, bool loop, int nq, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                    const float *stale, const int32_t *excl_start, const int32_t *excl, const float *min_score,
                    const int32_t *conn_start, const int32_t *conn, int max_out, int32_t *n_cand, int32_t *cand, float *score_out,
                    const char *W) {
  if (!db || nq < 0 || max_out < 0) return VO_ERR_INVALID;
  if (nq == 0) return VO_OK;
  if (!q_start || !n_cand || (max_out > 0 && !cand)) return VO_ERR_INVALID;
  if (loop && (!excl_start || (!min_score && !conn_start))) return VO_ERR_INVALID;
  if (nq > db->max_batch) {
    vo::set_error("%s: %d queries, the database was created for batches of %d", W, nq, db->max_batch);
    return VO_ERR_CAPACITY;
  }
  const long long tq = csr_total(q_start, nq);
  if (tq < 0 || (tq > 0 && (!q_words || !q_values))) return VO_ERR_INVALID;
  for (int i = 0; i < nq; i++)
    if (q_start[i + 1] - q_start[i] > db->max_wpk) {
      vo::set_error("%s: query %d has %d words, the database was created for %d", W, i, q_start[i + 1] - q_start[i], db->max_wpk);
      return VO_ERR_CAPACITY;
    }
  for (long long i = 0; i < tq; i++)
    if (q_words[i] < 0 || q_words[i] >= db->n_words) {
      vo::set_error("%s: word %d out of range", W, q_words[i]);
      return VO_ERR_INVALID;
    }
  long long te = 0, tc = 0;
  if (loop) {
    te = csr_total(excl_start, nq);
    if (te < 0 || (te > 0 && !excl)) return VO_ERR_INVALID;
    for (long long i = 0; i < te; i++)
      if (excl[i] < 0 || excl[i] >= db->size) return VO_ERR_INVALID;
    if (!min_score) {
      tc = csr_total(conn_start, nq);
      if (tc < 0 || (tc > 0 && !conn)) return VO_ERR_INVALID;
      for (long long i = 0; i < tc; i++)
        if (conn[i] < 0 || conn[i] >= db->size) return VO_ERR_INVALID;
      for (int i = 0; i < nq; i++)
        if (conn_start[i + 1] - conn_start[i] > db->max_kf) return VO_ERR_CAPACITY;
    }
  }
  hipStream_t st = db->st;
  VO_CHECK(vo::upload(db->h_qs, q_start, (size_t)(nq + 1) * 4, st, W));
  VO_CHECK(vo::upload(db->h_qw, q_words, (size_t)tq * 4, st, W));
  VO_CHECK(vo::upload(db->h_qv, q_values, (size_t)tq * 8, st, W));
  if (!loop && stale) VO_CHECK(vo::upload(db->h_stale, stale, (size_t)db->size * 4, st, W));
  if (loop) {
    VO_CHECK(vo::upload(db->h_es, excl_start, (size_t)(nq + 1) * 4, st, W));
    VO_CHECK(vo::upload(db->h_ex, excl, (size_t)te * 4, st, W));
    if (min_score) {
      VO_CHECK(vo::upload(db->h_ms, min_score, (size_t)nq * 4, st, W));
    } else {
      VO_CHECK(vo::upload(db->h_cs, conn_start, (size_t)(nq + 1) * 4, st, W));
      VO_CHECK(vo::upload(db->h_cn, conn, (size_t)tc * 4, st, W));
    }
  }
  VO_CHECK(db->h_nc.reserve((size_t)nq * 4));
  VO_CHECK(db->h_cand.reserve(std::max<size_t>((size_t)nq * max_out * 4, 64)));
  VO_HIP_CHECK(hipMemsetAsync(db->err.p, 0, 4, st));
  VO_CHECK(kfdb_query_dev(db, loop, nq, db->h_qs.as<int>(), db->h_qw.as<int>(), db->h_qv.as<double>(),
                          !loop && stale ? db->h_stale.as<float>() : nullptr, db->h_es.as<int>(), db->h_ex.as<int>(),
                          loop && min_score ? db->h_ms.as<float>() : nullptr, db->h_cs.as<int>(), db->h_cn.as<int>(), max_out,
                          db->h_nc.as<int>(), db->h_cand.as<int>(), nullptr, W));
  int err = 0;
  VO_CHECK(vo::copy_d2h(n_cand, db->h_nc.p, (size_t)nq * 4, st, W));
  VO_CHECK(vo::copy_d2h(&err, db->err.p, 4, st, W));
  VO_CHECK(vo::stream_sync(st, W));
  if (err) {
    vo::set_error("%s: an id was out of range on the device", W);
    return VO_ERR_INVALID;
  }
  // candidates of query i: the first min(n_cand, max_out) entries of its row
  for (int i = 0; i < nq; i++) {
    const int m = std::min(n_cand[i], max_out);
    if (m > 0) VO_CHECK(vo::copy_d2h(cand + (size_t)i * max_out, db->h_cand.as<int>() + (size_t)i * max_out, (size_t)m * 4, st, W));
  }
  if (score_out && db->size > 0) VO_CHECK(vo::copy_d2h(score_out, db->score.p, (size_t)nq * db->size * 4, st, W));
  VO_CHECK(vo::stream_sync(st, W));
  for (int i = 0; i < nq; i++)
    if (n_cand[i] > max_out) {
      vo::set_error("%s: query %d has %d candidates, max_out is %d", W, i, n_cand[i], max_out);
      return VO_ERR_CAPACITY;
    }
  return VO_OK;
}

}  // namespace

// ---- the relocalisation query on a caller's stream (the tracker's: reloc.hip)
void vo::kfdb_info(const vo_kfdb *db, int *size, int *max_batch) {
  if (size) *size = db->size;
  if (max_batch) *max_batch = db->max_batch;
}

int vo::kfdb_query_reloc_on(vo_kfdb *db, hipStream_t st, int n_queries, const int32_t *q_start, const int32_t *q_words,
                            const double *q_values, const float *stale_score, int max_out, int32_t *n_cand, int32_t *cand) {
  if (!db) return VO_ERR_INVALID;
  hipStream_t own = db->st;
  if (own != st) {  // insertions enqueued on the database's stream come first; its later work waits for the query
    if (!db->ev_in) VO_HIP_CHECK(hipEventCreateWithFlags(&db->ev_in, hipEventDisableTiming));
    if (!db->ev_out) VO_HIP_CHECK(hipEventCreateWithFlags(&db->ev_out, hipEventDisableTiming));
    VO_HIP_CHECK(hipEventRecord(db->ev_in, own));
    VO_HIP_CHECK(hipStreamWaitEvent(st, db->ev_in, 0));
  }
  db->st = st;  // (the rebuild and the query launch read the handle's stream)
  const int rc = kfdb_query_dev(db, false, n_queries, q_start, q_words, q_values, stale_score, nullptr, nullptr, nullptr, nullptr,
                                nullptr, max_out, n_cand, cand, nullptr, "vo_tracker_relocalize_db");
  db->st = own;
  VO_CHECK(rc);
  if (own != st) {
    VO_HIP_CHECK(hipEventRecord(db->ev_out, st));
    VO_HIP_CHECK(hipStreamWaitEvent(own, db->ev_out, 0));
  }
  return VO_OK;
}

// ---- the loop query of one key-frame on a caller's stream (the store's: detect_loop.hip)
vo::KfdbDevView vo::kfdb_dev_view(const vo_kfdb *db) {
  return vo::KfdbDevView{db->size, db->max_kf, db->kf_start.as<int>(), db->nbr_n.as<int>(), db->nbr.as<int>()};
}

int vo::kfdb_order_before(vo_kfdb *db, hipStream_t st) {
  if (!db) return VO_ERR_INVALID;
  if (db->st == st) return VO_OK;
  if (!db->ev_in) VO_HIP_CHECK(hipEventCreateWithFlags(&db->ev_in, hipEventDisableTiming));
  VO_HIP_CHECK(hipEventRecord(db->ev_in, db->st));
  VO_HIP_CHECK(hipStreamWaitEvent(st, db->ev_in, 0));
  return VO_OK;
}

int vo::kfdb_query_loop_on(vo_kfdb *db, hipStream_t st, const int32_t *dev_q_start, const int32_t *dev_excl_start, const int32_t *dev_excl,
                           const int32_t *dev_conn_start, const int32_t *dev_conn, float *dev_min_score, int max_out, int32_t *n_cand,
                           int32_t *cand) {
  if (!db || !dev_q_start || !dev_excl_start || !dev_excl || !dev_conn_start || !dev_conn || !dev_min_score) return VO_ERR_INVALID;
  hipStream_t own = db->st;
  VO_CHECK(kfdb_order_before(db, st));
  db->st = st;  // (the rebuild and the query launch read the handle's stream)
  int rc = kfdb_rebuild(db);
  if (rc == VO_OK) {
    hipLaunchKernelGGL(k_kfdb_min_score, dim3(1), dim3(256), 0, st, db->size, db->max_kf, db->kf_start.as<int>(), db->kf_words.as<int>(),
                       db->kf_vals.as<double>(), dev_q_start, dev_conn_start, dev_conn, dev_min_score);
    if (hipGetLastError() != hipSuccess) rc = VO_ERR_HIP;
  }
  if (rc == VO_OK)
    rc = kfdb_query_dev(db, true, 1, dev_q_start, db->kf_words.as<int>(), db->kf_vals.as<double>(), nullptr, dev_excl_start, dev_excl,
                        dev_min_score, nullptr, nullptr, max_out, n_cand, cand, nullptr, "vo_kfstore_detect_loop");
  db->st = own;
  VO_CHECK(rc);
  if (own != st) {
    if (!db->ev_out) VO_HIP_CHECK(hipEventCreateWithFlags(&db->ev_out, hipEventDisableTiming));
    VO_HIP_CHECK(hipEventRecord(db->ev_out, st));
    VO_HIP_CHECK(hipStreamWaitEvent(own, db->ev_out, 0));
  }
  return VO_OK;
}

extern "C" {

int vo_bow_vector_dev(int n_frames, int n_features, const int32_t *dev_feat_start, const int32_t *dev_word, const double *dev_weight,
                      int32_t *dev_out_start, int32_t *dev_out_words, double *dev_out_values, void *hip_stream) {
  if (n_frames < 0 || n_features < 0 || (n_frames > 0 && (!dev_feat_start || !dev_out_start)) ||
      (n_features > 0 && (!dev_word || !dev_weight || !dev_out_words || !dev_out_values)))
    return VO_ERR_INVALID;
  if (n_frames == 0) return VO_OK;
  VO_CHECK(vo::ensure_device());
  // grow-only scratch of the calling thread (the un-compacted result; keys and sums of frames beyond kBowLds features)
  thread_local vo::ScratchBuf tw, tv, tkey, tsum, cnt;
  hipStream_t st = (hipStream_t)hip_stream;
  VO_CHECK(tw.reserve(std::max<size_t>((size_t)n_features * 4, 64)));
  VO_CHECK(tv.reserve(std::max<size_t>((size_t)n_features * 8, 64)));
  VO_CHECK(tkey.reserve(std::max<size_t>((size_t)n_features * 4, 64)));
  VO_CHECK(tsum.reserve(std::max<size_t>((size_t)n_features * 8, 64)));
  VO_CHECK(cnt.reserve((size_t)n_frames * 4));
  hipLaunchKernelGGL(k_bow_vector, dim3(n_frames), dim3(256), 0, st, dev_feat_start, dev_word, dev_weight, cnt.as<int>(),
                     tkey.as<int>(), tsum.as<double>(), tw.as<int>(), tv.as<double>());
  hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(1024), 0, st, cnt.as<int>(), n_frames, dev_out_start, (int *)nullptr);
  hipLaunchKernelGGL(k_bow_compact, dim3(n_frames), dim3(256), 0, st, dev_feat_start, dev_out_start, tw.as<int>(), tv.as<double>(),
                     dev_out_words, dev_out_values);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_bow_vector(int n_frames, const int32_t *feat_start, const int32_t *word, const double *weight, int32_t *out_start,
                  int32_t *out_words, double *out_values) {
  if (n_frames < 0 || (n_frames > 0 && (!feat_start || !out_start))) return VO_ERR_INVALID;
  if (n_frames == 0) return VO_OK;
  const long long n = csr_total(feat_start, n_frames);
  if (n < 0 || n > INT_MAX || (n > 0 && (!word || !weight || !out_words || !out_values))) return VO_ERR_INVALID;
  VO_CHECK(vo::ensure_device());
  thread_local vo::ScratchBuf fs, w, wt, os, ow, ov;
  hipStream_t st = vo::thread_stream();
  const char *W = "vo_bow_vector";
  VO_CHECK(vo::upload(fs, feat_start, (size_t)(n_frames + 1) * 4, st, W));
  VO_CHECK(vo::upload(w, word, (size_t)n * 4, st, W));
  VO_CHECK(vo::upload(wt, weight, (size_t)n * 8, st, W));
  VO_CHECK(os.reserve((size_t)(n_frames + 1) * 4));
  VO_CHECK(ow.reserve(std::max<size_t>((size_t)n * 4, 64)));
  VO_CHECK(ov.reserve(std::max<size_t>((size_t)n * 8, 64)));
  VO_CHECK(vo_bow_vector_dev(n_frames, (int)n, fs.as<int>(), w.as<int>(), wt.as<double>(), os.as<int>(), ow.as<int>(), ov.as<double>(), st));
  VO_CHECK(vo::copy_d2h(out_start, os.p, (size_t)(n_frames + 1) * 4, st, W));
  VO_CHECK(vo::stream_sync(st, W));
  const int m = out_start[n_frames];
  if (m < 0 || m > n) {
    vo::set_error("vo_bow_vector: inconsistent output size %d", m);
    return VO_ERR_HIP;
  }
  VO_CHECK(vo::copy_d2h(out_words, ow.p, (size_t)m * 4, st, W));
  VO_CHECK(vo::copy_d2h(out_values, ov.p, (size_t)m * 8, st, W));
  return vo::stream_sync(st, W);
}

int vo_kfdb_create(vo_kfdb **out, int n_words, int max_keyframes, int max_words_per_keyframe, int max_batch) {
  if (!out || n_words < 1 || max_keyframes < 1 || max_words_per_keyframe < 1 || max_batch < 1) return VO_ERR_INVALID;
  const long long cap = (long long)max_keyframes * max_words_per_keyframe, slab = (long long)max_batch * max_keyframes;
  if (cap > INT_MAX || slab > INT_MAX / 2 || n_words > INT_MAX / 2) {
    vo::set_error("vo_kfdb_create: %d key-frames x %d words or %d queries x %d key-frames exceed the 32-bit index range", max_keyframes,
                  max_words_per_keyframe, max_batch, max_keyframes);
    return VO_ERR_CAPACITY;
  }
  VO_CHECK(vo::ensure_device());
  vo_kfdb *db = new (std::nothrow) vo_kfdb;
  if (!db) return VO_ERR_HIP;
  db->n_words = n_words, db->max_kf = max_keyframes, db->max_wpk = max_words_per_keyframe, db->max_batch = max_batch;
  db->cap_total = cap;
  int rc = VO_OK;
  auto R = [&](vo::DevBuf &b, size_t bytes) {
    if (rc == VO_OK) rc = b.reserve(bytes);
  };
  R(db->kf_start, (size_t)(max_keyframes + 1) * 4), R(db->kf_words, (size_t)cap * 4), R(db->kf_vals, (size_t)cap * 8);
  R(db->nbr_n, (size_t)max_keyframes * 4), R(db->nbr, (size_t)max_keyframes * kMaxNbr * 4);
  R(db->post_cnt, (size_t)(n_words + 1) * 4), R(db->post_start, (size_t)(n_words + 1) * 4);
  R(db->post_tmp, (size_t)cap * 4), R(db->post_kf, (size_t)cap * 4);
  R(db->keys, (size_t)slab * 8), R(db->order, (size_t)slab * 4), R(db->grep, (size_t)slab * 4), R(db->gsc, (size_t)slab * 4);
  R(db->g_cnt, (size_t)slab * 4), R(db->g_first, (size_t)slab * 4), R(db->score, (size_t)slab * 4), R(db->err, 64);
  if (rc == VO_OK && (hipMemset(db->kf_start.p, 0, (size_t)(max_keyframes + 1) * 4) != hipSuccess ||
                      hipMemset(db->nbr_n.p, 0, (size_t)max_keyframes * 4) != hipSuccess ||
                      hipMemset(db->post_start.p, 0, (size_t)(n_words + 1) * 4) != hipSuccess || hipMemset(db->err.p, 0, 64) != hipSuccess)) {
    vo::set_error("vo_kfdb_create: hipMemset failed");
    rc = VO_ERR_HIP;
  }
  if (rc != VO_OK) {
    delete db;
    return rc;
  }
  *out = db;
  return VO_OK;
}

void vo_kfdb_destroy(vo_kfdb *db) {
  if (!db) return;
  (void)hipStreamSynchronize(db->st);
  if (db->ev_in) (void)hipEventDestroy(db->ev_in);
  if (db->ev_out) (void)hipEventDestroy(db->ev_out);
  delete db;
}

int vo_kfdb_set_stream(vo_kfdb *db, void *hip_stream) {
  if (!db) return VO_ERR_INVALID;
  db->st = (hipStream_t)hip_stream;
  return VO_OK;
}

int vo_kfdb_size(const vo_kfdb *db) { return db ? db->size : VO_ERR_INVALID; }

int vo_kfdb_set_option(vo_kfdb *db, int option, int value) {
  if (!db || option != VO_KFDB_OPT_LDS_KEYFRAMES || value < 0) return VO_ERR_INVALID;
  db->lds_kf = std::min(value, kLdsKeyframes);
  return VO_OK;
}

static int kfdb_insert_common(vo_kfdb *db, int n, const int32_t *words, const double *values, int32_t *index, bool host) {
  if (!db || n < 0 || (n > 0 && (!words || !values))) return VO_ERR_INVALID;
  if (db->size >= db->max_kf || n > db->max_wpk) {
    vo::set_error("vo_kfdb_insert: key-frame %d with %d words exceeds the database (%d key-frames, %d words each)", db->size, n,
                  db->max_kf, db->max_wpk);
    return VO_ERR_CAPACITY;
  }
  const char *W = "vo_kfdb_insert";
  if (host)
    for (int i = 0; i < n; i++)
      if (words[i] < 0 || words[i] >= db->n_words || (i > 0 && words[i] <= words[i - 1])) {
        vo::set_error("vo_kfdb_insert: word ids must ascend strictly within [0, %d)", db->n_words);
        return VO_ERR_INVALID;
      }
  int *dw = db->kf_words.as<int>() + db->total;
  double *dv = db->kf_vals.as<double>() + db->total;
  if (host) {
    // (the caller's arrays may be reused as soon as the call returns: stage through the handle, in stream order)
    VO_CHECK(vo::copy_h2d(dw, words, (size_t)n * 4, db->st, W));
    VO_CHECK(vo::copy_h2d(dv, values, (size_t)n * 8, db->st, W));
    VO_CHECK(vo::stream_sync(db->st, W));
  } else if (n > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(dw, words, (size_t)n * 4, hipMemcpyDeviceToDevice, db->st));
    VO_HIP_CHECK(hipMemcpyAsync(dv, values, (size_t)n * 8, hipMemcpyDeviceToDevice, db->st));
  }
  hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, db->st, db->kf_start.as<int>() + db->size + 1, (int)(db->total + n));
  VO_HIP_CHECK(hipGetLastError());
  if (index) *index = db->size;
  db->size++, db->total += n, db->dirty = true;
  return VO_OK;
}

int vo_kfdb_insert(vo_kfdb *db, int n, const int32_t *words, const double *values, int32_t *index) {
  return kfdb_insert_common(db, n, words, values, index, true);
}
int vo_kfdb_insert_dev(vo_kfdb *db, int n, const int32_t *dev_words, const double *dev_values, int32_t *index) {
  return kfdb_insert_common(db, n, dev_words, dev_values, index, false);
}

int vo_kfdb_set_neighbors(vo_kfdb *db, int keyframe, int n, const int32_t *ids) {
  if (!db || keyframe < 0 || keyframe >= db->size || n < 0 || n > kMaxNbr || (n > 0 && !ids)) return VO_ERR_INVALID;
  NbrRow r{};
  r.n = n;
  for (int i = 0; i < n; i++) {
    if (ids[i] < 0 || ids[i] >= db->size) return VO_ERR_INVALID;
    r.id[i] = ids[i];
  }
  hipLaunchKernelGGL(k_set_nbr, dim3(1), dim3(64), 0, db->st, db->nbr_n.as<int>(), db->nbr.as<int>(), keyframe, r);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_kfdb_set_neighbors_batch(vo_kfdb *db, int first, int count, const int32_t *n, const int32_t *ids) {
  if (!db || first < 0 || count < 0 || first + (long long)count > db->size || (count > 0 && (!n || !ids))) return VO_ERR_INVALID;
  if (count == 0) return VO_OK;
  std::vector<int32_t> rows((size_t)count * kMaxNbr, -1);
  for (int k = 0; k < count; k++) {
    if (n[k] < 0 || n[k] > kMaxNbr) return VO_ERR_INVALID;
    for (int i = 0; i < n[k]; i++) {
      const int32_t id = ids[(size_t)k * kMaxNbr + i];
      if (id < 0 || id >= db->size) return VO_ERR_INVALID;
      rows[(size_t)k * kMaxNbr + i] = id;
    }
  }
  const char *W = "vo_kfdb_set_neighbors_batch";
  VO_CHECK(vo::copy_h2d(db->nbr_n.as<int>() + first, n, (size_t)count * 4, db->st, W));
  VO_CHECK(vo::copy_h2d(db->nbr.as<int>() + (size_t)first * kMaxNbr, rows.data(), rows.size() * 4, db->st, W));
  return vo::stream_sync(db->st, W);  // (rows is a local: the copies must have read it)
}

int vo_kfdb_get_neighbors(vo_kfdb *db, int keyframe, int32_t *n, int32_t *ids) {
  const char *W = "vo_kfdb_get_neighbors";
  if (!db || keyframe < 0 || keyframe >= db->size || !n || !ids) return VO_ERR_INVALID;
  VO_CHECK(vo::copy_d2h(n, db->nbr_n.as<int>() + keyframe, 4, db->st, W));
  VO_CHECK(vo::copy_d2h(ids, db->nbr.as<int>() + (size_t)keyframe * kMaxNbr, kMaxNbr * 4, db->st, W));
  return vo::stream_sync(db->st, W);
}

int vo_kfdb_query_reloc(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                        const float *stale_score, int max_out, int32_t *n_cand, int32_t *cand, float *score_out) {
  return kfdb_query_host(db, false, n_queries, q_start, q_words, q_values, stale_score, nullptr, nullptr, nullptr, nullptr, nullptr,
                         max_out, n_cand, cand, score_out, "vo_kfdb_query_reloc");
}
int vo_kfdb_query_reloc_dev(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                            const float *stale_score, int max_out, int32_t *n_cand, int32_t *cand, float *score_out) {
  return kfdb_query_dev(db, false, n_queries, q_start, q_words, q_values, stale_score, nullptr, nullptr, nullptr, nullptr, nullptr,
                        max_out, n_cand, cand, score_out, "vo_kfdb_query_reloc_dev");
}
int vo_kfdb_query_loop(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                       const int32_t *excl_start, const int32_t *excl, const float *min_score, const int32_t *conn_start,
                       const int32_t *conn, int max_out, int32_t *n_cand, int32_t *cand, float *score_out) {
  return kfdb_query_host(db, true, n_queries, q_start, q_words, q_values, nullptr, excl_start, excl, min_score, conn_start, conn,
                         max_out, n_cand, cand, score_out, "vo_kfdb_query_loop");
}
int vo_kfdb_query_loop_dev(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                           const int32_t *excl_start, const int32_t *excl, const float *min_score, const int32_t *conn_start,
                           const int32_t *conn, int max_out, int32_t *n_cand, int32_t *cand, float *score_out) {
  return kfdb_query_dev(db, true, n_queries, q_start, q_words, q_values, nullptr, excl_start, excl, min_score, conn_start, conn,
                        max_out, n_cand, cand, score_out, "vo_kfdb_query_loop_dev");
}

}  // extern "C"
