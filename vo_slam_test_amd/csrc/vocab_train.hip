// vocab_train.hip -- DBoW3::Vocabulary::create as Map::createVocabulary calls it (reference src/map.cpp:60-99): the
// k-majority tree over 256-bit ORB descriptors, trained on the device.  Contract, deviations from DBoW3 and the numpy
// restatement that pins it (tests/vocab_ref.py): DESIGN.md §4d.  Integer arithmetic throughout; the idf's log is host libm.
//
// Level-synchronous: the nodes of one tree level that are clustered further form one segmented batch.  A segment is the
// contiguous range of one node's descriptors in the level's descriptor buffer (the buffer is physically re-ordered by
// k_vt_scatter at the end of every level, so every phase reads 32 contiguous bytes per lane); it is cut into chunks of 256
// descriptors, one workgroup each, so that level 1 (one segment of n) and level 5 (10^4 segments of a few dozen) go through
// the same kernels.  What crosses workgroups (the k-means++ running sums of a large segment, its bit counters, the stable
// partition's offsets) crosses at a kernel boundary: per-chunk partials, then one workgroup per segment.  The host reads one
// word per Lloyd iteration ("segments still moving") and does the tree's bookkeeping (node ids, child lists: n_nodes
// entries) once per level from the per-cluster counts.
#include <algorithm>
#include <cmath>
#include <vector>

#include "vo_common.h"

namespace {

constexpr int kChunk = 256;  // descriptors per chunk = threads per workgroup
constexpr int kMaxK = VO_VOCAB_MAX_K;

__host__ __device__ inline unsigned long long vt_mix(unsigned long long z) {  // splitmix64's step
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
__host__ __device__ inline unsigned long long vt_draw(unsigned long long key, unsigned j) { return vt_mix(vt_mix(key) + j); }

struct LevelDev {
  int S, C, k;
  // per segment (read-only in the kernels)
  const int *seg_start, *seg_size, *seg_chunk0, *seg_slot;  // slot: index of the segment's global counters, -1 = one chunk
  const unsigned long long *seg_key;
  const int *chunk_seg;  // [C]
  // per segment state
  int *ncent, *done, *moved, *iters, *capped;
  uint32_t *centres;  // [S][k][8]
  int *seg_counts;    // [S][k] members per cluster of the final assignment
  // per descriptor position
  uint8_t *assign;
  int *min_dist;
  // per chunk
  uint32_t *chunk_sum;  // [C] sum of min_dist
  int *chunk_hist;      // [C][k] members per cluster, then (k_vt_scan) the chunk's first offset per cluster in its segment
  uint32_t *big;        // [slots][k][257] bit counters + member count of the segments that span chunks
  int *n_moving;        // [1]
};

__device__ __forceinline__ int vt_dist(const uint32_t (&d)[8], const uint32_t *c) {
  int s = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) s += __popc(d[w] ^ c[w]);
  return s;
}
__device__ __forceinline__ void vt_load(const uint32_t *D, long long pos, uint32_t (&d)[8]) {
  const uint4 a = reinterpret_cast<const uint4 *>(D)[2 * pos], b = reinterpret_cast<const uint4 *>(D)[2 * pos + 1];
  d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w, d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
}

// inclusive scan over the 256 threads of a workgroup (buf: 512 entries); the caller reads buf-independent results only
__device__ unsigned long long vt_block_scan(unsigned long long v, unsigned long long *buf, unsigned long long *total) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  int in = 0;
  for (int o = 1; o < kChunk; o <<= 1) {
    unsigned long long x = buf[in * kChunk + t];
    if (t >= o) x += buf[in * kChunk + t - o];
    buf[(in ^ 1) * kChunk + t] = x;
    in ^= 1;
    __syncthreads();
  }
  *total = buf[in * kChunk + kChunk - 1];
  return buf[in * kChunk + t];
}

// ---- k-means++ seeding (initiateClustersKMpp with the integer draw) ------------------------------------------------
// first centre of every segment; a segment of <= k descriptors is its own clustering (one cluster per descriptor)
__global__ __launch_bounds__(64) void k_vt_seed_first(LevelDev V, const uint32_t *D) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int size = V.seg_size[s], start = V.seg_start[s];
  uint32_t *cen = V.centres + (size_t)s * V.k * 8;
  if (size <= V.k) {
    for (int i = lane; i < size * 8; i += 64) cen[i] = D[(size_t)start * 8 + i];
    for (int i = lane; i < size; i += 64) V.assign[start + i] = (uint8_t)i;
  } else {
    const int pick = (int)(vt_draw(V.seg_key[s], 0) % (unsigned long long)size);
    if (lane < 8) cen[lane] = D[((size_t)start + pick) * 8 + lane];
  }
  if (lane == 0) {
    V.ncent[s] = size <= V.k ? size : 1;
    V.done[s] = size <= V.k, V.moved[s] = 0, V.iters[s] = 0, V.capped[s] = 0;
  }
}

// round r: distance to centre r - 1 into min_dist, the chunk's sum of min_dist
__global__ __launch_bounds__(kChunk) void k_vt_seed_dist(LevelDev V, const uint32_t *D, int r) {
  const int b = blockIdx.x, seg = V.chunk_seg[b], t = threadIdx.x;
  if (V.done[seg] || V.ncent[seg] != r) return;  // small segment, or seeding ended early (all remaining coincide with a centre)
  const int off = (b - V.seg_chunk0[seg]) * kChunk + t;
  const bool valid = off < V.seg_size[seg];
  const long long pos = (long long)V.seg_start[seg] + off;
  int md = 0;
  if (valid) {
    uint32_t d[8];
    vt_load(D, pos, d);
    md = vt_dist(d, V.centres + ((size_t)seg * V.k + (r - 1)) * 8);
    if (r == 1) V.assign[pos] = 0xFF;
    else md = min(md, V.min_dist[pos]);
    V.min_dist[pos] = md;
  }
  __shared__ int part[kChunk / 64];
  int s = md;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  if (t == 0) V.chunk_sum[b] = (uint32_t)(part[0] + part[1] + part[2] + part[3]);
}

// round r: sum over the segment, cut = 1 + draw(r) mod sum, centre r = the first descriptor whose running sum reaches cut
__global__ __launch_bounds__(kChunk) void k_vt_seed_pick(LevelDev V, const uint32_t *D, int r) {
  const int s = blockIdx.x, t = threadIdx.x;
  if (V.done[s] || V.ncent[s] != r) return;
  __shared__ unsigned long long buf[2 * kChunk];
  __shared__ unsigned long long sh_cut;
  __shared__ int sh_chunk, sh_pick;
  if (t == 0) sh_chunk = 0, sh_pick = 0, sh_cut = 0;
  const int size = V.seg_size[s], start = V.seg_start[s], chunk0 = V.seg_chunk0[s];
  const int nch = (size + kChunk - 1) / kChunk, per = (nch + kChunk - 1) / kChunk;
  const int lo = min(nch, t * per), hi = min(nch, lo + per);
  unsigned long long mine = 0, total;
  for (int c = lo; c < hi; c++) mine += V.chunk_sum[chunk0 + c];
  const unsigned long long incl = vt_block_scan(mine, buf, &total);
  if (total == 0) return;  // uniform: every remaining descriptor coincides with a centre -- fewer than k centres
  const unsigned long long cut = 1 + vt_draw(V.seg_key[s], (unsigned)r) % total;
  if (incl - mine < cut && cut <= incl) {  // exactly one thread
    unsigned long long run = incl - mine;
    for (int c = lo; c < hi; c++) {
      const unsigned long long cs = V.chunk_sum[chunk0 + c];
      if (run + cs >= cut) {
        sh_chunk = c, sh_cut = cut - run;
        break;
      }
      run += cs;
    }
  }
  __syncthreads();
  const int off = sh_chunk * kChunk + t;
  const unsigned long long md = off < size ? (unsigned long long)V.min_dist[start + off] : 0ULL, ccut = sh_cut;
  unsigned long long ctotal;
  const unsigned long long ci = vt_block_scan(md, buf, &ctotal);
  if (ci - md < ccut && ccut <= ci) sh_pick = off;
  __syncthreads();
  if (t < 8) V.centres[((size_t)s * V.k + r) * 8 + t] = D[((size_t)start + sh_pick) * 8 + t];
  if (t == 0) V.ncent[s] = r + 1;
}

// ---- Lloyd --------------------------------------------------------------------------------------------------------
// nearest centre per descriptor, ties to the lowest cluster index (strict <); raises the segment's flag on any change
__global__ __launch_bounds__(kChunk) void k_vt_assign(LevelDev V, const uint32_t *D) {
  const int b = blockIdx.x, seg = V.chunk_seg[b], t = threadIdx.x;
  if (V.done[seg]) return;
  __shared__ uint32_t cen[kMaxK * 8];
  const int nc = V.ncent[seg];
  if (t < nc * 8) cen[t] = V.centres[(size_t)seg * V.k * 8 + t];
  __syncthreads();
  const int off = (b - V.seg_chunk0[seg]) * kChunk + t;
  const bool valid = off < V.seg_size[seg];
  const long long pos = (long long)V.seg_start[seg] + off;
  bool changed = false;
  if (valid) {
    uint32_t d[8];
    vt_load(D, pos, d);
    int best = 0, bestd = 1 << 30;
    for (int c = 0; c < nc; c++) {
      const int dist = vt_dist(d, cen + c * 8);
      if (dist < bestd) bestd = dist, best = c;
    }
    changed = V.assign[pos] != (uint8_t)best;
    if (changed) V.assign[pos] = (uint8_t)best;
  }
  const unsigned long long any = __ballot(changed);
  if (any && (t & 63) == 0) atomicOr(&V.moved[seg], 1);
}

// majority of one cluster's 256 bit counters (DescManip::meanValue): bit set iff count >= m / 2 + m % 2; a wave's ballot
// is 64 bits of the centre.  cnt: 257 counters (shared or global), [256] = m.  m == 0 keeps the centre.
template <class P>
__device__ __forceinline__ void vt_majority(P cnt, uint32_t *centre) {
  const int t = threadIdx.x;
  const uint32_t m = cnt[256];
  if (m == 0) return;  // uniform
  const unsigned long long bits = __ballot(cnt[t] >= (m >> 1) + (m & 1));
  if ((t & 63) == 0) centre[(t >> 6) * 2] = (uint32_t)bits, centre[(t >> 6) * 2 + 1] = (uint32_t)(bits >> 32);
}

// bit counters of the segments that moved: a wave turns its 64 descriptors into 256 lane masks by ballot (lane j keeps
// bits j, j + 64, j + 128, j + 192), a cluster's count of a bit is the popcount of (bit mask & cluster mask); workgroup
// counters in LDS; a one-chunk segment takes its majority here, a larger one adds into its global counters
__global__ __launch_bounds__(kChunk) void k_vt_update(LevelDev V, const uint32_t *D) {
  const int b = blockIdx.x, seg = V.chunk_seg[b], t = threadIdx.x, lane = t & 63;
  if (!V.moved[seg]) return;  // converged (now or earlier) or small
  __shared__ uint32_t cnt[kMaxK * 257];
  const int nc = V.ncent[seg];
  for (int i = t; i < nc * 257; i += kChunk) cnt[i] = 0;
  __syncthreads();
  const int off = (b - V.seg_chunk0[seg]) * kChunk + t;
  const bool valid = off < V.seg_size[seg];
  const long long pos = (long long)V.seg_start[seg] + off;
  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int a = -1;
  if (valid) {
    vt_load(D, pos, d);
    a = V.assign[pos];
  }
  unsigned long long mine[4] = {0, 0, 0, 0};
#pragma unroll
  for (int w = 0; w < 8; w++)
#pragma unroll
    for (int bit = 0; bit < 32; bit++) {
      const unsigned long long m = __ballot((d[w] >> bit) & 1u);
      if (lane == ((w * 32 + bit) & 63)) mine[(w * 32 + bit) >> 6] = m;
    }
  for (int c = 0; c < nc; c++) {
    const unsigned long long mc = __ballot(a == c);
    if (mc == 0) continue;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int v = __popcll(mine[q] & mc);
      if (v) atomicAdd(&cnt[c * 257 + q * 64 + lane], (uint32_t)v);
    }
    if (lane == 0) atomicAdd(&cnt[c * 257 + 256], (uint32_t)__popcll(mc));
  }
  __syncthreads();
  const int slot = V.seg_slot[seg];
  if (slot < 0) {
    for (int c = 0; c < nc; c++) vt_majority(cnt + c * 257, V.centres + ((size_t)seg * V.k + c) * 8);
  } else {
    uint32_t *g = V.big + (size_t)slot * V.k * 257;
    for (int i = t; i < nc * 257; i += kChunk)
      if (cnt[i]) atomicAdd(&g[i], cnt[i]);
  }
}

// end of iteration `it` for every segment: the majority of a segment that spans chunks (counters re-zeroed), and the state:
// not moved -> converged after `it` assignments; moved at the cap -> stops with its last assignment, counted as capped
__global__ __launch_bounds__(kChunk) void k_vt_majority(LevelDev V, int it, int cap) {
  const int s = blockIdx.x, t = threadIdx.x;
  if (V.done[s]) return;
  const int mv = V.moved[s], slot = V.seg_slot[s], nc = V.ncent[s];
  if (mv && it < cap && slot >= 0) {
    uint32_t *g = V.big + (size_t)slot * V.k * 257;
    for (int c = 0; c < nc; c++) {
      vt_majority(g + c * 257, V.centres + ((size_t)s * V.k + c) * 8);
      __syncthreads();
      g[c * 257 + t] = 0;
      if (t == 0) g[c * 257 + 256] = 0;
    }
  }
  __syncthreads();
  if (t == 0) {
    if (!mv) V.done[s] = 1, V.iters[s] = it;
    else if (it >= cap) V.done[s] = 1, V.iters[s] = it, V.capped[s] = 1;
    else V.moved[s] = 0, atomicAdd(V.n_moving, 1);
  }
}

// ---- stable partition of every segment by cluster -------------------------------------------------------------------
__global__ __launch_bounds__(kChunk) void k_vt_hist(LevelDev V) {
  const int b = blockIdx.x, seg = V.chunk_seg[b], t = threadIdx.x;
  __shared__ int h[kMaxK];
  if (t < kMaxK) h[t] = 0;
  __syncthreads();
  const int off = (b - V.seg_chunk0[seg]) * kChunk + t;
  const int a = off < V.seg_size[seg] ? (int)V.assign[(long long)V.seg_start[seg] + off] : -1;
  const int nc = V.ncent[seg];
  for (int c = 0; c < nc; c++) {
    const unsigned long long mc = __ballot(a == c);
    if (mc && (t & 63) == 0) atomicAdd(&h[c], __popcll(mc));
  }
  __syncthreads();
  if (t < V.k) V.chunk_hist[(size_t)b * V.k + t] = h[t];
}

// one wave per segment, lane = cluster: counts -> first offset of (chunk, cluster) within the segment, clusters in order
__global__ __launch_bounds__(64) void k_vt_scan(LevelDev V) {
  const int s = blockIdx.x, c = threadIdx.x;
  __shared__ int base[kMaxK];
  const int nch = (V.seg_size[s] + kChunk - 1) / kChunk, chunk0 = V.seg_chunk0[s];
  int total = 0;
  if (c < V.k) {
    for (int ch = 0; ch < nch; ch++) {
      int *p = &V.chunk_hist[(size_t)(chunk0 + ch) * V.k + c];
      const int h = *p;
      *p = total;
      total += h;
    }
    V.seg_counts[(size_t)s * V.k + c] = total;
    base[c] = total;
  }
  __syncthreads();
  if (c == 0) {
    int run = 0;
    for (int i = 0; i < V.k; i++) {
      const int x = base[i];
      base[i] = run;
      run += x;
    }
  }
  __syncthreads();
  if (c < V.k && base[c])
    for (int ch = 0; ch < nch; ch++) V.chunk_hist[(size_t)(chunk0 + ch) * V.k + c] += base[c];
}

__global__ __launch_bounds__(kChunk) void k_vt_scatter(LevelDev V, const uint32_t *D, uint32_t *Dout) {
  const int b = blockIdx.x, seg = V.chunk_seg[b], t = threadIdx.x, lane = t & 63, wave = t >> 6;
  __shared__ int wcount[kChunk / 64][kMaxK];
  const int off = (b - V.seg_chunk0[seg]) * kChunk + t;
  const bool valid = off < V.seg_size[seg];
  const long long start = V.seg_start[seg], pos = start + off;
  const int a = valid ? (int)V.assign[pos] : -1;
  const int nc = V.ncent[seg];
  int rank = 0;
  for (int c = 0; c < nc; c++) {
    const unsigned long long mc = __ballot(a == c);
    if (a == c) rank = __popcll(mc & ((1ULL << lane) - 1ULL));
    if (lane == 0) wcount[wave][c] = __popcll(mc);
  }
  __syncthreads();
  if (!valid) return;
  int dst = V.chunk_hist[(size_t)b * V.k + a] + rank;
  for (int w = 0; w < wave; w++) dst += wcount[w][a];
  const uint4 *src = reinterpret_cast<const uint4 *>(D) + 2 * pos;
  uint4 *out = reinterpret_cast<uint4 *>(Dout) + 2 * (start + dst);
  out[0] = src[0], out[1] = src[1];
}

// ---- idf: Ni[w] = number of images with a descriptor whose word is w.  One (word, image) pair is counted once: the first
// thread to insert it into an open-addressing table (2n slots or more, at most n keys: a probe always ends) adds to Ni.
__global__ __launch_bounds__(256) void k_vt_presence(int n, const int *word, int n_images, const int *image_offsets,
                                                     unsigned long long *table, unsigned long long mask, int *Ni) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int w = word[i];
  if (w < 0) return;
  int lo = 0, hi = n_images;  // the last image m with image_offsets[m] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (image_offsets[mid] <= i) lo = mid;
    else hi = mid;
  }
  const unsigned long long key = (((unsigned long long)(unsigned)w << 32) | (unsigned)lo) + 1ULL;
  unsigned long long h = vt_mix(key) & mask;
  for (;;) {
    const unsigned long long prev = atomicCAS(&table[h], 0ULL, key);
    if (prev == 0ULL) {
      atomicAdd(&Ni[w], 1);
      return;
    }
    if (prev == key) return;
    h = (h + 1) & mask;
  }
}

struct Seg {
  int start, size, node;
  unsigned long long key;
};

struct Work {  // device buffers of one training call (a one-off: released when it ends)
  vo::OwnedDevBuf d[24];
};

int train_resident(int n, const uint8_t *d_desc, int n_images, const int32_t *h_off, const int32_t *d_off, int k, int L,
                   uint64_t seed, hipStream_t st, vo_vocab **out, vo_vocab_train_info *info) {
  const char *W = "vo_vocab_train";
  Work wk;
  vo::DevBuf &bD0 = wk.d[0], &bD1 = wk.d[1], &bAssign = wk.d[2], &bMin = wk.d[3], &bSegI = wk.d[4], &bKey = wk.d[5],
             &bChunkSeg = wk.d[6], &bState = wk.d[7], &bCen = wk.d[8], &bCounts = wk.d[9], &bChunkSum = wk.d[10],
             &bHist = wk.d[11], &bBig = wk.d[12], &bMoving = wk.d[13];
  // the tree, breadth-first: node 0 = root; the children of the nodes of one level are numbered in node order, so the
  // child list of the whole tree is 1, 2, 3, ... and child_start is the running sum of the child counts
  std::vector<int32_t> n_child(1, 0), level(1, 0);
  std::vector<uint8_t> node_desc(32, 0);
  int it_max = 0, n_capped = 0;
  if (n > 0) {
    VO_CHECK(bD0.reserve((size_t)n * 32));
    VO_CHECK(bD1.reserve((size_t)n * 32));
    VO_CHECK(bAssign.reserve((size_t)n));
    VO_CHECK(bMin.reserve((size_t)n * 4));
    VO_CHECK(bMoving.reserve(64));
    VO_HIP_CHECK(hipMemcpyAsync(bD0.p, d_desc, (size_t)n * 32, hipMemcpyDeviceToDevice, st));
  }
  uint32_t *D = bD0.as<uint32_t>(), *Dn = bD1.as<uint32_t>();
  std::vector<Seg> segs;
  if (n > 0) segs.push_back(Seg{0, n, 0, vt_mix(seed)});
  std::vector<int32_t> segi, chunk_seg, h_state, h_counts;
  std::vector<unsigned long long> keys;
  std::vector<uint32_t> h_cen;
  while (!segs.empty()) {
    const int S = (int)segs.size();
    // the level's batch: segments, their chunks, the global counters of the segments that span chunks
    segi.assign((size_t)4 * S, 0), keys.resize(S), chunk_seg.clear();
    int slots = 0, n_lloyd = 0;
    for (int s = 0; s < S; s++) {
      const int nch = (segs[s].size + kChunk - 1) / kChunk;
      segi[s] = segs[s].start, segi[S + s] = segs[s].size, segi[2 * S + s] = (int)chunk_seg.size();
      segi[3 * S + s] = nch > 1 ? slots++ : -1;
      keys[s] = segs[s].key;
      chunk_seg.insert(chunk_seg.end(), nch, s);
      n_lloyd += segs[s].size > k;
    }
    const int C = (int)chunk_seg.size();
    VO_CHECK(vo::upload(bSegI, segi.data(), segi.size() * 4, st, W));
    VO_CHECK(vo::upload(bKey, keys.data(), keys.size() * 8, st, W));
    VO_CHECK(vo::upload(bChunkSeg, chunk_seg.data(), (size_t)C * 4, st, W));
    VO_CHECK(bState.reserve((size_t)5 * S * 4));
    VO_CHECK(bCen.reserve((size_t)S * k * 32));
    VO_CHECK(bCounts.reserve((size_t)S * k * 4));
    VO_CHECK(bChunkSum.reserve((size_t)C * 4));
    VO_CHECK(bHist.reserve((size_t)C * k * 4));
    VO_CHECK(bBig.reserve(std::max<size_t>((size_t)slots * k * 257 * 4, 64)));
    if (slots) VO_HIP_CHECK(hipMemsetAsync(bBig.p, 0, (size_t)slots * k * 257 * 4, st));
    LevelDev V{};
    V.S = S, V.C = C, V.k = k;
    V.seg_start = bSegI.as<int>(), V.seg_size = V.seg_start + S, V.seg_chunk0 = V.seg_start + 2 * S, V.seg_slot = V.seg_start + 3 * S;
    V.seg_key = bKey.as<unsigned long long>(), V.chunk_seg = bChunkSeg.as<int>();
    V.ncent = bState.as<int>(), V.done = V.ncent + S, V.moved = V.ncent + 2 * S, V.iters = V.ncent + 3 * S, V.capped = V.ncent + 4 * S;
    V.centres = bCen.as<uint32_t>(), V.seg_counts = bCounts.as<int>(), V.assign = bAssign.as<uint8_t>(), V.min_dist = bMin.as<int>();
    V.chunk_sum = bChunkSum.as<uint32_t>(), V.chunk_hist = bHist.as<int>(), V.big = bBig.as<uint32_t>(), V.n_moving = bMoving.as<int>();

    hipLaunchKernelGGL(k_vt_seed_first, dim3(S), dim3(64), 0, st, V, D);
    if (n_lloyd) {
      for (int r = 1; r < k; r++) {
        hipLaunchKernelGGL(k_vt_seed_dist, dim3(C), dim3(kChunk), 0, st, V, D, r);
        hipLaunchKernelGGL(k_vt_seed_pick, dim3(S), dim3(kChunk), 0, st, V, D, r);
      }
      // Lloyd: one word read per iteration
      for (int it = 1; it <= VO_VOCAB_MAX_LLOYD; it++) {
        hipLaunchKernelGGL(k_vt_assign, dim3(C), dim3(kChunk), 0, st, V, D);
        if (it < VO_VOCAB_MAX_LLOYD) hipLaunchKernelGGL(k_vt_update, dim3(C), dim3(kChunk), 0, st, V, D);
        VO_HIP_CHECK(hipMemsetAsync(V.n_moving, 0, 4, st));
        hipLaunchKernelGGL(k_vt_majority, dim3(S), dim3(kChunk), 0, st, V, it, (int)VO_VOCAB_MAX_LLOYD);
        VO_HIP_CHECK(hipGetLastError());
        int moving = 0;
        VO_CHECK(vo::copy_d2h(&moving, V.n_moving, 4, st, W));
        VO_CHECK(vo::stream_sync(st, W));
        if (moving == 0) break;
      }
    }
    hipLaunchKernelGGL(k_vt_hist, dim3(C), dim3(kChunk), 0, st, V);
    hipLaunchKernelGGL(k_vt_scan, dim3(S), dim3(64), 0, st, V);
    hipLaunchKernelGGL(k_vt_scatter, dim3(C), dim3(kChunk), 0, st, V, D, Dn);
    VO_HIP_CHECK(hipGetLastError());
    h_state.resize((size_t)5 * S), h_counts.resize((size_t)S * k), h_cen.resize((size_t)S * k * 8);
    VO_CHECK(vo::copy_d2h(h_state.data(), bState.p, h_state.size() * 4, st, W));
    VO_CHECK(vo::copy_d2h(h_counts.data(), bCounts.p, h_counts.size() * 4, st, W));
    VO_CHECK(vo::copy_d2h(h_cen.data(), bCen.p, h_cen.size() * 4, st, W));
    VO_CHECK(vo::stream_sync(st, W));
    // bookkeeping: every cluster is a child; it is clustered further iff its level < L and it holds more than one descriptor
    std::vector<Seg> next;
    for (int s = 0; s < S; s++) {
      const int nc = h_state[s], lvl = level[segs[s].node] + 1;
      it_max = std::max(it_max, h_state[3 * S + s]), n_capped += h_state[4 * S + s];
      n_child[segs[s].node] = nc;
      int run = 0;
      for (int c = 0; c < nc; c++) {
        const int child = (int)n_child.size(), cnt = h_counts[(size_t)s * k + c];
        n_child.push_back(0), level.push_back(lvl);
        const uint8_t *cd = reinterpret_cast<const uint8_t *>(&h_cen[((size_t)s * k + c) * 8]);
        node_desc.insert(node_desc.end(), cd, cd + 32);
        if (lvl < L && cnt > 1) next.push_back(Seg{segs[s].start + run, cnt, child, vt_mix(segs[s].key ^ (unsigned long long)(c + 1))});
        run += cnt;
      }
      if (run != segs[s].size) {
        vo::set_error("%s: the partition of node %d lost descriptors (%d of %d)", W, segs[s].node, run, segs[s].size);
        return VO_ERR_HIP;
      }
    }
    segs.swap(next);
    std::swap(D, Dn);
  }
  const int N = (int)n_child.size();
  std::vector<int32_t> cs(N + 1, 0), ch(std::max(N - 1, 0)), wid(N, -1), word_node;
  for (int i = 0; i < N; i++) {
    cs[i + 1] = cs[i] + n_child[i];
    if (i > 0) ch[i - 1] = i;
    if (i > 0 && n_child[i] == 0) wid[i] = (int32_t)word_node.size(), word_node.push_back(i);
  }
  const int n_words = (int)word_node.size();
  std::vector<double> wt(N, 0.0);
  vo_vocab *v = nullptr;
  VO_CHECK(vo_vocab_create(&v, N, L, cs.data(), ch.data(), node_desc.data(), wt.data(), wid.data()));
  // setNodeWeights: idf over the images by transform of the training set (DBoW does not reuse the partition)
  if (n > 0 && n_words > 0) {
    vo::DevBuf &bWord = wk.d[14], &bWt = wk.d[15], &bNode = wk.d[16], &bTable = wk.d[17], &bNi = wk.d[18];
    size_t slots = 1024;
    while (slots < 2 * (size_t)n) slots <<= 1;
    int rc = VO_OK;
    std::vector<int32_t> ni(n_words, 0);
    auto run = [&]() -> int {
      VO_CHECK(bWord.reserve((size_t)n * 4));
      VO_CHECK(bWt.reserve((size_t)n * 8));
      VO_CHECK(bNode.reserve((size_t)n * 4));
      VO_CHECK(bTable.reserve(slots * 8));
      VO_CHECK(bNi.reserve((size_t)n_words * 4));
      VO_HIP_CHECK(hipMemsetAsync(bTable.p, 0, slots * 8, st));
      VO_HIP_CHECK(hipMemsetAsync(bNi.p, 0, (size_t)n_words * 4, st));
      VO_CHECK(vo::vocab_transform_resident(v, n, reinterpret_cast<const uint32_t *>(d_desc), 0, bWord.as<int>(), bWt.as<double>(),
                                            bNode.as<int>(), st));
      hipLaunchKernelGGL(k_vt_presence, dim3((n + 255) / 256), dim3(256), 0, st, n, bWord.as<int>(), n_images, d_off,
                         bTable.as<unsigned long long>(), (unsigned long long)(slots - 1), bNi.as<int>());
      VO_HIP_CHECK(hipGetLastError());
      VO_CHECK(vo::copy_d2h(ni.data(), bNi.p, (size_t)n_words * 4, st, W));
      VO_CHECK(vo::stream_sync(st, W));
      for (int w = 0; w < n_words; w++)
        if (ni[w] > 0) wt[word_node[w]] = std::log((double)n_images / (double)ni[w]);
      return vo::vocab_set_weights(v, wt.data(), st);
    };
    if ((rc = run()) != VO_OK) {
      vo_vocab_destroy(v);
      return rc;
    }
  }
  if (info) {
    info->n_nodes = N, info->n_words = n_words, info->n_levels = *std::max_element(level.begin(), level.end());
    info->lloyd_iterations_max = it_max, info->n_capped = n_capped;
  }
  *out = v;
  return VO_OK;
}

int check_args(const char *W, int n_desc, const void *desc, int n_images, const void *off, int k, int L, vo_vocab **out) {
  if (!out || n_desc < 0 || n_images < 0 || !off || (n_desc > 0 && !desc) || k < 2 || L < 1) {
    vo::set_error("%s: needs out, n_desc >= 0 (with descriptors), image_offsets[n_images + 1], k >= 2, L >= 1", W);
    return VO_ERR_INVALID;
  }
  if (k > VO_VOCAB_MAX_K || L > VO_VOCAB_MAX_L || n_desc > VO_VOCAB_MAX_DESC) {
    vo::set_error("%s: k = %d, L = %d, %d descriptors exceed the limits %d, %d, %d", W, k, L, n_desc, VO_VOCAB_MAX_K, VO_VOCAB_MAX_L,
                  VO_VOCAB_MAX_DESC);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

int check_offsets(const char *W, int n_desc, int n_images, const int32_t *off) {
  bool ok = off[0] == 0 && off[n_images] == n_desc;
  for (int m = 0; ok && m < n_images; m++) ok = off[m] <= off[m + 1];
  if (!ok) {
    vo::set_error("%s: image_offsets must start at 0, ascend and end at n_desc = %d", W, n_desc);
    return VO_ERR_INVALID;
  }
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_vocab_train(int n_desc, const uint8_t *desc, int n_images, const int32_t *image_offsets, int k, int L, uint64_t seed,
                   vo_vocab **out, vo_vocab_train_info *info) {
  const char *W = "vo_vocab_train";
  VO_CHECK(check_args(W, n_desc, desc, n_images, image_offsets, k, L, out));
  VO_CHECK(check_offsets(W, n_desc, n_images, image_offsets));
  VO_CHECK(vo::ensure_device());
  hipStream_t st = vo::thread_stream();
  vo::OwnedDevBuf d_desc, d_off;  // (released on return, behind the synchronisation)
  int rc = vo::upload(d_desc, desc, (size_t)n_desc * 32, st, W);
  if (rc == VO_OK) rc = vo::upload(d_off, image_offsets, (size_t)(n_images + 1) * 4, st, W);
  if (rc == VO_OK) rc = train_resident(n_desc, d_desc.as<uint8_t>(), n_images, image_offsets, d_off.as<int32_t>(), k, L, seed, st, out, info);
  (void)hipStreamSynchronize(st);
  return rc;
}

int vo_vocab_train_dev(int n_desc, const uint8_t *dev_desc, int n_images, const int32_t *dev_image_offsets, int k, int L,
                       uint64_t seed, void *hip_stream, vo_vocab **out, vo_vocab_train_info *info) {
  const char *W = "vo_vocab_train_dev";
  VO_CHECK(check_args(W, n_desc, dev_desc, n_images, dev_image_offsets, k, L, out));
  VO_CHECK(vo::ensure_device());
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  std::vector<int32_t> off((size_t)n_images + 1);
  VO_CHECK(vo::copy_d2h(off.data(), dev_image_offsets, off.size() * 4, st, W));
  VO_CHECK(vo::stream_sync(st, W));
  VO_CHECK(check_offsets(W, n_desc, n_images, off.data()));
  const int rc = train_resident(n_desc, dev_desc, n_images, off.data(), dev_image_offsets, k, L, seed, st, out, info);
  (void)hipStreamSynchronize(st);  // the call's buffers are released on return
  return rc;
}

}  // extern "C"
