// block_sort.h -- a workgroup-wide sort of 64-bit keys (k_featvec in match.hip, k_reloc_local_ids in reloc.hip) and the
// workgroup-wide prefix count of the depth walks (keyframe_create.hip, handover.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace vo {

// Ascending bitonic sort of keys[0 .. np2) by every thread of the workgroup; np2 is a power of two (pad with ~0ull).
// keys may live in LDS or in device memory that only this workgroup touches.  log2(np2) * (log2(np2) + 1) / 2 steps of
// np2 / 2 compare-exchanges, a barrier between steps.  The network is fixed: the result is a function of the keys alone,
// and with distinct keys it is THE sorted order -- no dependence on which thread runs when.
__device__ __forceinline__ void block_bitonic_sort(unsigned long long *keys, int np2) {
  const int nt = (int)blockDim.x, half = np2 >> 1;
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = (int)threadIdx.x; t < half; t += nt) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;  // i: bit j clear
        const unsigned long long a = keys[i], b = keys[l];
        if ((a > b) == ((i & k) == 0)) keys[i] = b, keys[l] = a;
      }
    }
  __syncthreads();
}

// exclusive prefix of `flag` over the workgroup in thread order; *total = the workgroup's sum.  s_w: one int per
// wavefront.  Two barriers.  (the depth walks of keyframe_create.hip and handover.hip)
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

__host__ __device__ __forceinline__ int pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace vo
