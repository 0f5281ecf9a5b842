// wave_ops.h -- wavefront / workgroup reductions and the inter-workgroup hand-off of the FP64 solver kernels
// (ba.hip, pose_only.hip, sim3.hip, chol.hip).  Header-only: every helper is __device__ __forceinline__.
#pragma once
#include <hip/hip_runtime.h>

namespace vo {

// ============================================================================================
// block reductions (fixed order => deterministic)
// ============================================================================================
// 64-lane sum, same value in every lane.  The four in-row steps are DPP moves of the two 32-bit halves (no LDS
// crossbar, a fraction of a ds_bpermute's latency); the cross-row steps use v_readlane of the row sums.  Fixed order.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror: every lane holds its row's sum
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
#ifdef VO_BA_STAMPS
// time stamp that cannot move above the computation of `dep`
__device__ __forceinline__ unsigned long long stamp_after(double &dep) {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t), "+v"(dep)::"memory");
  return t;
}
#endif
template <int N, int NW = 0>  // NW: wavefronts per block when known at compile time (0: blockDim.x / 64)
__device__ __forceinline__ void block_sum(double (&v)[N], double *lds /*>= nw*N*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; i++) v[i] = wave_sum(v[i]);
  const int nw = NW ? NW : (int)(blockDim.x >> 6);
  if (nw == 1) return;  // one wavefront: the wave sum is the block sum (no LDS, no barrier)
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) lds[wave * N + i] = v[i];
  }
  __syncthreads();
  // all partials are read in one batch and summed in wave order (a runtime loop over the waves waits for LDS once
  // per term: 4 us for 27 sums)
  if (NW == 8 || (NW == 0 && nw == 8)) {
    double p[8][N];
#pragma unroll
    for (int w = 0; w < 8; w++)
#pragma unroll
      for (int i = 0; i < N; i++) p[w][i] = lds[w * N + i];
#pragma unroll
    for (int i = 0; i < N; i++)
      v[i] = (((((((0.0 + p[0][i]) + p[1][i]) + p[2][i]) + p[3][i]) + p[4][i]) + p[5][i]) + p[6][i]) + p[7][i];
    return;
  }
  if (NW == 2 || (NW == 0 && nw == 2)) {
    double p[2][N];
#pragma unroll
    for (int w = 0; w < 2; w++)
#pragma unroll
      for (int i = 0; i < N; i++) p[w][i] = lds[w * N + i];
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = (0.0 + p[0][i]) + p[1][i];
    return;
  }
  if (NW == 4 || (NW == 0 && nw == 4)) {
    double p[4][N];
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int i = 0; i < N; i++) p[w][i] = lds[w * N + i];
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = (((0.0 + p[0][i]) + p[1][i]) + p[2][i]) + p[3][i];
    return;
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    double s = 0;
    for (int w = 0; w < nw; w++) s += lds[w * N + i];
    v[i] = s;
  }
}

// Inter-workgroup hand-off ("last block reduces") without fences, MI355X guide Guideline 16 form
// R1: EVERY handed-off byte is stored write-through (agent-scope relaxed atomic store = `sc1`) and
// loaded with an agent-scope relaxed atomic load (`sc1`, bypasses this CU's L1); every storing wave
// drains its stores (s_waitcnt vmcnt(0)), the block barriers, one lane takes a ticket with a relaxed
// agent-scope add.  The block that draws the last ticket reads the others' data.  Placement
// independent: per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs.
__device__ __forceinline__ void st_sc1(double *p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), __double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1(const double *p) {
  return __longlong_as_double(__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ bool arrive_and_check_last(unsigned int *counter, unsigned int expected, int *s_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (t == expected - 1u);
    if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    *s_flag = last;
  }
  __syncthreads();
  return *s_flag != 0;
}

}  // namespace vo
