// loop.hip -- small batched kernels around the loop-closing and local-mapping callers of the hot path:
//   k_sim3_ransac   Sim3Solver::iterate's hypotheses (reference src/sim3Solver.cpp:98-280): Horn's closed form per
//                   sample triplet + checkInliers over all correspondences, one workgroup per hypothesis
//   k_triangulate   the 4 x 4 linear triangulation of LocalMapping::createNewMapPoints (src/localMapping.cpp:234-251)
//   k_bow_score     Map::score, the L1 similarity of two BoW vectors (src/map.cpp:335-376), one candidate per thread
//   k_rgb2gray      cv::cvtColor(CV_RGB2GRAY / CV_BGR2GRAY) of VisualOdometry::createFrame (src/visualOdometry.cpp:146-159)
// Compiled with -ffp-contract=off (float gates that must round like the x86-64 reference build).
#include "vo_common.h"

#include "sim3_horn.h"
#include "triangulate.h"

#include <vector>

namespace {

using vo::sim3_horn;  // (sim3_horn.h: shared with loop_sim3.hip)
using vo::sim3_inlier;
using vo::sim3_with_inverse;

__global__ __launch_bounds__(256) void k_sim3_ransac(int n, const double *pc1, const double *pc2, const double *px1,
                                                     const double *px2, const int *me1, const int *me2, float fx, float fy,
                                                     float cx, float cy, const int *triplets, int fix_scale, int *counts,
                                                     uint8_t *flags, double *sims) {
  __shared__ double T[26];  // R (9) t (3) s | Ri (9) ti (3) si
  __shared__ int s_cnt;
  const int k = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    double P1[9], P2[9], R[9], t[3], s;
    for (int i = 0; i < 3; i++) {
      const int idx = triplets[3 * k + i];
      for (int a = 0; a < 3; a++) P1[3 * i + a] = pc1[3 * idx + a], P2[3 * i + a] = pc2[3 * idx + a];
    }
    sim3_horn(P1, P2, fix_scale, R, t, s);
    sim3_with_inverse(R, t, s, T);
    for (int a = 0; a < 13; a++) sims[13LL * k + a] = T[a];
    s_cnt = 0;
  }
  __syncthreads();
  int local = 0;
  for (int i = tid; i < n; i += 256) {
    const bool in = sim3_inlier(T, pc1 + 3 * i, pc2 + 3 * i, px1 + 2 * i, px2 + 2 * i, me1[i], me2[i], fx, fy, cx, cy);  // :268
    flags[(long long)k * n + i] = in ? 1 : 0;
    local += in;
  }
  if (local) atomicAdd(&s_cnt, local);
  __syncthreads();
  if (tid == 0) counts[k] = s_cnt;
}

__global__ __launch_bounds__(256) void k_triangulate(int n, const float *xn1, const float *xn2, const float *T1, const float *T2,
                                                     long long t2_stride, float *out, uint8_t *ok) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float p[3];
  ok[i] = vo::triangulate_pair(xn1[2 * i], xn1[2 * i + 1], xn2[2 * i], xn2[2 * i + 1], T1, T2 + (long long)i * t2_stride, p);
  for (int a = 0; a < 3; a++) out[3 * i + a] = p[a];
}

// Map::score (map.cpp:335-376): L1 score of the query BoW vector against candidate c's (both ascending word ids)
__global__ __launch_bounds__(256) void k_bow_score(int nq, const int *qw, const double *qv, int n_cand, const int *start,
                                                   const int *cw, const double *cv, double *score) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cand) return;
  int i = 0, j = start[c];
  const int je = start[c + 1];
  double s = 0;
  while (i < nq && j < je) {
    const int a = qw[i], b = cw[j];
    if (a == b) {
      s += fabs(qv[i] - cv[j]) - fabs(qv[i]) - fabs(cv[j]);
      i++, j++;
    } else if (a < b) {
      i++;  // (lower_bound jumps of the reference visit the same matches)
    } else {
      j++;
    }
  }
  score[c] = -s / 2.0;
}

__global__ __launch_bounds__(256) void k_rgb2gray(const uint8_t *src, long long n_px, int channels, int first_is_red, uint8_t *dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  const int c0 = src[i * channels], c1 = src[i * channels + 1], c2 = src[i * channels + 2];
  const int r = first_is_red ? c0 : c2, b = first_is_red ? c2 : c0;
  dst[i] = (uint8_t)((r * 4899 + c1 * 9617 + b * 1868 + (1 << 13)) >> 14);
}

}  // namespace

extern "C" {

int vo_sim3_ransac_eval(int n, const double *cam1_points, const double *cam2_points, const double *pixels1,
                        const double *pixels2, const int32_t *max_err1, const int32_t *max_err2, const float cam4[4],
                        int n_hypotheses, const int32_t *triplets, int fix_scale, int32_t *counts, uint8_t *inlier_flags,
                        double *sims) {
  // all six correspondence arrays NULL: the correspondences this host thread uploaded with its previous call stay in place
  // (Sim3Solver::iterate evaluates one hypothesis per trip to keep rand() in step with the reference: five trips per call
  // of the loop closer, one upload -- ADVICE r4)
  const bool resident = !cam1_points && !cam2_points && !pixels1 && !pixels2 && !max_err1 && !max_err2;
  if (n < 0 || n_hypotheses < 0 || !cam4 || (n_hypotheses > 0 && (!triplets || !counts || !sims)) ||
      (n > 0 && !resident && (!cam1_points || !cam2_points || !pixels1 || !pixels2 || !max_err1 || !max_err2)))
    return VO_ERR_INVALID;
  if (n_hypotheses == 0) return VO_OK;
  for (int k = 0; k < 3 * n_hypotheses; k++)
    if (triplets[k] < 0 || triplets[k] >= n) {
      vo::set_error("vo_sim3_ransac_eval: sample index %d out of range", triplets[k]);
      return VO_ERR_INVALID;
    }
  VO_CHECK(vo::ensure_device());
  thread_local vo::ScratchBuf d1, d2, p1, p2, e1, e2, tr, cn, fl, sm;
  thread_local int resident_n = -1;
  hipStream_t st = vo::thread_stream();
  const char *W = "vo_sim3_ransac_eval";
  if (resident && n > 0) {
    // (the buffers themselves are checked, not only the count: vo_release_thread_scratch() on this thread frees them, and a
    //  failed upload leaves them short -- a launch with null or short pointers is a GPU memory fault, not an error code)
    const bool held = d1.p && d2.p && p1.p && p2.p && e1.p && e2.p && d1.bytes >= (size_t)n * 24 && d2.bytes >= (size_t)n * 24 &&
                      p1.bytes >= (size_t)n * 16 && p2.bytes >= (size_t)n * 16 && e1.bytes >= (size_t)n * 4 && e2.bytes >= (size_t)n * 4;
    if (resident_n != n || !held) {
      vo::set_error("vo_sim3_ransac_eval: no correspondences of this size are resident for this thread (%d requested, %d held%s)", n,
                    resident_n, held ? "" : ", buffers released");
      resident_n = -1;
      return VO_ERR_INVALID;
    }
  } else {
    resident_n = -1;
    VO_CHECK(vo::upload(d1, cam1_points, (size_t)n * 24, st, W));
    VO_CHECK(vo::upload(d2, cam2_points, (size_t)n * 24, st, W));
    VO_CHECK(vo::upload(p1, pixels1, (size_t)n * 16, st, W));
    VO_CHECK(vo::upload(p2, pixels2, (size_t)n * 16, st, W));
    VO_CHECK(vo::upload(e1, max_err1, (size_t)n * 4, st, W));
    VO_CHECK(vo::upload(e2, max_err2, (size_t)n * 4, st, W));
    resident_n = n;
  }
  VO_CHECK(vo::upload(tr, triplets, (size_t)n_hypotheses * 12, st, W));
  VO_CHECK(cn.reserve((size_t)n_hypotheses * 4));
  VO_CHECK(fl.reserve(std::max<size_t>((size_t)n_hypotheses * n, 64)));
  VO_CHECK(sm.reserve((size_t)n_hypotheses * 13 * 8));
  hipLaunchKernelGGL(k_sim3_ransac, dim3(n_hypotheses), dim3(256), 0, st, n, d1.as<double>(), d2.as<double>(), p1.as<double>(),
                     p2.as<double>(), e1.as<int>(), e2.as<int>(), cam4[0], cam4[1], cam4[2], cam4[3], tr.as<int>(), fix_scale,
                     cn.as<int>(), fl.as<uint8_t>(), sm.as<double>());
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(vo::copy_d2h(counts, cn.p, (size_t)n_hypotheses * 4, st, W));
  if (inlier_flags && n > 0) VO_CHECK(vo::copy_d2h(inlier_flags, fl.p, (size_t)n_hypotheses * n, st, W));
  VO_CHECK(vo::copy_d2h(sims, sm.p, (size_t)n_hypotheses * 13 * 8, st, W));
  return vo::stream_sync(st, W);
}

int vo_triangulate(int n, const float *xn1, const float *xn2, const float Tcw1[12], const float *Tcw2, int per_pair_pose2,
                   float *points, uint8_t *ok) {
  if (n < 0 || (n > 0 && (!xn1 || !xn2 || !Tcw1 || !Tcw2 || !points || !ok))) return VO_ERR_INVALID;
  if (n == 0) return VO_OK;
  VO_CHECK(vo::ensure_device());
  thread_local vo::ScratchBuf a, b, t1, t2, o, k;
  hipStream_t st = vo::thread_stream();
  const char *W = "vo_triangulate";
  VO_CHECK(vo::upload(a, xn1, (size_t)n * 8, st, W));
  VO_CHECK(vo::upload(b, xn2, (size_t)n * 8, st, W));
  VO_CHECK(vo::upload(t1, Tcw1, 48, st, W));
  VO_CHECK(vo::upload(t2, Tcw2, per_pair_pose2 ? (size_t)n * 48 : 48, st, W));
  VO_CHECK(o.reserve((size_t)n * 12));
  VO_CHECK(k.reserve((size_t)n + 64));
  hipLaunchKernelGGL(k_triangulate, dim3((n + 255) / 256), dim3(256), 0, st, n, a.as<float>(), b.as<float>(), t1.as<float>(),
                     t2.as<float>(), per_pair_pose2 ? 12LL : 0LL, o.as<float>(), k.as<uint8_t>());
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(vo::copy_d2h(points, o.p, (size_t)n * 12, st, W));
  VO_CHECK(vo::copy_d2h(ok, k.p, (size_t)n, st, W));
  return vo::stream_sync(st, W);
}

int vo_bow_score(int n_query, const int32_t *query_words, const double *query_values, int n_candidates,
                 const int32_t *cand_start, const int32_t *cand_words, const double *cand_values, double *scores) {
  if (n_query < 0 || n_candidates < 0 || (n_candidates > 0 && (!cand_start || !scores)) ||
      (n_query > 0 && (!query_words || !query_values)))
    return VO_ERR_INVALID;
  if (n_candidates == 0) return VO_OK;
  const int total = cand_start[n_candidates];
  if (total < 0 || (total > 0 && (!cand_words || !cand_values))) return VO_ERR_INVALID;
  VO_CHECK(vo::ensure_device());
  thread_local vo::ScratchBuf qw, qv, cs, cw, cv, sc;
  hipStream_t st = vo::thread_stream();
  const char *W = "vo_bow_score";
  VO_CHECK(vo::upload(qw, query_words, (size_t)n_query * 4, st, W));
  VO_CHECK(vo::upload(qv, query_values, (size_t)n_query * 8, st, W));
  VO_CHECK(vo::upload(cs, cand_start, (size_t)(n_candidates + 1) * 4, st, W));
  VO_CHECK(vo::upload(cw, cand_words, (size_t)total * 4, st, W));
  VO_CHECK(vo::upload(cv, cand_values, (size_t)total * 8, st, W));
  VO_CHECK(sc.reserve((size_t)n_candidates * 8));
  hipLaunchKernelGGL(k_bow_score, dim3((n_candidates + 255) / 256), dim3(256), 0, st, n_query, qw.as<int>(), qv.as<double>(),
                     n_candidates, cs.as<int>(), cw.as<int>(), cv.as<double>(), sc.as<double>());
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(vo::copy_d2h(scores, sc.p, (size_t)n_candidates * 8, st, W));
  return vo::stream_sync(st, W);
}

int vo_rgb_to_gray_dev(const uint8_t *dev_src, long long n_pixels, int channels, int first_is_red, uint8_t *dev_dst,
                       void *hip_stream) {
  if (!dev_src || !dev_dst || n_pixels < 0 || (channels != 3 && channels != 4)) return VO_ERR_INVALID;
  if (n_pixels == 0) return VO_OK;
  VO_CHECK(vo::ensure_device());
  hipLaunchKernelGGL(k_rgb2gray, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, dev_src, n_pixels,
                     channels, first_is_red, dev_dst);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_rgb_to_gray(const uint8_t *src, long long n_pixels, int channels, int first_is_red, uint8_t *dst) {
  if (!src || !dst || n_pixels < 0 || (channels != 3 && channels != 4)) return VO_ERR_INVALID;
  if (n_pixels == 0) return VO_OK;
  VO_CHECK(vo::ensure_device());
  thread_local vo::ScratchBuf a, b;
  hipStream_t st = vo::thread_stream();
  VO_CHECK(vo::upload(a, src, (size_t)n_pixels * channels, st, "vo_rgb_to_gray"));
  VO_CHECK(b.reserve((size_t)n_pixels));
  VO_CHECK(vo_rgb_to_gray_dev(a.as<uint8_t>(), n_pixels, channels, first_is_red, b.as<uint8_t>(), st));
  VO_CHECK(vo::copy_d2h(dst, b.p, (size_t)n_pixels, st, "vo_rgb_to_gray"));
  return vo::stream_sync(st, "vo_rgb_to_gray");
}

}  // extern "C"
