// new_points.hip -- LocalMapping::createNewMapPoints (src/localMapping.cpp:132-361) on the key-frame store (DESIGN.md
// section 4j): the state vo_kfstore_enable_mapping adds (poses, key-point positions, the id counter, the result record and
// the scratch of one neighbour step) and k_np_create, the last of a step's three launches: every match of the step's
// searchForTriangulation (match.hip: k_tri_walk, k_node_replay) through the parallax test, the three-way choice of the
// point, the depth, reprojection and scale gates (:197-341), then the commit of :344-355 in ascending idx1.
// Compiled with -ffp-contract=off (float gates that must round like the x86-64 reference build).
#include "kfstore.h"

#include "triangulate.h"

#include <algorithm>

namespace {

// every array of the block once: measure (block == nullptr) or assign
struct MapLayout {
  uint8_t *block;
  size_t at = 0;
  template <class T>
  void take(T *&field, size_t bytes) {
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += vo::up16(bytes);
  }
};

void map_layout(MapLayout &L, vo::KfMapView &M, int max_kf, int NK) {
  const size_t K = (size_t)max_kf, N = (size_t)NK;
  L.take(M.pose, K * vo::kNpPoseDoubles * 8);
  L.take(M.xy, K * N * 8);
  L.take(M.counter, 16);
  L.take(M.rec, (size_t)vo::kNpRecInts * 4);
  L.take(M.created, (size_t)vo::kKfGraphNb * N * 16);
  L.take(M.queries, N * 16);
  L.take(M.claims, N * 16);
  L.take(M.args, vo::tri_args_bytes());
  L.take(M.bok, N);
  L.take(M.match, N * 4);
  L.take(M.nm, 16);
  L.take(M.step, sizeof(vo::NpStep));
}

__global__ void k_np_counter(int *counter, int first) {
  if (threadIdx.x == 0) counter[0] = first;
}

__global__ void k_np_pose(double *pose, int *pose_set, const double *src) {
  if (threadIdx.x < 12) pose[threadIdx.x] = src[threadIdx.x];
  if (threadIdx.x == 12) *pose_set = 1;
}

__global__ __launch_bounds__(256) void k_np_split_xy(const float *xy, int n, float *x, float *y) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = xy[2 * i], y[i] = xy[2 * i + 1];
}

// Camera::pixel2camera(kpt, z) (camera.cpp:87-95): float arithmetic, widened
__device__ __forceinline__ void pixel2camera(const float *cam, float u, float v, float z, double pc[3]) {
  const float x = (u - cam[2]) * z / cam[0], y = (v - cam[3]) * z / cam[1];
  pc[0] = x, pc[1] = y, pc[2] = z;
}

// Camera::pixel2world(kpt, depth, Tcw) = Tcw^-1 * pixel2camera: R^T pc + Ow
__device__ __forceinline__ void back_project(const float *cam, float u, float v, float depth, const double *T, const double *Ow, double p[3]) {
  double pc[3];
  pixel2camera(cam, u, v, depth, pc);
  for (int i = 0; i < 3; i++) p[i] = (T[i] * pc[0] + T[3 + i] * pc[1] + T[6 + i] * pc[2]) + Ow[i];
}

struct NpFeature {
  float u, v, ur, depth;
  int octave;
};

// the gates behind the choice of the point (:262-341): z signs, reprojection (mono 5.991, stereo 7.815), distances, scale
// consistency.  dist1 = |p - Owc| as the float the reference holds
__device__ bool np_gates(const vo::NpStep &G, const float *cam, const float *sf, const NpFeature &f1, const NpFeature &f2, const double p[3],
                         float &dist1) {
  const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], bf = cam[4];
  const double *T1 = G.T1, *T2 = G.T2;
  const float z1 = (float)((T1[6] * p[0] + T1[7] * p[1] + T1[8] * p[2]) + T1[11]);
  if (z1 <= 0) return false;
  const float z2 = (float)((T2[6] * p[0] + T2[7] * p[1] + T2[8] * p[2]) + T2[11]);
  if (z2 <= 0) return false;
  const float s1 = sf[min(max(f1.octave, 0), 15)], s2 = sf[min(max(f2.octave, 0), 15)];
  {
    const float x1 = (float)((T1[0] * p[0] + T1[1] * p[1] + T1[2] * p[2]) + T1[9]);
    const float y1 = (float)((T1[3] * p[0] + T1[4] * p[1] + T1[5] * p[2]) + T1[10]);
    const float invz1 = 1.0f / z1, invSigma1 = 1.0f / s1;
    const float u1 = fx * x1 * invz1 + cx, v1 = fy * y1 * invz1 + cy;
    const float eu = u1 - f1.u, ev = v1 - f1.v;
    const float e1 = eu * eu + ev * ev;
    if (!(f1.ur >= 0)) {
      if (e1 * invSigma1 * invSigma1 > 5.991f) return false;
    } else {
      const float u1r = u1 - bf * invz1, er = u1r - f1.ur;
      const float e1r = e1 + er * er;
      if (e1r * invSigma1 * invSigma1 > 7.815f) return false;
    }
  }
  {
    const float x2 = (float)((T2[0] * p[0] + T2[1] * p[1] + T2[2] * p[2]) + T2[9]);
    const float y2 = (float)((T2[3] * p[0] + T2[4] * p[1] + T2[5] * p[2]) + T2[10]);
    const float invz2 = 1.0f / z2, invSigma2 = 1.0f / s2;
    const float u2 = fx * x2 * invz2 + cx, v2 = fy * y2 * invz2 + cy;
    const float eu = u2 - f2.u, ev = v2 - f2.v;
    const float e2 = eu * eu + ev * ev;
    if (!(f2.ur >= 0)) {
      if (e2 * invSigma2 * invSigma2 > 5.991f) return false;
    } else {
      const float u2r = u2 - bf * invz2, er = u2r - f2.ur;
      const float e2r = e2 + er * er;
      if (e2r * invSigma2 * invSigma2 > 7.815f) return false;
    }
  }
  const double a0 = p[0] - G.Ow1[0], a1 = p[1] - G.Ow1[1], a2 = p[2] - G.Ow1[2];
  const double b0 = p[0] - G.Ow2[0], b1 = p[1] - G.Ow2[1], b2 = p[2] - G.Ow2[2];
  dist1 = (float)sqrt(a0 * a0 + a1 * a1 + a2 * a2);
  const float dist2 = (float)sqrt(b0 * b0 + b1 * b1 + b2 * b2);
  if ((double)dist1 < 1e-6 || (double)dist2 < 1e-6) return false;
  const float distRatio = dist2 / dist1;  // NOTE: dist2/dist1  :336
  const float scaleRatio = s1 / s2, scaleFactor = 1.5f * sf[1];
  if (distRatio * scaleFactor < scaleRatio || distRatio > scaleRatio * scaleFactor) return false;
  return true;
}

// one match (:197-341) -> the point and dist1, or false
__device__ bool np_evaluate(const vo::NpStep &G, const float *T1f, const float *T2f, const float *cam, const float *sf, const NpFeature &f1,
                            const NpFeature &f2, double p[3], float &dist1) {
  const float b = cam[5];
  const bool stereo1 = f1.ur >= 0, stereo2 = f2.ur >= 0;
  double pc1[3], pc2[3], r1[3], r2[3];
  pixel2camera(cam, f1.u, f1.v, 1.0f, pc1);
  pixel2camera(cam, f2.u, f2.v, 1.0f, pc2);
  for (int i = 0; i < 3; i++) {
    r1[i] = G.T1[i] * pc1[0] + G.T1[3 + i] * pc1[1] + G.T1[6 + i] * pc1[2];
    r2[i] = G.T2[i] * pc2[0] + G.T2[3 + i] * pc2[1] + G.T2[6 + i] * pc2[2];
  }
  const double dot = r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2];
  const double n1 = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]), n2 = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
  const float cosRay = (float)(dot / (n1 * n2));
  float cd1 = 2.0f, cd2 = 2.0f;
  if (stereo1) cd1 = cosf((float)(2 * atan2(0.5 * (double)b, (double)f1.depth)));
  else if (stereo2) cd2 = cosf((float)(2 * atan2(0.5 * (double)b, (double)f2.depth)));  // QUIRK: only when !stereo1 (:222)
  const float cd = fminf(cd1, cd2);
  if (cosRay > 0 && cosRay < cd && (stereo1 || stereo2 || (double)cosRay < 0.9998)) {
    float o[3];
    if (!vo::triangulate_pair((float)pc1[0], (float)pc1[1], (float)pc2[0], (float)pc2[1], T1f, T2f, o)) return false;
    p[0] = o[0], p[1] = o[1], p[2] = o[2];
  } else if (stereo1 && cd1 < cd2) {
    back_project(cam, f1.u, f1.v, f1.depth, G.T1, G.Ow1, p);
  } else if (stereo2 && cd2 < cd1) {
    back_project(cam, f2.u, f2.v, f2.depth, G.T2, G.Ow2, p);
  } else {
    return false;
  }
  return np_gates(G, cam, sf, f1, f2, p, dist1);
}

struct CreateArgs {
  vo::KfStoreView S;
  vo::KfCullView X;
  vo::KfMapView M;
  double *normals;  // [max_kf][NK][3]
  int *ref_kf;      // [max_kf][NK] MapPoint::keyFrame_ref_ of a store with local BA, else NULL
  int current, step;
};

// One workgroup.  The step's matches are packed in ascending idx1, then a thread per match (256 at a time) evaluates it;
// the survivors are ranked in the same order by ballot + prefix counts (wave sums through LDS), which is the reference's
// creation order, and committed: one writer per byte and word, idx1 and idx2 each appear in at most one match.
__global__ __launch_bounds__(256) void k_np_create(CreateArgs A) {
  __shared__ int wsum[4];
  const vo::KfMapView &M = A.M;
  const vo::NpStep &G = *M.step;
  if (G.status != VO_KFSTORE_NP_SEARCHED) return;  // (uniform; the walk wrote the record's entry)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cur = A.current, kf = G.kf, NK = A.S.NK;
  const int nA = min(max(vo::kf_head(A.S, cur)[0], 0), NK), nB = min(max(vo::kf_head(A.S, kf)[0], 0), NK);
  const int id0 = *M.counter, row0 = M.rec[1];
  uint8_t *rc = const_cast<uint8_t *>(A.S.base) + (size_t)cur * A.S.rec, *rk = const_cast<uint8_t *>(A.S.base) + (size_t)kf * A.S.rec;
  float T1f[12], T2f[12];  // the cv::Mat_<float>(3, 4) of :154-157, :179-182
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T1f[4 * r + c] = (float)G.T1[3 * r + c], T2f[4 * r + c] = (float)G.T2[3 * r + c];
    T1f[4 * r + 3] = (float)G.T1[9 + r], T2f[4 * r + 3] = (float)G.T2[9 + r];
  }
  const float *xc = vo::np_x(M, cur), *yc = vo::np_y(M, cur), *xk = vo::np_x(M, kf), *yk = vo::np_y(M, kf);
  const uint8_t *dlow = cur < kf ? rc + A.S.o_desc : rk + A.S.o_desc;  // computeDescriptor with two holders: the lower-numbered one's
  // rank of the flagged threads in thread order and their number: ballot + prefix count, the wave sums through LDS
  auto block_rank = [&](bool flag, int &total) {
    const unsigned long long mk = __builtin_amdgcn_ballot_w64(flag);
    const int within = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
    if (lane == 0) wsum[wave] = (int)__popcll(mk);
    __syncthreads();
    int r = within;
    for (int w = 0; w < wave; w++) r += wsum[w];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return r;
  };
  // the matched features of `current` in ascending idx1, packed (the query list is free: the search is over), so that a
  // pass of 256 evaluations -- whose length is the slowest Jacobi of the pass -- is full
  int *list = reinterpret_cast<int *>(M.queries);
  int n_list = 0;
  for (int b0 = 0; b0 < nA; b0 += 256) {
    const int i1 = b0 + tid, i2 = i1 < nA ? M.match[i1] : -1;
    const bool has = i2 >= 0 && i2 < nB;
    int total;
    const int r = block_rank(has, total);
    if (has) list[n_list + r] = i1;
    n_list += total;
  }
  __syncthreads();
  int created = 0;
  for (int c0 = 0; c0 < n_list; c0 += 256) {
    const int i1 = c0 + tid < n_list ? list[c0 + tid] : -1;
    const int i2 = i1 >= 0 ? M.match[i1] : -1;
    bool ok = false;
    double p[3] = {0, 0, 0};
    float dist1 = 0;
    NpFeature f1{}, f2{};
    if (i2 >= 0) {
      f1 = NpFeature{xc[i1], yc[i1], vo::cull_uright(A.X, cur)[i1], vo::cull_depth(A.X, cur)[i1], vo::cull_octave(A.X, cur)[i1]};
      f2 = NpFeature{xk[i2], yk[i2], vo::cull_uright(A.X, kf)[i2], vo::cull_depth(A.X, kf)[i2], vo::cull_octave(A.X, kf)[i2]};
      ok = np_evaluate(G, T1f, T2f, M.cam, M.sf, f1, f2, p, dist1);
    }
    int total;
    const int rank = created + block_rank(ok, total);
    if (ok) {
      const int id = id0 + rank;
      // MapPoint::updateNormalAndDepth (mappoint.cpp:90-114): holders in ascending key-frame number, reference = current
      double na[3], nb[3], la = 0, lb = 0, nrm[3];
      const double *Oa = cur < kf ? G.Ow1 : G.Ow2, *Ob = cur < kf ? G.Ow2 : G.Ow1;
      for (int i = 0; i < 3; i++) na[i] = p[i] - Oa[i], nb[i] = p[i] - Ob[i], la += na[i] * na[i], lb += nb[i] * nb[i];
      la = sqrt(la), lb = sqrt(lb);
      for (int i = 0; i < 3; i++) nrm[i] = (na[i] / la + nb[i] / lb) / 2;
      const float maxd = dist1 * M.sf[min(max(f1.octave, 0), 15)], mind = maxd / M.sf[min(max(M.n_levels - 1, 0), 15)];
      const uint4 d0 = reinterpret_cast<const uint4 *>(dlow)[2 * (cur < kf ? i1 : i2)];
      const uint4 d1 = reinterpret_cast<const uint4 *>(dlow)[2 * (cur < kf ? i1 : i2) + 1];
      for (int side = 0; side < 2; side++) {
        uint8_t *r = side ? rk : rc;
        const int i = side ? i2 : i1, k = side ? kf : cur;
        (r + A.S.o_flags)[i] = 3;  // bit 0: the point exists and is not bad; bit 1: observe_cnt_ > 0
        reinterpret_cast<int *>(r + A.S.o_ids)[i] = id;
        double *pt = reinterpret_cast<double *>(r + A.S.o_points) + 3 * (size_t)i;
        pt[0] = p[0], pt[1] = p[1], pt[2] = p[2];
        reinterpret_cast<uint4 *>(r + A.S.o_pdesc)[2 * i] = d0, reinterpret_cast<uint4 *>(r + A.S.o_pdesc)[2 * i + 1] = d1;
        reinterpret_cast<float *>(r + A.S.o_mind)[i] = mind, reinterpret_cast<float *>(r + A.S.o_maxd)[i] = maxd;
        double *n = A.normals + ((size_t)k * NK + i) * 3;
        n[0] = nrm[0], n[1] = nrm[1], n[2] = nrm[2];
        if (A.ref_kf) A.ref_kf[(size_t)k * NK + i] = cur;  // keyFrame_ref_(keyframe) (mappoint.cpp:37)
      }
      M.created[row0 + rank] = make_int4(kf, i1, i2, id);
    }
    created += total;
  }
  __syncthreads();
  if (tid == 0) {
    *M.counter = id0 + created, M.rec[1] = row0 + created;
    M.rec[4 + 4 * A.step + 2] = *M.nm, M.rec[4 + 4 * A.step + 3] = created;
  }
}

}  // namespace

namespace {

using namespace vo;

size_t mapping_bytes(int max_kf, int NK) {
  MapLayout L{nullptr};
  KfMapView M{};
  map_layout(L, M, max_kf, NK);
  return L.at;
}

KfMapView mapping_layout(void *block, int max_kf, int NK) {
  MapLayout L{reinterpret_cast<uint8_t *>(block)};
  KfMapView M{};
  map_layout(L, M, max_kf, NK);
  M.NK = NK;
  return M;
}

int mapping_init(const KfMapView &M, size_t bytes, int first_point_id, hipStream_t st) {
  VO_HIP_CHECK(hipMemsetAsync(M.pose, 0, bytes, st));  // (pose is the block's first array: poses and pose-set words zero)
  hipLaunchKernelGGL(k_np_counter, dim3(1), dim3(64), 0, st, M.counter, first_point_id);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int mapping_set_pose_dev(const KfMapView &M, int k, const double *dev_Tcw12, hipStream_t st) {
  hipLaunchKernelGGL(k_np_pose, dim3(1), dim3(64), 0, st, np_pose(M, k), np_pose_set(M, k), dev_Tcw12);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int mapping_split_xy(const KfMapView &M, int k, int n, const float *dev_xy, hipStream_t st) {
  if (n <= 0) return VO_OK;
  hipLaunchKernelGGL(k_np_split_xy, dim3((n + 255) / 256), dim3(256), 0, st, dev_xy, n, np_x(M, k), np_y(M, k));
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// (ref_kf: the column of a store with local BA, else NULL -- a created point's keyFrame_ref_ is `current`, mappoint.cpp:37)
int np_create(const KfStoreView &S, const KfCullView &X, const KfMapView &M, double *normals, int *ref_kf, int current, int step,
              hipStream_t st) {
  CreateArgs A{S, X, M, normals, ref_kf, current, step};
  hipLaunchKernelGGL(k_np_create, dim3(1), dim3(256), 0, st, A);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_kfstore_enable_mapping(vo_kfstore *s, const float cam[6], int n_levels, const float *scale_factors, int32_t first_point_id) {
  const char *W = "vo_kfstore_enable_mapping";
  const bool args_ok = cam && scale_factors && n_levels >= 1 && n_levels <= 16 && first_point_id >= 0;
  if (const int rc = enable_begin(s, W, kLayerCulling, kLayerMapping, args_ok)) return rc < 0 ? rc : VO_OK;
  if (s->NK > 16384) {
    set_error("%s: %d features per key-frame, the search kernel handles 16384", W, s->NK);
    return VO_ERR_CAPACITY;
  }
  s->map_bytes = mapping_bytes(s->max_kf, s->NK);
  VO_CHECK(s->map.reserve(s->map_bytes));
  s->M = mapping_layout(s->map.p, s->max_kf, s->NK);
  s->M.n_levels = n_levels;
  for (int i = 0; i < 6; i++) s->M.cam[i] = cam[i];
  for (int i = 0; i < 16; i++) s->M.sf[i] = scale_factors[i < n_levels ? i : n_levels - 1];
  VO_CHECK(mapping_init(s->M, s->map_bytes, first_point_id, s->st));
  VO_CHECK(stream_sync(s->st, W));
  s->layers |= kLayerMapping;
  return VO_OK;
}

int vo_kfstore_set_pose(vo_kfstore *s, int keyframe, const double *Tcw12) {
  const char *W = "vo_kfstore_set_pose";
  VO_CHECK(need(s, W, kLayerMapping));
  VO_CHECK(need_keyframe(s, W, keyframe));
  if (!Tcw12) return VO_ERR_INVALID;
  s->gen++;
  // the pose-set word lies behind the pose (the thirteenth slot): one copy
  double *h = reinterpret_cast<double *>(s->stage.data());
  memcpy(h, Tcw12, 96);
  const int32_t one[2] = {1, 0};
  memcpy(h + 12, one, 8);
  VO_CHECK(copy_h2d(np_pose(s->M, keyframe), h, kNpPoseDoubles * 8, s->st, W));
  return stream_sync(s->st, W);
}

int vo_kfstore_set_pose_dev(vo_kfstore *s, int keyframe, const double *dev_Tcw12) {
  const char *W = "vo_kfstore_set_pose_dev";
  VO_CHECK(need(s, W, kLayerMapping));
  VO_CHECK(need_keyframe(s, W, keyframe));
  if (!dev_Tcw12) return VO_ERR_INVALID;
  s->gen++;
  return mapping_set_pose_dev(s->M, keyframe, dev_Tcw12, s->st);
}

int vo_kfstore_set_keypoint_xy(vo_kfstore *s, int keyframe, const float *xy) {
  const char *W = "vo_kfstore_set_keypoint_xy";
  VO_CHECK(need(s, W, kLayerMapping));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe], NK = (size_t)s->NK;
  if (n == 0) return VO_OK;
  if (!xy) return VO_ERR_INVALID;
  s->gen++;
  // the two columns of a key-frame lie side by side: staged whole (zero beyond n), one copy
  float *hx = reinterpret_cast<float *>(s->stage.data()), *hy = hx + NK;  // (a record is longer than 8 bytes a feature)
  for (size_t i = 0; i < NK; i++) hx[i] = i < n ? xy[2 * i] : 0.f, hy[i] = i < n ? xy[2 * i + 1] : 0.f;
  VO_CHECK(copy_h2d(np_x(s->M, keyframe), hx, NK * 8, s->st, W));
  return stream_sync(s->st, W);
}

int vo_kfstore_set_keypoint_xy_dev(vo_kfstore *s, int keyframe, const float *dev_xy) {
  const char *W = "vo_kfstore_set_keypoint_xy_dev";
  VO_CHECK(need(s, W, kLayerMapping));
  VO_CHECK(need_keyframe(s, W, keyframe));
  const int n = s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  if (!dev_xy) return VO_ERR_INVALID;
  s->gen++;
  return mapping_split_xy(s->M, keyframe, n, dev_xy, s->st);
}

int vo_kfstore_next_point_id(vo_kfstore *s, int32_t *id) {
  const char *W = "vo_kfstore_next_point_id";
  VO_CHECK(need(s, W, kLayerMapping));
  if (!id) return VO_ERR_INVALID;
  VO_CHECK(copy_d2h(id, s->M.counter, 4, s->st, W));
  return stream_sync(s->st, W);
}

int vo_kfstore_create_map_points(vo_kfstore *s, int current, int max_neighbors) {
  const char *W = "vo_kfstore_create_map_points";
  VO_CHECK(need(s, W, kLayerMapping));
  VO_CHECK(need_keyframe(s, W, current));
  if (max_neighbors < 1 || max_neighbors > kKfGraphNb) {
    set_error("%s: max_neighbors %d outside [1, %d]", W, max_neighbors, kKfGraphNb);
    return VO_ERR_INVALID;
  }
  // (that `current` has been erased or has no pose only the device knows: k_tri_walk then reaches no neighbour and raises
  //  the sticky VO_KFSTORE_CONNECTIONS_INVALID)
  const KfStoreView V = kfstore_view(s);
  const KfConnView C = connections_view(s->conn);
  for (int i = 0; i < max_neighbors; i++) {  // step i + 1 reads the flags step i wrote: walk, replay, create per neighbour
    VO_CHECK(tri_walk_replay(V, s->X, s->M, s->graph.as<int>(), C.status, current, i, s->st));
    VO_CHECK(np_create(V, s->X, s->M, s->normals.as<double>(), (s->layers & kLayerLocalBa) ? s->B.ref_kf : nullptr, current, i, s->st));
  }
  s->obs_dirty = true, s->gen++;  // (whether anything was created only the device knows)
  if (s->layers & kLayerUpkeep) VO_CHECK(upkeep_created_enqueue(s->M, s->U, C.status, current, s->st));  // addedMapPoints_.push_back (:355)
  return VO_OK;
}

int vo_kfstore_new_points_result(vo_kfstore *s, int32_t *n_neighbors, int32_t *neighbor_kf, int32_t *status, int32_t *n_matches,
                                 int32_t *n_created, int32_t *created, int created_capacity) {
  const char *W = "vo_kfstore_new_points_result";
  VO_CHECK(need(s, W, kLayerMapping));
  if (!n_neighbors || created_capacity < 0 || (created_capacity > 0 && !created)) return VO_ERR_INVALID;
  int32_t rec[kNpRecInts] = {0};
  VO_CHECK(copy_d2h(rec, s->M.rec, sizeof(rec), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  const int n = std::min(std::max(rec[0], 0), kKfGraphNb);
  const int total = std::min(std::max(rec[1], 0), kKfGraphNb * s->NK);
  *n_neighbors = n;
  for (int i = 0; i < kKfGraphNb; i++) {
    if (neighbor_kf) neighbor_kf[i] = i < n ? rec[4 + 4 * i] : -1;
    if (status) status[i] = i < n ? rec[4 + 4 * i + 1] : VO_KFSTORE_NP_NOT_REACHED;
    if (n_matches) n_matches[i] = i < n ? rec[4 + 4 * i + 2] : 0;
    if (n_created) n_created[i] = i < n ? rec[4 + 4 * i + 3] : 0;
  }
  const int rows = std::min(total, created_capacity);
  if (rows > 0) {
    VO_CHECK(copy_d2h(created, s->M.created, (size_t)rows * 16, s->st, W));
    VO_CHECK(stream_sync(s->st, W));
  }
  if (total > created_capacity) {
    set_error("%s: the call created %d points, created_capacity is %d", W, total, created_capacity);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

int vo_kfstore_get_points(vo_kfstore *s, int keyframe, uint8_t *flags, int32_t *ids, double *points, uint8_t *point_desc,
                          float *min_distance, float *max_distance, double *normals) {
  const char *W = "vo_kfstore_get_points";
  if (!s) return VO_ERR_INVALID;
  VO_CHECK(need_keyframe(s, W, keyframe));
  const size_t n = (size_t)s->n[(size_t)keyframe];
  if (n == 0) return VO_OK;
  const KfStoreView &V = s->V;
  const uint8_t *r = s->record(keyframe);
  if (flags) VO_CHECK(copy_d2h(flags, r + V.o_flags, n, s->st, W));
  if (ids) VO_CHECK(copy_d2h(ids, r + V.o_ids, n * 4, s->st, W));
  if (points) VO_CHECK(copy_d2h(points, r + V.o_points, n * 24, s->st, W));
  if (point_desc) VO_CHECK(copy_d2h(point_desc, r + V.o_pdesc, n * 32, s->st, W));
  if (min_distance) VO_CHECK(copy_d2h(min_distance, r + V.o_mind, n * 4, s->st, W));
  if (max_distance) VO_CHECK(copy_d2h(max_distance, r + V.o_maxd, n * 4, s->st, W));
  if (normals) VO_CHECK(copy_d2h(normals, s->normals.as<double>() + (size_t)keyframe * s->NK * 3, n * 24, s->st, W));
  return stream_sync(s->st, W);
}

int vo_kfstore_get_pose(vo_kfstore *s, int keyframe, double *Tcw12, int32_t *pose_set) {
  const char *W = "vo_kfstore_get_pose";
  VO_CHECK(need(s, W, kLayerMapping));
  VO_CHECK(need_keyframe(s, W, keyframe));
  double h[kNpPoseDoubles];
  VO_CHECK(copy_d2h(h, np_pose(s->M, keyframe), sizeof(h), s->st, W));
  VO_CHECK(stream_sync(s->st, W));
  if (Tcw12) memcpy(Tcw12, h, 96);
  if (pose_set) memcpy(pose_set, h + 12, 4);
  return VO_OK;
}

}  // extern "C"
