// kf_area.h -- KeyFrame::getFeaturesInArea (keyframe.cpp:268-309) over a key-frame of the store, whose grid is never built:
// the floor-computed cell range of a window, the ROUNDED cell of a feature (frame.cpp:83-86), the radius test, and the key
// that orders the window's features as the reference visits them (cell column, cell row, feature).  Shared by the fusion
// search (fuse.hip: k_fuse_search) and the loop searches (loop_sim3.hip), so that both read a window the same way.
// Include from translation units compiled with -ffp-contract=off only.
#pragma once
#include "vo_common.h"

namespace vo {

constexpr int kAreaCols = 64, kAreaRows = 48;

struct AreaWindow {
  int x0, x1, y0, y1;
  bool any;  // false: the reference returns an empty list before it visits a cell
};

__device__ __forceinline__ AreaWindow area_window(const KfFuseView &F, float u, float v, float radius) {
  AreaWindow W;
  W.x0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, F.xmin), radius), F.gpw)));
  W.x1 = min(kAreaCols - 1, (int)floorf(__fmul_rn(__fadd_rn(__fsub_rn(u, F.xmin), radius), F.gpw)));
  W.y0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, F.ymin), radius), F.gph)));
  W.y1 = min(kAreaRows - 1, (int)floorf(__fmul_rn(__fadd_rn(__fsub_rn(v, F.ymin), radius), F.gph)));
  W.any = !(W.x0 >= kAreaCols || W.x1 < 0 || W.y0 >= kAreaRows || W.y1 < 0);
  return W;
}

// is the feature at (x, y) in the list getFeaturesInArea(u, v, radius) returns?  (gx, gy): its cell
__device__ __forceinline__ bool area_holds(const KfFuseView &F, const AreaWindow &W, float x, float y, float u, float v, float radius,
                                           int &gx, int &gy) {
  // the feature's own cell is ROUNDED (frame.cpp:83-86); outside the grid it is in no cell
  gx = (int)roundf(__fmul_rn(__fsub_rn(x, F.xmin), F.gpw)), gy = (int)roundf(__fmul_rn(__fsub_rn(y, F.ymin), F.gph));
  if (gx < 0 || gx >= kAreaCols || gy < 0 || gy >= kAreaRows || gx < W.x0 || gx > W.x1 || gy < W.y0 || gy > W.y1) return false;
  return fabsf(__fsub_rn(x, u)) < radius && fabsf(__fsub_rn(y, v)) < radius;
}

// the place of a feature in the visiting order: cell column, cell row, feature
__device__ __forceinline__ unsigned long long area_order(int gx, int gy, int f) {
  return ((unsigned long long)gx << 38) | ((unsigned long long)gy << 32) | (unsigned)f;
}
// the strictly smallest distance in the visiting order is the smallest key
__device__ __forceinline__ unsigned long long area_key(int d, int gx, int gy, int f) { return ((unsigned long long)d << 44) | area_order(gx, gy, f); }

__device__ __forceinline__ int hamming256(const uint4 &qa, const uint4 &qb, const uint4 &da, const uint4 &db) {
  return __popc(qa.x ^ da.x) + __popc(qa.y ^ da.y) + __popc(qa.z ^ da.z) + __popc(qa.w ^ da.w) + __popc(qb.x ^ db.x) + __popc(qb.y ^ db.y) +
         __popc(qb.z ^ db.z) + __popc(qb.w ^ db.w);
}

// MapPoint::predictScale (mappoint.cpp:198-212), as reloc.hip and fuse.hip do it; log_sf1 = (float)log((double)sf[1])
__device__ __forceinline__ int predict_level(float maxd, float dist, float log_sf1, int n_levels) {
  const float ratio = __fdiv_rn(maxd, dist);
  const float lg = (float)log((double)ratio);
  const int sc = (int)ceilf(__fdiv_rn(lg, log_sf1));
  return sc < 0 ? 0 : (sc >= n_levels ? n_levels - 1 : sc);
}

}  // namespace vo
