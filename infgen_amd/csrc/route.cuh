// The projection rule of the route records (include/infgen_hip.h, "route masks"), shared by k_route_mask
// (route_kernels.hip) and k_idm_command (controller_kernels.hip).
#pragma once
#include "kernels.h"

namespace ig {

constexpr int RT_SEGS = RT_MAX_POINTS;  // list entries per wave (31 used at most)

// the point (ex, ey) of the row's frame on the m list entries (la = q0 x, y, direction x, y; lb = L, cum): the arc length s of its
// projection onto the FIRST segment of least squared distance d2
struct RouteHit { float s, d2; };
__device__ __forceinline__ RouteHit route_project(float ex, float ey, const float4* la, const float4* lb, int m) {
  RouteHit h{0.f, __builtin_inff()};
  for (int e = 0; e < m; ++e) {
    const float4 g = la[e];
    const float4 q = lb[e];
    const float rx = ex - g.x, ry = ey - g.y;
    const float t = fminf(fmaxf(rx * g.z + ry * g.w, 0.f), q.x);
    const float fx = rx - t * g.z, fy = ry - t * g.w;
    const float d2 = fx * fx + fy * fy;
    if (d2 < h.d2) { h.d2 = d2; h.s = q.y + t; }
  }
  return h;
}

// the same rule, the same operations in the same order, with the list entry e of that segment and the offset vector (fx, fy) from the
// projection to the point.  A second function, so that k_route_mask's instructions stay what they were
struct RouteHitAt { float s, d2, fx, fy; int e; };
__device__ __forceinline__ RouteHitAt route_project_at(float ex, float ey, const float4* la, const float4* lb, int m) {
  RouteHitAt h{0.f, __builtin_inff(), 0.f, 0.f, 0};
  for (int e = 0; e < m; ++e) {
    const float4 g = la[e];
    const float4 q = lb[e];
    const float rx = ex - g.x, ry = ey - g.y;
    const float t = fminf(fmaxf(rx * g.z + ry * g.w, 0.f), q.x);
    const float fx = rx - t * g.z, fy = ry - t * g.w;
    const float d2 = fx * fx + fy * fy;
    if (d2 < h.d2) { h.d2 = d2; h.s = q.y + t; h.fx = fx; h.fy = fy; h.e = e; }
  }
  return h;
}

}  // namespace ig
