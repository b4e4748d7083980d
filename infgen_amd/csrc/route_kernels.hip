// Route-following decoding (include/infgen_hip.h, "route masks"): the allowed-token sets of one decode step from the
// rows' own routes.
//
// k_route_records         once per (re)load of the routes: one wave per row, lane j makes the record of segment j; the arc length in
//                         front of a segment is the in-order fp32 sum of the live lengths before it.
// k_route_mask            the row skeleton of rider.cuh, one wave per row.  Its own part: the row's at most 31 records are moved into
//                         the row's frame once (lane j takes record j) and compacted, in order, into the wave's LDS list; every lane
//                         projects the row's centre (s0, d0) and then the end-box centres of its words' tokens onto the list.  With
//                         pace > 0 the lane's words are walked twice: the first walk finds the on-route tokens and the wave's largest
//                         gain, the second bans what stays under the pace bar.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), no atomics, plain vector stores.
#include "kernels.h"
#include "rider.cuh"
#include "route.cuh"

namespace ig {

__global__ __launch_bounds__(64 * RIDER_WAVES) void k_route_records(RouteRecArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row_at = (long long)blockIdx.x * RIDER_WAVES + wave;
  if (row_at >= (long long)a.rows) return;                                     // (uniform per wave; the kernel has no workgroup barrier)
  const int row = (int)row_at, segs = a.P - 1;
  const int n = min(max(a.n_points[row], 0), a.P);
  const float* pt = a.routes + (size_t)row * a.P * 2;
  const float inf = __builtin_inff();
  float x0 = 0.f, y0 = 0.f, ux = 1.0f, uy = 0.f, L = -1.0f;                    // the dead record
  if (lane + 1 < n) {                                                          // segment `lane` joins the points lane, lane + 1
    const float ax = pt[2 * lane], ay = pt[2 * lane + 1], bx = pt[2 * lane + 2], by = pt[2 * lane + 3];
    const float dx = bx - ax, dy = by - ay;
    const float len = sqrtf(dx * dx + dy * dy);
    if (len > 0.f && len < inf && fabsf(ax) < inf && fabsf(ay) < inf) { x0 = ax; y0 = ay; ux = dx / len; uy = dy / len; L = len; }
  }
  // cum: the serial loop over the segments in order, run by every lane alike on the broadcast lengths - the in-order fp32 sum itself,
  // no prefix tree
  float run = 0.f, cum = 0.f;
  for (int j = 0; j < segs; ++j) {
    const float Lj = __shfl(L, j, 64);
    if (j == lane) cum = run;
    if (Lj > 0.f) run = run + Lj;
  }
  if (lane < segs) {
    float4* const out = reinterpret_cast<float4*>(a.records + ((size_t)row * segs + lane) * RT_REC);
    out[0] = make_float4(x0, y0, ux, uy);
    out[1] = make_float4(L, L > 0.f ? cum : 0.f, 0.f, 0.f);
  }
  if (lane == 0) a.total[row] = run;
}

__global__ __launch_bounds__(64 * RIDER_WAVES) void k_route_mask(RouteArgs a) {
  __shared__ float4 rt_lds[RIDER_WAVES * 2 * RT_SEGS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4* const list_a = rt_lds + wave * (2 * RT_SEGS);
  float4* const list_b = list_a + RT_SEGS;
  const long long row_at = (long long)blockIdx.x * RIDER_WAVES + wave;
  if (row_at >= (long long)a.S * a.A_cap) return;                              // (uniform per wave; the kernel has no workgroup barrier)
  const int row = (int)row_at, A_cap = a.A_cap, words = a.token_size >> 5;
  const int s = row / A_cap, i = row - s * A_cap;
  const int n = scene_rows(a.n_agents, a.first_new, s, A_cap);
  const size_t col = ((size_t)s * a.T + a.c) * A_cap;                          // row 0 of column c
  unsigned cur[RIDER_WPL];
  const unsigned* bset = base_words(cur, a.base, row, words, lane);
  const int ty = clamp_type(a.type[row]);
  const size_t rrow = (size_t)(s / a.copies) * A_cap + i;                      // the row of the route tables
  const float total = a.total[rrow];
  float4 prog = make_float4(0.f, 0.f, total, 0.f);
  if (i < n && a.state[col + i] != INVALID && type_ruled(a.types, ty) != 0 && total > 0.f) {
    const RowBox r = row_box(a.pos, a.head, a.shape, a.end_pose, a.token_size, col, row, i, ty);
    const int segs = a.P - 1;
    bool in = false;
    float4 ea = make_float4(0.f, 0.f, 1.0f, 0.f), eb = make_float4(-1.0f, 0.f, 0.f, 0.f);
    if (lane < segs) {
      const float4* rec = reinterpret_cast<const float4*>(a.records) + (rrow * segs + lane) * 2;
      const float4 r0 = rec[0], r1 = rec[1];
      in = r1.x > 0.f;
      const float dx = r0.x - r.px, dy = r0.y - r.py;                          // world coordinates enter through this difference only
      ea = make_float4(dx * r.ci + dy * r.si, dy * r.ci - dx * r.si, r0.z * r.ci + r0.w * r.si, r0.w * r.ci - r0.z * r.si);
      eb = make_float4(r1.x, r1.y, 0.f, 0.f);
    }
    int m = 0;
    list_put(in, ea, eb, list_a, list_b, m, lane, [](int) {});                 // (31 entries at most: the list never fills)
    __builtin_amdgcn_wave_barrier();
    const RouteHit h0 = route_project(0.f, 0.f, list_a, list_b, m);            // the row's centre, by every lane alike
    const float s0 = h0.s, d0 = sqrtf(h0.d2);
    const bool finished = !(s0 < total - a.finish);
    prog = make_float4(s0, d0, total, finished ? 2.0f : 1.0f);
    if (!finished) {
      const float lo = s0 - a.back;
      float gmax = -__builtin_inff();
#pragma unroll
      for (int q = 0; q < RIDER_WPL; ++q) {
        if (!cur[q]) continue;
        const int first = 32 * (lane + 64 * q);
        unsigned out = cur[q];
        for (int b = 0; b < 32; ++b) {
          if (!((cur[q] >> b) & 1u)) continue;
          const float4 p = r.pose[first + b];                                  // dx, dy of the end box's centre in the row's frame
          const RouteHit h = route_project(p.x, p.y, list_a, list_b, m);
          const float dk = sqrtf(h.d2);
          if ((dk <= a.corridor || dk < d0) && h.s >= lo) gmax = fmaxf(gmax, h.s - s0);
          else out &= ~(1u << b);
        }
        cur[q] = out;
      }
      if (a.pace > 0.f) {                                                      // (uniform)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, off, 64));
        if (gmax > 0.f) {
          const float bar = a.pace * gmax;
#pragma unroll
          for (int q = 0; q < RIDER_WPL; ++q) {
            if (!cur[q]) continue;
            const int first = 32 * (lane + 64 * q);
            unsigned out = cur[q];
            for (int b = 0; b < 32; ++b) {
              if (!((cur[q] >> b) & 1u)) continue;
              const float4 p = r.pose[first + b];
              const RouteHit h = route_project(p.x, p.y, list_a, list_b, m);
              if (h.s - s0 < bar) out &= ~(1u << b);
            }
            cur[q] = out;
          }
        }
      }
    }
  }
  row_store(cur, bset, a.out_bits, a.out_count, row, words, lane);
  if (a.out_progress && lane == 0) *reinterpret_cast<float4*>(a.out_progress + 4 * (size_t)row) = prog;
}

}  // namespace ig
