// Rule-based controlled agents (include/infgen_hip.h, "IDM commands"): the next target pose of the rows that follow
// their route under the intelligent-driver law, in front of k_command_rows.
//
// k_idm_command           the row layout of rider.cuh, one wave per row, RIDER_WAVES rows per workgroup, no workgroup barrier.  A wave
//                         whose row is not ruled writes its zeros and leaves.  Otherwise lane j moves record j into the row's frame
//                         and list_put compacts the live ones, in order, into the wave's LDS list (k_route_mask's ea / eb, with the
//                         stored world direction in eb.z, eb.w for the target's heading); every lane projects the origin (s0, e0);
//                         the scene's rows are walked 64 at a time, lane = candidate j, each lane keeping its best (gap, j, vl); one
//                         wave arg-min by __shfl_xor, lexicographic on (gap, j), and a __shfl of the winner's vl; the law and the
//                         target are uniform, computed by every lane alike, stored by lane 0.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), no atomics, plain vector stores.
#include "kernels.h"
#include "rider.cuh"
#include "route.cuh"

namespace ig {

constexpr int IDM_NONE = 0x7fffffff;    // "no candidate" in the arg-min's index

__global__ __launch_bounds__(64 * RIDER_WAVES) void k_idm_command(IdmArgs a) {
  __shared__ float4 rt_lds[RIDER_WAVES * 2 * RT_SEGS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4* const list_a = rt_lds + wave * (2 * RT_SEGS);
  float4* const list_b = list_a + RT_SEGS;
  const long long row_at = (long long)blockIdx.x * RIDER_WAVES + wave;
  if (row_at >= (long long)a.S * a.A_cap) return;                              // (uniform per wave; the kernel has no workgroup barrier)
  const int row = (int)row_at, A_cap = a.A_cap;
  const int s = row / A_cap, i = row - s * A_cap;
  const int n = scene_rows(a.n_agents, nullptr, s, A_cap);
  const size_t col = ((size_t)s * a.T + a.c) * A_cap;                          // row 0 of column c
  const size_t prev = col - A_cap;                                             // ... of column c - 1 (c >= 1)
  const int ty = clamp_type(a.type[row]);
  const size_t rrow = (size_t)(s / a.copies) * A_cap + i;                      // the row of the route tables
  const float total = a.total[rrow];
  const float inf = __builtin_inff();
  if (!(a.ctl_row[row] != 0 && i < n && a.state[col + i] != INVALID && type_ruled(a.types, ty) != 0 && total > 0.f)) {
    if (lane == 0) {
      if (a.out_state) {
        float4* const out = reinterpret_cast<float4*>(a.out_state + 8 * (size_t)row);
        out[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        out[1] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (a.out_lead) a.out_lead[row] = -1;
    }
    return;
  }
  const float px = a.pos[2 * (col + i)], py = a.pos[2 * (col + i) + 1];
  const float ph = a.head[col + i];
  const float ci = cosf(ph), si = sinf(ph);
  const float len_i = a.shape[3 * (size_t)row], w_i = a.shape[3 * (size_t)row + 1];
  float v = 0.f;
  if (a.state[prev + i] != INVALID) {
    const float dx = px - a.pos[2 * (prev + i)], dy = py - a.pos[2 * (prev + i) + 1];
    v = sqrtf(dx * dx + dy * dy) / a.dt;
  }
  // the route list
  const int segs = a.P - 1;
  bool in = false;
  float4 ea = make_float4(0.f, 0.f, 1.0f, 0.f), eb = make_float4(-1.0f, 0.f, 1.0f, 0.f);
  if (lane < segs) {
    const float4* rec = reinterpret_cast<const float4*>(a.records) + (rrow * segs + lane) * 2;
    const float4 r0 = rec[0], r1 = rec[1];
    in = r1.x > 0.f;
    const float dx = r0.x - px, dy = r0.y - py;                                // world coordinates enter through this difference only
    ea = make_float4(dx * ci + dy * si, dy * ci - dx * si, r0.z * ci + r0.w * si, r0.w * ci - r0.z * si);
    eb = make_float4(r1.x, r1.y, r0.z, r0.w);
  }
  int m = 0;
  list_put(in, ea, eb, list_a, list_b, m, lane, [](int) {});                   // (31 entries at most: the list never fills)
  __builtin_amdgcn_wave_barrier();
  if (m == 0) {                                                                // (total > 0 without a live record - not a table of
    if (lane == 0) { list_a[0] = make_float4(0.f, 0.f, 1.0f, 0.f); list_b[0] = make_float4(0.f, 0.f, 1.0f, 0.f); }   // infgen_route_records:
    __builtin_amdgcn_wave_barrier();                                           // a stand-in entry, so that no stale LDS is read; the
  }                                                                            // row keeps its position and is given heading 0)
  const RouteHitAt h0 = route_project_at(0.f, 0.f, list_a, list_b, m);         // the row's centre, by every lane alike
  const float s0 = h0.s;
  const float4 u0 = list_a[h0.e];
  const float e0 = h0.fx * (-u0.w) + h0.fy * u0.z;
  // the lead search: lane = candidate j, 64 at a time
  float best_gap = inf, best_vl = 0.f;
  int best_j = IDM_NONE;
  for (int first = 0; first < n; first += 64) {
    const int j = first + lane;
    if (j < n && j != i && a.state[col + j] != INVALID) {
      const float jx = a.pos[2 * (col + j)], jy = a.pos[2 * (col + j) + 1];
      const float dx = jx - px, dy = jy - py;
      const RouteHitAt h = route_project_at(dx * ci + dy * si, dy * ci - dx * si, list_a, list_b, m);
      const size_t jrow = (size_t)s * A_cap + j;
      const float len_j = a.shape[3 * jrow], w_j = a.shape[3 * jrow + 1];
      if (sqrtf(h.d2) <= a.lateral + 0.5f * (w_i + w_j) && h.s > s0) {
        const float gap = (h.s - s0) - 0.5f * (len_i + len_j);
        if (gap < best_gap) {                                                  // (j ascends in a lane: ties stay with the lowest)
          float vl = 0.f;
          if (a.state[prev + j] != INVALID) {
            const float vx = jx - a.pos[2 * (prev + j)], vy = jy - a.pos[2 * (prev + j) + 1];
            const float4 uj = list_a[h.e];
            vl = fmaxf(0.f, ((vx * ci + vy * si) * uj.z + (vy * ci - vx * si) * uj.w) / a.dt);
          }
          best_gap = gap; best_j = j; best_vl = vl;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float og = __shfl_xor(best_gap, off, 64);
    const int oj = __shfl_xor(best_j, off, 64);
    if (og < best_gap || (og == best_gap && oj < best_j)) { best_gap = og; best_j = oj; }
  }
  float gap = inf, vl = 0.f;
  int lead = -1;
  const float won = __shfl(best_vl, best_j & 63, 64);                          // (candidate j sat in lane j & 63 of its trip)
  if (best_j != IDM_NONE) { gap = best_gap; vl = won; lead = best_j; }
  if (a.stop_at_end != 0) {
    const float end_gap = (total - s0) - 0.5f * len_i;
    if (end_gap < gap) { gap = end_gap; vl = 0.f; lead = -2; }
  }
  // the law
  const float g = fmaxf(gap, 0.1f);
  float v0 = ty == 0 ? a.v0_type[0] : ty == 1 ? a.v0_type[1] : a.v0_type[2];
  if (a.v_des) {
    const float want = a.v_des[rrow];
    if (want > 0.f) v0 = want;
  }
  const float sstar = a.s_min + fmaxf(0.f, v * a.headway + v * (v - vl) / (2.0f * sqrtf(a.a_max * a.b_comf)));
  const float r = v / v0;
  const float free_term = 1.0f - (r * r) * (r * r);
  const float q = lead == -1 ? 0.f : sstar / g;
  const float acc = fminf(fmaxf(a.a_max * (free_term - q * q), -a.b_max), a.a_max);
  const float v1 = fmaxf(0.f, v + acc * a.dt);
  const float s1 = fminf(s0 + 0.5f * (v + v1) * a.dt, total);
  // the target
  int at = max(m - 1, 0);
  for (int e = 0; e < m; ++e) {
    const float4 lb = list_b[e];
    if (s1 <= lb.y + lb.x) { at = e; break; }
  }
  const float4 ga = list_a[at], gb = list_b[at];
  const float a1 = fminf(fmaxf(s1 - gb.y, 0.f), gb.x);
  const float ke = a.keep * e0;
  const float tx = (ga.x + a1 * ga.z) + ke * (-ga.w);
  const float tz = (ga.y + a1 * ga.w) + ke * ga.z;
  const float x = px + (tx * ci - tz * si), y = py + (tx * si + tz * ci);
  const float heading = atan2f(gb.w, gb.z);
  if (lane == 0) {
    float* const pose = a.cmd_pose + 3 * (size_t)row;
    pose[0] = x; pose[1] = y; pose[2] = heading;
    if (a.out_state) {
      float4* const out = reinterpret_cast<float4*>(a.out_state + 8 * (size_t)row);
      out[0] = make_float4(s0, e0, v, gap);
      out[1] = make_float4(acc, v1, s1, 1.0f);
    }
    if (a.out_lead) a.out_lead[row] = lead;
  }
}

}  // namespace ig
