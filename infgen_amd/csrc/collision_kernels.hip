// Collision-aware decoding (include/infgen_hip.h, "collision masks"): the allowed-token sets of one decode step from the
// agents' boxes.
//
// k_collision_end_poses   once per vocabulary: (dx, dy, cos dtheta, sin dtheta) of every token's last contour in the agent frame and
//                         the largest displacement of each type.
// k_collision_mask        the row skeleton of rider.cuh, one wave per row, the rows of a scene grouped in workgroups (grid: row groups
//                         x scenes).  Its own part is the obstacle source: the workgroup stages the scene's obstacle rows in LDS once
//                         - centre of column c, the constant-velocity step (predict), cos / sin of the obstacle's heading, half extents
//                         enlarged by the margin, the enclosing radius (negative: not in the scene) - and a wave keeps the ones its
//                         row can reach at all (centre distance <= own radius + obstacle radius + the type's largest displacement).
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), plain stores.
#include "kernels.h"
#include "rider.cuh"
#include "tile.cuh"

namespace ig {

__global__ __launch_bounds__(256) void k_collision_end_poses(EndPoseArgs a) {
  __shared__ float s_max[4];
  const int ty = blockIdx.x, t = threadIdx.x;
  float best = 0.f;
  for (int k = t; k < a.token_size; k += 256) {
    const float* ct = a.vocab + ((size_t)ty * a.token_size + k) * 48 + 40;      // the last (k == 5) contour
    const float4 p0 = *reinterpret_cast<const float4*>(ct);
    const float4 p1 = *reinterpret_cast<const float4*>(ct + 4);
    const float dx = (((p0.x + p0.z) + p1.x) + p1.z) * 0.25f;
    const float dy = (((p0.y + p0.w) + p1.y) + p1.w) * 0.25f;
    const float hx = p0.x - p1.z, hy = p0.y - p1.w;                             // front-left minus rear-left
    const float len = sqrtf(hx * hx + hy * hy);
    const float cd = len > 0.f ? hx / len : 1.0f, sd = len > 0.f ? hy / len : 0.f;
    *reinterpret_cast<float4*>(a.end_pose + ((size_t)ty * a.token_size + k) * 4) = make_float4(dx, dy, cd, sd);
    best = fmaxf(best, sqrtf(dx * dx + dy * dy));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  if ((t & 63) == 0) s_max[t >> 6] = best;
  __syncthreads();
  if (t == 0) {
    a.end_pose[(size_t)3 * a.token_size * 4 + ty] = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    if (ty == 0) a.end_pose[(size_t)3 * a.token_size * 4 + 3] = 0.f;
  }
}

__global__ __launch_bounds__(64 * RIDER_WAVES) void k_collision_mask(CollisionArgs a) {
  extern __shared__ float4 cm_lds[];
  // [RIDER_WAVES][RIDER_LIST] x 2 float4 lists, then CM_STAGE planes of A_cap floats
  float4* const list_a = cm_lds + (threadIdx.x >> 6) * (2 * RIDER_LIST);
  float4* const list_b = list_a + RIDER_LIST;
  float* const stage = reinterpret_cast<float*>(cm_lds + RIDER_WAVES * 2 * RIDER_LIST);
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A_cap = a.A_cap, words = a.token_size >> 5;
  const int n = scene_rows(a.n_agents, a.first_new, s, A_cap);
  float* const g_cx = stage, *g_cy = stage + A_cap, *g_vx = stage + 2 * A_cap, *g_vy = stage + 3 * A_cap, *g_co = stage + 4 * A_cap,
       *g_so = stage + 5 * A_cap, *g_hl = stage + 6 * A_cap, *g_hw = stage + 7 * A_cap, *g_rad = stage + 8 * A_cap;
  const size_t col = ((size_t)s * a.T + a.c) * A_cap;                          // row 0 of column c; column c - 1 is A_cap in front
  for (int j = threadIdx.x; j < n; j += 64 * RIDER_WAVES) {
    const bool in = a.state[col + j] != INVALID;
    const bool vel = in && a.predict && a.c > 0 && a.state[col - A_cap + j] != INVALID;
    const float x = a.pos[2 * (col + j)], y = a.pos[2 * (col + j) + 1], h = a.head[col + j];
    float vx = 0.f, vy = 0.f, ang = h;
    if (vel) {
      vx = x - a.pos[2 * (col - A_cap + j)]; vy = y - a.pos[2 * (col - A_cap + j) + 1];
      ang = h + (h - a.head[col - A_cap + j]);
    }
    const float hl = 0.5f * a.shape[3 * ((size_t)s * A_cap + j)] + a.margin, hw = 0.5f * a.shape[3 * ((size_t)s * A_cap + j) + 1] + a.margin;
    g_cx[j] = x; g_cy[j] = y; g_vx[j] = vx; g_vy[j] = vy; g_co[j] = cosf(ang); g_so[j] = sinf(ang);
    g_hl[j] = hl; g_hw[j] = hw; g_rad[j] = in ? sqrtf(hl * hl + hw * hw) : -1.0f;
  }
  __syncthreads();
  const int r1 = min(A_cap, (int)(blockIdx.x + 1) * a.rows_per_wg);
  for (int i = blockIdx.x * a.rows_per_wg + wave; i < r1; i += RIDER_WAVES) {   // (uniform per wave)
    const int row = s * A_cap + i;
        unsigned cur[RIDER_WPL];
    const unsigned* bset = base_words(cur, a.base, row, words, lane);
    if (i < n && a.state[col + i] != INVALID) {
      const RowBox r = row_box(a.pos, a.head, a.shape, a.end_pose, a.token_size, col, row, i, clamp_type(a.type[row]));
      auto pass = [&](int m) __attribute__((always_inline)) { token_pass<false>(cur, lane, r, nullptr, list_a, list_b, m, 0); };
      int m = 0;
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        bool in = false;
        float4 ea = make_float4(0.f, 0.f, 1.0f, 0.f), eb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < n && j != i) {
          const float rad = g_rad[j];
          const float rx = (g_cx[j] - r.px) + g_vx[j], ry = (g_cy[j] - r.py) + g_vy[j];
          const float lim = r.reach + rad;
          in = rad >= 0.f && rx * rx + ry * ry <= lim * lim;
          if (in) {
            const float co = g_co[j], so = g_so[j];
            ea = make_float4(rx * r.ci + ry * r.si, ry * r.ci - rx * r.si, co * r.ci + so * r.si, so * r.ci - co * r.si);
            eb = make_float4(g_hl[j], g_hw[j], rad, 0.f);
          }
        }
        list_put(in, ea, eb, list_a, list_b, m, lane, pass);
      }
      if (m > 0) {
        __builtin_amdgcn_wave_barrier();
        pass(m);
        __builtin_amdgcn_wave_barrier();       // (the next row of this wave rewrites the list)
      }
    }
    row_store(cur, bset, a.out_bits, a.out_count, row, words, lane);
  }
}

}  // namespace ig
