// Collision-aware decoding (include/infgen_hip.h, "collision masks"): the allowed-token sets of one decode step from the
// agents' boxes.
//
// k_collision_end_poses   once per vocabulary: (dx, dy, cos dtheta, sin dtheta) of every token's last contour in the agent frame and
//                         the largest displacement of each type.
// k_collision_mask        one wave per row, the rows of a scene grouped in workgroups (grid: row groups x scenes):
//   1. the workgroup stages the scene's obstacle rows in LDS once: centre of column c, the constant-velocity step (predict), cos / sin
//      of the obstacle's heading, half extents enlarged by the margin, the enclosing radius (negative: not in the scene);
//   2. a wave walks them 64 at a time and compacts - ballot + popcount - the ones its row can reach at all (centre distance <= own
//      radius + obstacle radius + the type's largest token displacement) into its own LDS list, already moved into the ROW's frame
//      (translated by pos[c][i] first, then rotated by -head[c][i]): magnitudes stay at tens of metres wherever the scene lies;
//   3. lane l owns the 32-token words l, l + 64 of the set: for each of a word's tokens still allowed it runs a circle reject, then the
//      separating-axis test over the four axes, against the list; the word is assembled in a register and leaves with one store.
//      A row with an empty list writes base(i) without reading a token; more than CM_LIST reachable obstacles take further passes;
//   4. the "any token left?" of the fallback is a wave reduction of the words' OR, the count one of their popcounts.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), plain stores.
#include "kernels.h"
#include "sat.cuh"
#include "tile.cuh"

namespace ig {

constexpr int CM_INVALID = 0;           // valid_state_type id of 'invalid' (edge_kernels.hip)

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

// the tokens of word `cur` (bits still allowed) of a row with half extents (hla, hwa) and radius ra against the n list entries of the
// wave: returns the word without the colliding tokens.  pose: the type's end poses of the word's 32 tokens
__device__ __forceinline__ unsigned collide_word(unsigned cur, const float4* __restrict__ pose, const float4* la, const float4* lb, int n,
                                                 float hla, float hwa, float ra) {
  unsigned out = cur;
  for (int b = 0; b < 32; ++b) {
    if (!((cur >> b) & 1u)) continue;
    const float4 p = pose[b];                                                  // dx, dy, cos, sin of the candidate in the row's frame
    bool hit = false;
    for (int e = 0; e < n && !hit; ++e) {
      const float4 o = la[e];                                                  // centre, cos, sin of the obstacle in the row's frame
      const float4 q = lb[e];                                                  // half length, half width, radius
      const float ddx = o.x - p.x, ddy = o.y - p.y;
      const float rr = ra + q.z;
      if (ddx * ddx + ddy * ddy > rr * rr) continue;                           // the enclosing circles are apart
      hit = sat_sep(ddx, ddy, p.z, p.w, hla, hwa, o.z, o.w, q.x, q.y) < 0.f;      // (sat.cuh: the four axes, shared with k_road_mask)
    }
    if (hit) out &= ~(1u << b);
  }
  return out;
}

__global__ __launch_bounds__(64 * CM_WAVES) void k_collision_mask(CollisionArgs a) {
  extern __shared__ float4 cm_lds[];
  // [CM_WAVES][CM_LIST] x 2 float4 lists, then CM_STAGE planes of A_cap floats
  float4* const list_a = cm_lds + (threadIdx.x >> 6) * (2 * CM_LIST);
  float4* const list_b = list_a + CM_LIST;
  float* const stage = reinterpret_cast<float*>(cm_lds + CM_WAVES * 2 * CM_LIST);
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A_cap = a.A_cap, words = a.token_size >> 5;
  int n = a.n_agents[s];
  if (a.first_new) n = min(n, a.first_new[s]);
  n = min(n, A_cap);
  float* const g_cx = stage, *g_cy = stage + A_cap, *g_vx = stage + 2 * A_cap, *g_vy = stage + 3 * A_cap, *g_co = stage + 4 * A_cap,
       *g_so = stage + 5 * A_cap, *g_hl = stage + 6 * A_cap, *g_hw = stage + 7 * A_cap, *g_rad = stage + 8 * A_cap;
  const size_t col = ((size_t)s * a.T + a.c) * A_cap;                          // row 0 of column c; column c - 1 is A_cap in front
  for (int j = threadIdx.x; j < n; j += 64 * CM_WAVES) {
    const bool in = a.state[col + j] != CM_INVALID;
    const bool vel = in && a.predict && a.c > 0 && a.state[col - A_cap + j] != CM_INVALID;
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
  for (int i = blockIdx.x * a.rows_per_wg + wave; i < r1; i += CM_WAVES) {      // (uniform per wave)
    const int row = s * A_cap + i;
    const unsigned* bset = a.base.bits ? token_mask_set(a.base, row, words) : nullptr;
    unsigned* const out = a.out_bits + (size_t)row * words;
    unsigned cur[CM_WPL];
#pragma unroll
    for (int q = 0; q < CM_WPL; ++q) {
      const int w = lane + 64 * q;
      cur[q] = w < words ? (bset ? bset[w] : 0xffffffffu) : 0u;
    }
    const bool live = i < n && a.state[col + i] != CM_INVALID;
    int ty = a.type[row];
    if (ty < 0 || ty > 2) ty = 0;
    if (live) {
      const float px = a.pos[2 * (col + i)], py = a.pos[2 * (col + i) + 1], ph = a.head[col + i];
      const float ci = cosf(ph), si = sinf(ph);
      const float hla = 0.5f * a.shape[3 * (size_t)row], hwa = 0.5f * a.shape[3 * (size_t)row + 1];
      const float ra = sqrtf(hla * hla + hwa * hwa);
      const float reach = ra + a.end_pose[(size_t)3 * a.token_size * 4 + ty];
      const float4* pose = reinterpret_cast<const float4*>(a.end_pose) + (size_t)ty * a.token_size;
      int m = 0;
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        bool in = false;
        float rx = 0.f, ry = 0.f, rad = 0.f;
        if (j < n && j != i) {
          rad = g_rad[j];
          rx = (g_cx[j] - px) + g_vx[j]; ry = (g_cy[j] - py) + g_vy[j];
          const float lim = reach + rad;
          in = rad >= 0.f && rx * rx + ry * ry <= lim * lim;
        }
        unsigned long long bal = __ballot(in);
        while (bal) {                                                           // (uniform: at most two rounds per 64 obstacles)
          const int before = __popcll(bal & ((1ull << lane) - 1ull));
          const bool put = in && ((bal >> lane) & 1ull) && m + before < CM_LIST;
          if (put) {
            const float co = g_co[j], so = g_so[j];
            list_a[m + before] = make_float4(rx * ci + ry * si, ry * ci - rx * si, co * ci + so * si, so * ci - co * si);
            list_b[m + before] = make_float4(g_hl[j], g_hw[j], rad, 0.f);
          }
          const unsigned long long done = __ballot(put);
          m += (int)__popcll(done);
          bal &= ~done;
          if (bal) {                                                            // the list is full: a pass over the tokens, then go on
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < CM_WPL; ++q)
              if (cur[q]) cur[q] = collide_word(cur[q], pose + 32 * (lane + 64 * q), list_a, list_b, m, hla, hwa, ra);
            __builtin_amdgcn_wave_barrier();
            m = 0;
          }
        }
      }
      if (m > 0) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < CM_WPL; ++q)
          if (cur[q]) cur[q] = collide_word(cur[q], pose + 32 * (lane + 64 * q), list_a, list_b, m, hla, hwa, ra);
        __builtin_amdgcn_wave_barrier();       // (the next row of this wave rewrites the list)
      }
    }
    // the fallback's "any token left?" and the count: wave reductions over the words
    unsigned any = 0u;
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < CM_WPL; ++q) { any |= cur[q]; cnt += __popc(cur[q]); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { any |= __shfl_xor(any, off, 64); cnt += __shfl_xor(cnt, off, 64); }
    if (a.out_count && lane == 0) a.out_count[row] = cnt;
    const bool fallback = any == 0u;      // (every reachable token collides: the row keeps its static set)
#pragma unroll
    for (int q = 0; q < CM_WPL; ++q) {
      const int w = lane + 64 * q;
      if (w < words) out[w] = fallback ? (bset ? bset[w] : 0xffffffffu) : cur[q];
    }
  }
}

}  // namespace ig
