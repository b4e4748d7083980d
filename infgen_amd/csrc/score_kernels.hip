// Step scores (include/infgen_hip.h, "step scores"): the per-slot overlap, off-road and comfort terms of the column a
// decode step just produced, 8 floats per scene slot, and one flag byte per row.
//
// k_step_score            one workgroup per scene slot:
//   0. lane i stages row i's pose of column c1 - world position, cos, sin - and its half extents and radius in LDS (radius -1: not
//      live), and keeps the row's comfort terms (speed change over columns c1 - 2 .. c1, yaw rate over c1 - 1 .. c1) in registers;
//   1. the pair pass: SC_NT lanes cover (row, slice of the other rows), P = 1 .. 64 adjacent lanes per row.  pos[j] - pos[i] is formed
//      from the staged world coordinates, rotated into row i's frame, and meets sat_sep behind a circle reject that also knows the
//      lane's running minimum: with D the centre distance, sep >= D / sqrt(2) - (r_i + r_j), so a pair whose bound is neither below
//      0 nor below the minimum so far can change neither the flag nor min_sep;
//   2. the road pass: the same lanes cover (row, slice of records); the records stream from global memory (two 16-byte loads per
//      lane) and enter through rider.cuh's road-record entry - the one k_road_mask bans by -, the row's box (its own frame) and,
//      with sweep, its path rectangle (world axes) each behind a circle reject;
//   3. counts, the minimum and the two maxima: a wave reduction each, one LDS combine over the waves, two 16-byte stores; the flag
//      bytes leave LDS with plain byte stores.
// Every reduction is a count, a min or a max: the result does not depend on the order.  fp32 throughout, no fused multiply-add (the
// build's -ffp-contract=off), no atomics, plain vector stores.
#include "kernels.h"
#include "rider.cuh"

namespace ig {

__device__ __forceinline__ float score_abs_wrap(float a) {          // |wrap to [-pi, pi)| of a heading difference
  const float PI_F = 3.14159274f, TWO_PI_F = 6.28318548f;
  float r = fmodf(a + PI_F, TWO_PI_F);
  if (r < 0.f) r += TWO_PI_F;
  return fabsf(r - PI_F);
}

__global__ __launch_bounds__(SC_NT) void k_step_score(ScoreArgs a) {
  __shared__ float4 row_a[MAX_SCENE_AGENTS];                 // world x, y, cos, sin of the pose of column c1
  __shared__ float4 row_b[MAX_SCENE_AGENTS];                 // half length, half width, radius (-1: the row is not live), 0
  __shared__ unsigned char row_flag[MAX_SCENE_AGENTS];
  __shared__ float red_f[SC_NT / 64][3];
  __shared__ int red_i[SC_NT / 64][3];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A_cap = a.A_cap, c1 = a.c1;
  const int n = min(max(a.n_agents[s], 0), A_cap);
  const size_t col = ((size_t)s * a.T + c1) * A_cap;                             // row 0 of column c1
  const float inf = __builtin_inff();
  int n_live = 0, n_overlap = 0, n_offroad = 0;
  float min_sep = inf, max_accel = 0.f, max_yaw = 0.f;

  // 0. staging, and the comfort terms of the rows this lane stages
  const float dt2 = a.dt * a.dt;
  for (int i = tid; i < A_cap; i += SC_NT) {
    const bool live = i < n && a.state[col + i] != INVALID;
    float4 ra = make_float4(0.f, 0.f, 1.0f, 0.f), rb = make_float4(0.f, 0.f, -1.0f, 0.f);
    if (live) {
      const float px = a.pos[2 * (col + i)], py = a.pos[2 * (col + i) + 1], ph = a.head[col + i];
      const float hl = 0.5f * a.shape[3 * ((size_t)s * A_cap + i)], hw = 0.5f * a.shape[3 * ((size_t)s * A_cap + i) + 1];
      ra = make_float4(px, py, cosf(ph), sinf(ph));
      rb = make_float4(hl, hw, sqrtf(hl * hl + hw * hw), 0.f);
      ++n_live;
      if (c1 >= 1 && a.state[col - A_cap + i] != INVALID) {
        const size_t p1 = col - A_cap + i;
        max_yaw = fmaxf(max_yaw, score_abs_wrap(ph - a.head[p1]) / a.dt);
        if (c1 >= 2 && a.state[p1 - A_cap] != INVALID) {
          const size_t p2 = p1 - A_cap;
          const float x1 = a.pos[2 * p1], y1 = a.pos[2 * p1 + 1];
          const float ux = px - x1, uy = py - y1, vx = x1 - a.pos[2 * p2], vy = y1 - a.pos[2 * p2 + 1];
          max_accel = fmaxf(max_accel, fabsf(sqrtf(ux * ux + uy * uy) - sqrtf(vx * vx + vy * vy)) / dt2);
        }
      }
    }
    row_a[i] = ra;
    row_b[i] = rb;
    row_flag[i] = live ? 1 : 0;
  }
  __syncthreads();

  // P adjacent lanes per row, a power of two: the rows' lanes never straddle a wave
  int P = 1;
  while (P < 64 && n * P < SC_NT) P <<= 1;
  const int shift = __builtin_ctz(P);
  const int rounds = (n * P + SC_NT - 1) / SC_NT;
  const int ms = s / a.copies;
  const int nr = a.records ? min(max(a.n_records[ms], 0), a.rec_cap) : 0;
  const float4* rec = nr > 0 ? reinterpret_cast<const float4*>(a.records) + (size_t)ms * a.rec_cap * 2 : nullptr;

  for (int round = 0; round < rounds; ++round) {             // (uniform: every lane of a wave reaches the shuffles)
    const int item = round * SC_NT + tid;
    const int i = item >> shift, q = item & (P - 1);
    float4 ia = make_float4(0.f, 0.f, 1.0f, 0.f), ib = make_float4(0.f, 0.f, -1.0f, 0.f);
    if (i < n) { ia = row_a[i]; ib = row_b[i]; }
    const bool live = ib.z >= 0.f;

    // 1. the pair pass
    float m = inf;
    int hit = 0;
    if (live) {
      for (int j = q; j < n; j += P) {
        const float4 jb = row_b[j];
        if (j == i || jb.z < 0.f) continue;
        const float4 ja = row_a[j];
        const float dx = ja.x - ia.x, dy = ja.y - ia.y;
        const float lim = (ib.z + jb.z) + fmaxf(m, 0.f);
        if (dx * dx + dy * dy >= 2.0f * (lim * lim)) continue;                   // sep >= D / sqrt(2) - (r_i + r_j) >= max(m, 0)
        const float ox = dx * ia.z + dy * ia.w, oy = dy * ia.z - dx * ia.w;
        const float oc = ja.z * ia.z + ja.w * ia.w, os = ja.w * ia.z - ja.z * ia.w;
        const float sep = sat_sep(ox, oy, 1.0f, 0.f, ib.x, ib.y, oc, os, jb.x, jb.y);
        m = fminf(m, sep);
        hit |= sep < 0.f ? 1 : 0;
      }
    }
    for (int off = P >> 1; off > 0; off >>= 1) { m = fminf(m, __shfl_xor(m, off, 64)); hit |= __shfl_xor(hit, off, 64); }
    min_sep = fminf(min_sep, m);

    // 2. the road pass
    int off_road = 0;
    if (nr > 0) {                                                                 // (uniform)
      if (live) {
        if (type_ruled(a.types, clamp_type(a.type[(size_t)s * A_cap + i])) != 0) {
          float ddx = 0.f, ddy = 0.f, ux = 1.0f, uy = 0.f, hd = 0.f;             // the displacement, its direction and half length
          if (a.sweep && c1 >= 1 && a.state[col - A_cap + i] != INVALID) {
            ddx = ia.x - a.pos[2 * (col - A_cap + i)]; ddy = ia.y - a.pos[2 * (col - A_cap + i) + 1];
            const float d = sqrtf(ddx * ddx + ddy * ddy);
            if (d > 0.f) { ux = ddx / d; uy = ddy / d; hd = 0.5f * d; }
          }
          const bool swept = hd > 0.f;
          const float rp = hd + ib.y;                                             // a radius that encloses the path rectangle
          for (int j = q; j < nr && !off_road; j += P) {
            const float4 r0 = rec[2 * j], r1 = rec[2 * j + 1];
            if (!(r1.w >= 0.f)) continue;
            const RoadRel e = road_rel(r0, r1, ia.x, ia.y, a.margin);
            const float rr = ib.z + e.orad;
            float4 at;
            if (e.rx * e.rx + e.ry * e.ry <= rr * rr) off_road = road_own_sep(e, r1, ia.z, ia.w, ib.x, ib.y, a.margin, &at) < 0.f ? 1 : 0;
            if (!off_road && swept) {
              const float ex = e.rx + 0.5f * ddx, ey = e.ry + 0.5f * ddy;        // the record seen from the displacement's midpoint
              const float rs = rp + e.orad;
              if (ex * ex + ey * ey <= rs * rs) off_road = sat_sep(ex, ey, ux, uy, hd, ib.y, r1.x, r1.y, e.hlo, a.margin) < 0.f ? 1 : 0;
            }
          }
        }
      }
      for (int off = P >> 1; off > 0; off >>= 1) off_road |= __shfl_xor(off_road, off, 64);
    }
    if (live && q == 0) {                                                         // one lane owns the row's flags
      n_overlap += hit;
      n_offroad += off_road;
      row_flag[i] = (unsigned char)(1 | (hit << 1) | (off_road << 2));
    }
  }

  // 3. wave reductions, one LDS combine
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_live += __shfl_xor(n_live, off, 64); n_overlap += __shfl_xor(n_overlap, off, 64); n_offroad += __shfl_xor(n_offroad, off, 64);
    min_sep = fminf(min_sep, __shfl_xor(min_sep, off, 64));
    max_accel = fmaxf(max_accel, __shfl_xor(max_accel, off, 64));
    max_yaw = fmaxf(max_yaw, __shfl_xor(max_yaw, off, 64));
  }
  if (lane == 0) {
    red_i[wave][0] = n_live; red_i[wave][1] = n_overlap; red_i[wave][2] = n_offroad;
    red_f[wave][0] = min_sep; red_f[wave][1] = max_accel; red_f[wave][2] = max_yaw;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SC_NT / 64; ++w) {
      n_live += red_i[w][0]; n_overlap += red_i[w][1]; n_offroad += red_i[w][2];
      min_sep = fminf(min_sep, red_f[w][0]); max_accel = fmaxf(max_accel, red_f[w][1]); max_yaw = fmaxf(max_yaw, red_f[w][2]);
    }
    float4* const out = reinterpret_cast<float4*>(a.out + (size_t)s * a.out_stride);
    out[0] = make_float4((float)n_live, (float)n_overlap, min_sep, (float)n_offroad);
    out[1] = make_float4(max_accel, max_yaw, 0.f, 0.f);
  }
  if (a.out_row)
    for (int i = tid; i < A_cap; i += SC_NT) a.out_row[(size_t)s * A_cap + i] = row_flag[i];
}

}  // namespace ig
