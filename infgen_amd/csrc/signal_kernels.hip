// Signal-aware decoding (include/infgen_hip.h, "signal masks"): the allowed-token sets of one decode step from the map
// scene's stop lines and their phase at that step.
//
// k_signal_records        once per (re)load of the lines: one lane per line makes its record.
// k_signal_mask           the row skeleton of rider.cuh, one wave per row.  Its own part: lane l takes record l of the row's scene
//                         (K <= 64: one trip) and its phase byte, moves the record into the row's frame and evaluates "governs"; the
//                         governing records the row's tokens can reach at all are compacted, in order, into the wave's LDS list (two
//                         float4 per entry: q, v | half + hwa, g0, l0); every lane then walks the still-allowed tokens of its words
//                         against the list.  A row with an empty list reads no token and stores its base.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), no atomics, plain vector stores.
#include "kernels.h"
#include "rider.cuh"

namespace ig {

__global__ __launch_bounds__(64 * RIDER_WAVES) void k_signal_records(SignalRecArgs a) {
  const long long at = (long long)blockIdx.x * (64 * RIDER_WAVES) + threadIdx.x;
  if (at >= (long long)a.S0 * a.K) return;
  const int s0 = (int)(at / a.K), j = (int)(at - (long long)s0 * a.K);
  const int n = min(max(a.n_lines[s0], 0), a.K);
  const float inf = __builtin_inff();
  float4 r0 = make_float4(0.f, 0.f, 1.0f, 0.f), r1 = make_float4(-1.0f, 0.f, 0.f, 0.f);      // the dead record
  if (j < n) {
    const float4 ln = *reinterpret_cast<const float4*>(a.lines + 4 * (size_t)at);
    const float dx = ln.z - ln.x, dy = ln.w - ln.y;
    const float len = sqrtf(dx * dx + dy * dy);
    if (len > 0.f && len < inf && fabsf(ln.x) < inf && fabsf(ln.y) < inf) {
      const float ux = dx / len, uy = dy / len;
      r0 = make_float4(ln.x + 0.5f * dx, ln.y + 0.5f * dy, -uy, ux);
      r1.x = 0.5f * len;
    }
  }
  float4* const out = reinterpret_cast<float4*>(a.records + (size_t)at * SG_REC);
  out[0] = r0;
  out[1] = r1;
}

__global__ __launch_bounds__(64 * RIDER_WAVES) void k_signal_mask(SignalArgs a) {
  __shared__ float4 sg_lds[RIDER_WAVES * 2 * SG_MAX_LINES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4* const list_a = sg_lds + wave * (2 * SG_MAX_LINES);
  float4* const list_b = list_a + SG_MAX_LINES;
  const long long row_at = (long long)blockIdx.x * RIDER_WAVES + wave;
  if (row_at >= (long long)a.S * a.A_cap) return;                              // (uniform per wave; the kernel has no workgroup barrier)
  const int row = (int)row_at, A_cap = a.A_cap, words = a.token_size >> 5;
  const int s = row / A_cap, i = row - s * A_cap;
  const int n = scene_rows(a.n_agents, a.first_new, s, A_cap);
  const size_t col = ((size_t)s * a.T + a.c) * A_cap;                          // row 0 of column c
  unsigned cur[RIDER_WPL];
  const unsigned* bset = base_words(cur, a.base, row, words, lane);
  const int ty = clamp_type(a.type[row]);
  float4 info = make_float4(0.f, -1.0f, 0.f, 0.f);
  if (i < n && a.state[col + i] != INVALID && type_ruled(a.types, ty) != 0) {
    const RowBox r = row_box(a.pos, a.head, a.shape, a.end_pose, a.token_size, col, row, i, ty);
    const float dmax = a.end_pose[(size_t)3 * a.token_size * 4 + ty];          // the type's largest displacement
    const size_t s0 = (size_t)(s / a.copies);
    bool in = false;
    float gap = 0.f;
    int jb = -1;
    float4 ea = make_float4(0.f, 0.f, 1.0f, 0.f), eb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < a.K) {
      const float4* rec = reinterpret_cast<const float4*>(a.records) + (s0 * a.K + lane) * 2;
      const float4 r0 = rec[0];
      const float half = rec[1].x;
      const bool closed = a.phase[(s0 * a.n_phase + (size_t)(a.t % a.n_phase)) * a.K + lane] != 0;
      if (closed && half >= 0.f) {
        const float dx = r0.x - r.px, dy = r0.y - r.py;                        // world coordinates enter through this difference only
        const float qx = dx * r.ci + dy * r.si, qy = dy * r.ci - dx * r.si;
        const float vx = r0.z * r.ci + r0.w * r.si, vy = r0.w * r.ci - r0.z * r.si;
        const float ex = r.hla - qx, ey = 0.f - qy;                            // the row's front point less q
        const float g0 = (ex * vx + ey * vy) + a.setback;
        const float l0 = ex * vy - ey * vx;
        const float w = half + r.hwa;
        if (vx >= a.align && g0 <= 0.f) {                                      // governs
          if (fabsf(l0) <= w) { gap = 0.f - g0; jb = lane; }
          const float reach = (((dmax + r.hla) + w) + a.setback) + 0.01f;      // beyond it no token can make the front point cross
          in = qx * qx + qy * qy <= reach * reach;
          ea = make_float4(qx, qy, vx, vy);
          eb = make_float4(w, g0, l0, 0.f);
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                                   // the smallest gap, ties to the smaller index
      const float og = __shfl_xor(gap, off, 64);
      const int oj = __shfl_xor(jb, off, 64);
      if (oj >= 0 && (jb < 0 || og < gap || (og == gap && oj < jb))) { gap = og; jb = oj; }
    }
    info = make_float4(jb >= 0 ? gap : 0.f, (float)jb, jb >= 0 && gap <= dmax ? 2.0f : 1.0f, 0.f);
    // list_put bounds its index by RIDER_LIST, this kernel's lists hold SG_MAX_LINES entries: safe because the one call per row brings
    // at most 64 candidates (one per lane).  A second list_put per row would run list_a over into list_b
    static_assert(SG_MAX_LINES <= RIDER_LIST && SG_MAX_LINES == 64, "one list_put of a wave's 64 candidates fills a list at most");
    int m = 0;
    list_put(in, ea, eb, list_a, list_b, m, lane, [](int) {});                 // (64 entries at most: the list never fills)
    __builtin_amdgcn_wave_barrier();
    if (m > 0) {
#pragma unroll
      for (int q = 0; q < RIDER_WPL; ++q) {
        if (!cur[q]) continue;
        const int first = 32 * (lane + 64 * q);
        unsigned out = cur[q];
        for (int b = 0; b < 32; ++b) {
          if (!((cur[q] >> b) & 1u)) continue;
          const float4 p = r.pose[first + b];                                  // dx, dy, cos, sin of the end box in the row's frame
          const float fx = p.x + r.hla * p.z, fy = p.y + r.hla * p.w;          // the token's front point
          bool runs = false;
          for (int e = 0; e < m && !runs; ++e) {
            const float4 g = list_a[e];                                        // q, v
            const float4 h = list_b[e];                                        // half + hwa, g0, l0
            const float ex = fx - g.x, ey = fy - g.y;
            const float gk = (ex * g.z + ey * g.w) + a.setback;
            if (gk > 0.f) {
              const float lk = ex * g.w - ey * g.z;
              runs = fabsf(h.z * gk - lk * h.y) <= h.x * (gk - h.y);
            }
          }
          if (runs) out &= ~(1u << b);
        }
        cur[q] = out;
      }
    }
  }
  row_store(cur, bset, a.out_bits, a.out_count, row, words, lane);
  if (a.out_info && lane == 0) *reinterpret_cast<float4*>(a.out_info + 4 * (size_t)row) = info;
}

}  // namespace ig
