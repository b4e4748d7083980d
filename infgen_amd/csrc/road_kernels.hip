// Road-aware decoding (include/infgen_hip.h, "road masks"): the allowed-token sets of one decode step from the map's
// road-edge segments.
//
// k_road_records_map / k_road_records_seg   once per reload: the compacted table of segment records of every distinct scene, from the
//                         EDGE map tokens' vocabulary polylines or from explicit world-coordinate segments.
// k_road_paths            once per vocabulary: direction and half length of every token's end displacement (the path rectangle).
// k_road_mask             one wave per row:
//   1. the wave streams its map scene's records 64 at a time from global memory (two 16-byte loads per lane) and keeps the ones the
//      row can reach at all (midpoint distance <= own radius + the type's largest token displacement + the obstacle's radius), moved
//      into the ROW's frame: (anchor - pos[c][i]) + offset first - world coordinates enter through that exact difference only -, then
//      rotated by -head[c][i];
//   2. a record whose obstacle rectangle overlaps the row's current box (the identity pose of that frame) is straddled and dropped;
//      the others are ballot-compacted into the wave's LDS list;
//   3. lane l owns the 32-token words l, l + 64 of the set: every token still allowed is tested against the list, its end box and
//      (sweep) its path rectangle, each behind a circle reject; the word is assembled in a register and leaves with one store.
//      A row with an empty list writes base(i) without reading a token; more than RM_LIST kept records take further passes;
//   4. the fallback's "any token left?" is a wave reduction of the words' OR, the count one of their popcounts.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), plain vector stores.
#include "kernels.h"
#include "sat.cuh"

namespace ig {

constexpr int RM_INVALID = 0;           // valid_state_type id of 'invalid' (edge_kernels.hip)
constexpr long long RM_EDGE = 12;       // the map-token type EDGE
constexpr int RM_POLY = 11;             // points of a map-vocabulary polyline

// one record from a segment given relative to its anchor: (x0, y0) -> (x1, y1).  A zero-length or non-finite segment: all zeros, radius -1
__device__ __forceinline__ void road_record(float* rec, float ax, float ay, float x0, float y0, float x1, float y1) {
  const float dx = x1 - x0, dy = y1 - y0;
  const float L = sqrtf(dx * dx + dy * dy);
  const float inf = __builtin_inff();
  const bool ok = L > 0.f && L < inf && fabsf(ax) < inf && fabsf(ay) < inf && fabsf(x0) < inf && fabsf(y0) < inf;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(1.0f, 0.f, 0.f, -1.0f);
  if (ok) {
    r0 = make_float4(ax, ay, 0.5f * (x0 + x1), 0.5f * (y0 + y1));
    r1 = make_float4(dx / L, dy / L, 0.5f * L, 0.5f * L);
  }
  *reinterpret_cast<float4*>(rec) = r0;
  *reinterpret_cast<float4*>(rec + 4) = r1;
}

__global__ __launch_bounds__(64) void k_road_records_map(RoadMapArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(a.n_map[s], 0), a.M_cap);
  const int hop = (RM_POLY - 1) / a.detail;
  float* const out = a.records + (size_t)s * a.rec_cap * RM_REC;
  int count = 0;                                                                 // EDGE tokens in front of this round (uniform)
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane;
    const size_t at = (size_t)s * a.M_cap + m;
    long long tk = 0;
    bool edge = false;
    if (m < n) {
      tk = a.map_tok[at];
      edge = a.map_type[at] == RM_EDGE && tk >= 0 && tk < a.n_token;
    }
    const unsigned long long bal = __ballot(edge);
    if (edge) {
      const int rank = count + (int)__popcll(bal & ((1ull << lane) - 1ull));
      const float ax = a.map_pos[2 * at], ay = a.map_pos[2 * at + 1], th = a.map_orient[at];
      const float co = cosf(th), so = sinf(th);
      const float* pl = a.map_vocab + (size_t)tk * (RM_POLY * 2);
      for (int j = 0; j < a.detail; ++j) {
        const int slot = rank * a.detail + j;
        if (slot >= a.rec_cap) break;
        const float qx0 = pl[2 * (j * hop)], qy0 = pl[2 * (j * hop) + 1], qx1 = pl[2 * ((j + 1) * hop)], qy1 = pl[2 * ((j + 1) * hop) + 1];
        road_record(out + (size_t)slot * RM_REC, ax, ay, qx0 * co - qy0 * so, qx0 * so + qy0 * co, qx1 * co - qy1 * so, qx1 * so + qy1 * co);
      }
    }
    count += (int)__popcll(bal);
  }
  if (lane == 0) a.n_records[s] = min(count * a.detail, a.rec_cap);
}

__global__ __launch_bounds__(256) void k_road_records_seg(RoadSegArgs a) {
  const int s = blockIdx.x;
  const int n = min(min(max(a.n_segments[s], 0), a.E), a.rec_cap);
  for (int e = threadIdx.x; e < n; e += 256) {
    const float4 g = *reinterpret_cast<const float4*>(a.segments + ((size_t)s * a.E + e) * 4);
    road_record(a.records + ((size_t)s * a.rec_cap + e) * RM_REC, g.x, g.y, 0.f, 0.f, g.z - g.x, g.w - g.y);
  }
  if (threadIdx.x == 0) a.n_records[s] = n;
}

__global__ __launch_bounds__(256) void k_road_paths(RoadPathArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= 3 * a.token_size) return;
  const float4 p = *reinterpret_cast<const float4*>(a.end_pose + (size_t)k * 4);
  const float d = sqrtf(p.x * p.x + p.y * p.y);
  *reinterpret_cast<float4*>(a.paths + (size_t)k * 4) = d > 0.f ? make_float4(p.x / d, p.y / d, 0.5f * d, 0.f) : make_float4(1.0f, 0.f, 0.f, 0.f);
}

// the tokens of word `cur` (bits still allowed) of a row with half extents (hla, hwa) and radius ra against the n list entries of the
// wave: returns the word without the off-road tokens.  pose / path: the type's end poses and path entries of the word's 32 tokens
__device__ __forceinline__ unsigned road_word(unsigned cur, const float4* __restrict__ pose, const float4* __restrict__ path, const float4* la,
                                              const float4* lb, int n, float hla, float hwa, float ra, int sweep) {
  unsigned out = cur;
  for (int b = 0; b < 32; ++b) {
    if (!((cur >> b) & 1u)) continue;
    const float4 p = pose[b];                                                  // dx, dy, cos, sin of the end box in the row's frame
    float4 w = make_float4(1.0f, 0.f, 0.f, 0.f);
    if (sweep) w = path[b];                                                    // cos, sin, half length of the path rectangle
    const bool swept = w.z > 0.f;
    const float mx = 0.5f * p.x, my = 0.5f * p.y, rp = w.z + hwa;              // its centre and a radius that encloses it
    bool hit = false;
    for (int e = 0; e < n && !hit; ++e) {
      const float4 o = la[e];                                                  // midpoint, cos, sin of the record in the row's frame
      const float4 q = lb[e];                                                  // half length, half width, radius of its obstacle rectangle
      const float ddx = o.x - p.x, ddy = o.y - p.y;
      const float rr = ra + q.z;
      if (ddx * ddx + ddy * ddy <= rr * rr) hit = sat_sep(ddx, ddy, p.z, p.w, hla, hwa, o.z, o.w, q.x, q.y) < 0.f;
      if (!hit && swept) {
        const float ex = o.x - mx, ey = o.y - my;
        const float rs = rp + q.z;
        if (ex * ex + ey * ey <= rs * rs) hit = sat_sep(ex, ey, w.x, w.y, w.z, hwa, o.z, o.w, q.x, q.y) < 0.f;
      }
    }
    if (hit) out &= ~(1u << b);
  }
  return out;
}

__global__ __launch_bounds__(64 * RM_WAVES) void k_road_mask(RoadArgs a) {
  __shared__ float4 rm_lds[RM_WAVES * 2 * RM_LIST];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4* const list_a = rm_lds + wave * (2 * RM_LIST);
  float4* const list_b = list_a + RM_LIST;
  const long long row_at = (long long)blockIdx.x * RM_WAVES + wave;
  if (row_at >= (long long)a.S * a.A_cap) return;                              // (uniform per wave; the kernel has no workgroup barrier)
  const int row = (int)row_at, A_cap = a.A_cap, words = a.token_size >> 5;
  const int s = row / A_cap, i = row - s * A_cap;
  int n = a.n_agents[s];
  if (a.first_new) n = min(n, a.first_new[s]);
  n = min(n, A_cap);
  const size_t col = ((size_t)s * a.T + a.c) * A_cap;                          // row 0 of column c
  const unsigned* bset = a.base.bits ? token_mask_set(a.base, row, words) : nullptr;
  unsigned* const out = a.out_bits + (size_t)row * words;
  unsigned cur[RM_WPL];
#pragma unroll
  for (int q = 0; q < RM_WPL; ++q) {
    const int w = lane + 64 * q;
    cur[q] = w < words ? (bset ? bset[w] : 0xffffffffu) : 0u;
  }
  int ty = a.type[row];
  if (ty < 0 || ty > 2) ty = 0;
  const int ruled = ty == 0 ? a.types[0] : ty == 1 ? a.types[1] : a.types[2];
  const bool live = i < n && a.state[col + i] != RM_INVALID && ruled != 0;
  if (live) {
    const float px = a.pos[2 * (col + i)], py = a.pos[2 * (col + i) + 1], ph = a.head[col + i];
    const float ci = cosf(ph), si = sinf(ph);
    const float hla = 0.5f * a.shape[3 * (size_t)row], hwa = 0.5f * a.shape[3 * (size_t)row + 1];
    const float ra = sqrtf(hla * hla + hwa * hwa);
    const float reach = ra + a.end_pose[(size_t)3 * a.token_size * 4 + ty];
    const float4* pose = reinterpret_cast<const float4*>(a.end_pose) + (size_t)ty * a.token_size;
    const float4* path = reinterpret_cast<const float4*>(a.paths) + (size_t)ty * a.token_size;
    const int ms = s / a.copies;
    const int nr = min(max(a.n_records[ms], 0), a.rec_cap);
    const float4* rec = reinterpret_cast<const float4*>(a.records) + (size_t)ms * a.rec_cap * 2;
    const float hwo = a.margin;                                                // the obstacle rectangle's half width
    int m = 0;
    for (int j0 = 0; j0 < nr; j0 += 64) {
      const int j = j0 + lane;
      bool in = false;
      float ox = 0.f, oy = 0.f, oc = 1.0f, os = 0.f, hlo = 0.f, orad = 0.f;
      if (j < nr) {
        const float4 r0 = rec[2 * j], r1 = rec[2 * j + 1];
        const float rx = (r0.x - px) + r0.z, ry = (r0.y - py) + r0.w;
        hlo = r1.z + a.margin;
        orad = sqrtf(hlo * hlo + hwo * hwo);
        const float lim = reach + orad;
        in = r1.w >= 0.f && rx * rx + ry * ry <= lim * lim;
        if (in) {
          ox = rx * ci + ry * si; oy = ry * ci - rx * si;
          oc = r1.x * ci + r1.y * si; os = r1.y * ci - r1.x * si;
          // astride the row's current box (the identity pose of its own frame): not an obstacle of this row in this step
          in = !(sat_sep(ox, oy, 1.0f, 0.f, hla, hwa, oc, os, hlo, hwo) < 0.f);
        }
      }
      unsigned long long bal = __ballot(in);
      while (bal) {                                                             // (uniform: at most two rounds per 64 records)
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        const bool put = in && ((bal >> lane) & 1ull) && m + before < RM_LIST;
        if (put) {
          list_a[m + before] = make_float4(ox, oy, oc, os);
          list_b[m + before] = make_float4(hlo, hwo, orad, 0.f);
        }
        const unsigned long long done = __ballot(put);
        m += (int)__popcll(done);
        bal &= ~done;
        if (bal) {                                                              // the list is full: a pass over the tokens, then go on
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int q = 0; q < RM_WPL; ++q)
            if (cur[q]) cur[q] = road_word(cur[q], pose + 32 * (lane + 64 * q), path + 32 * (lane + 64 * q), list_a, list_b, m, hla, hwa, ra, a.sweep);
          __builtin_amdgcn_wave_barrier();
          m = 0;
        }
      }
    }
    if (m > 0) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < RM_WPL; ++q)
        if (cur[q]) cur[q] = road_word(cur[q], pose + 32 * (lane + 64 * q), path + 32 * (lane + 64 * q), list_a, list_b, m, hla, hwa, ra, a.sweep);
    }
  }
  // the fallback's "any token left?" and the count: wave reductions over the words
  unsigned any = 0u;
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < RM_WPL; ++q) { any |= cur[q]; cnt += __popc(cur[q]); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { any |= __shfl_xor(any, off, 64); cnt += __shfl_xor(cnt, off, 64); }
  if (a.out_count && lane == 0) a.out_count[row] = cnt;
  const bool fallback = any == 0u;      // (every token left the road: the row keeps base(i))
#pragma unroll
  for (int q = 0; q < RM_WPL; ++q) {
    const int w = lane + 64 * q;
    if (w < words) out[w] = fallback ? (bset ? bset[w] : 0xffffffffu) : cur[q];
  }
}

}  // namespace ig
