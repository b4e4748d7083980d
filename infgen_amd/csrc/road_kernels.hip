// Road-aware decoding (include/infgen_hip.h, "road masks"): the allowed-token sets of one decode step from the map's
// road-edge segments.
//
// k_road_records_map / k_road_records_seg   once per reload: the compacted table of segment records of every distinct scene, from the
//                         EDGE map tokens' vocabulary polylines or from explicit world-coordinate segments.
// k_road_paths            once per vocabulary: direction and half length of every token's end displacement (the path rectangle).
// k_road_mask             the row skeleton of rider.cuh, one wave per row.  Its own part is the obstacle source: the wave streams its map
//                         scene's records 64 at a time from global memory (two 16-byte loads per lane), keeps the ones the row can
//                         reach at all (midpoint distance <= own radius + the type's largest displacement + the obstacle's radius)
//                         and drops the straddled ones, whose obstacle rectangle overlaps the row's current box.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), plain vector stores.
#include "kernels.h"
#include "rider.cuh"

namespace ig {

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

__global__ __launch_bounds__(64 * RIDER_WAVES) void k_road_mask(RoadArgs a) {
  __shared__ float4 rm_lds[RIDER_WAVES * 2 * RIDER_LIST];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4* const list_a = rm_lds + wave * (2 * RIDER_LIST);
  float4* const list_b = list_a + RIDER_LIST;
  const long long row_at = (long long)blockIdx.x * RIDER_WAVES + wave;
  if (row_at >= (long long)a.S * a.A_cap) return;                              // (uniform per wave; the kernel has no workgroup barrier)
  const int row = (int)row_at, A_cap = a.A_cap, words = a.token_size >> 5;
  const int s = row / A_cap, i = row - s * A_cap;
  const int n = scene_rows(a.n_agents, a.first_new, s, A_cap);
  const size_t col = ((size_t)s * a.T + a.c) * A_cap;                          // row 0 of column c
    unsigned cur[RIDER_WPL];
  const unsigned* bset = base_words(cur, a.base, row, words, lane);
  const int ty = clamp_type(a.type[row]);
  if (i < n && a.state[col + i] != INVALID && type_ruled(a.types, ty) != 0) {
    const RowBox r = row_box(a.pos, a.head, a.shape, a.end_pose, a.token_size, col, row, i, ty);
    const float4* path = reinterpret_cast<const float4*>(a.paths) + (size_t)ty * a.token_size;
    auto pass = [&](int m) __attribute__((always_inline)) { token_pass<true>(cur, lane, r, path, list_a, list_b, m, a.sweep); };
    const int ms = s / a.copies;
    const int nr = min(max(a.n_records[ms], 0), a.rec_cap);
    const float4* rec = reinterpret_cast<const float4*>(a.records) + (size_t)ms * a.rec_cap * 2;
    int m = 0;
    for (int j0 = 0; j0 < nr; j0 += 64) {
      const int j = j0 + lane;
      bool in = false;
      float4 ea = make_float4(0.f, 0.f, 1.0f, 0.f), eb = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < nr) {
        const float4 r0 = rec[2 * j], r1 = rec[2 * j + 1];
        const RoadRel e = road_rel(r0, r1, r.px, r.py, a.margin);
        const float lim = r.reach + e.orad;
        in = r1.w >= 0.f && e.rx * e.rx + e.ry * e.ry <= lim * lim;
        // astride the row's current box: not an obstacle of this row in this step
        if (in) in = !(road_own_sep(e, r1, r.ci, r.si, r.hla, r.hwa, a.margin, &ea) < 0.f);
        eb = make_float4(e.hlo, a.margin, e.orad, 0.f);
      }
      list_put(in, ea, eb, list_a, list_b, m, lane, pass);
    }
    if (m > 0) {
      __builtin_amdgcn_wave_barrier();
      pass(m);
    }
  }
  row_store(cur, bset, a.out_bits, a.out_count, row, words, lane);
}

}  // namespace ig
