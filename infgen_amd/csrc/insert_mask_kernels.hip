// Insertion rules (include/infgen_hip.h, "insertion rules"): the allowed cells of scenario insertion for one column.
//
// k_insert_cell_mask   one workgroup of 256 threads per scene.  Lane l of wave w takes cell 64 * (w + 4 * i) + l in round i, so a
//                      wave holds 64 consecutive cells; a thread keeps one verdict bit per round in a register.  Each rule stages its
//                      obstacles - the scene's boxes, road records, map tokens, zones - in the ego frame of the column, IM_TILE entries
//                      of IM_F floats at a time in LDS (24 KB), and every lane walks the tile for each of its cells: all lanes read the
//                      same LDS address (a broadcast, no bank conflict).  The verdicts of a wave are packed by __ballot into two 32-bit
//                      words that lane 0 writes with one 8-byte vector store.  Counts are sums of population counts: integers, the
//                      result is bitwise reproducible.  No atomics, no scratch.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off), plain vector stores.
#include "kernels.h"

namespace ig {

static_assert(IM_TILE == MAX_SCENE_AGENTS, "the clearance rule stages a scene's boxes once");
constexpr int IM_INVALID = 0;

// a world difference (dx, dy) in the ego frame: the inverse of decode_pos' rotation by phi = ego heading - pi / 2
__device__ __forceinline__ float2 im_rot(float dx, float dy, float cs, float sn) {
  return make_float2(dx * cs + dy * sn, dy * cs - dx * sn);
}

__global__ __launch_bounds__(IM_NT) void k_insert_cell_mask(InsertCellMaskArgs a) {
  __shared__ float tile[IM_TILE * IM_F];
  __shared__ int red[8];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ms = s / a.copies;
  const int nchunk = a.W >> 1;                               // 64-cell chunks (W is a multiple of 4 words)
  const size_t col = ((size_t)s * a.T + a.c) * a.A_cap;
  const int av = min(max(a.av_index[s], 0), a.A_cap - 1);
  const float ex = a.pos[2 * (col + av)], ey = a.pos[2 * (col + av) + 1], eh = a.head[col + av];
  const float phi = eh - HALF_PI_F;
  const float cs = cosf(phi), sn = sinf(phi);
  unsigned ban = 0;                                          // bit i: the cell of round i is banned by a static rule

  if (a.static_pass != 2) {
    if (a.rules & IM_KEEPOUT) {
      for (int i = 0; w + 4 * i < nchunk; ++i) {
        const int g = 64 * (w + 4 * i) + lane;
        if (g < a.G) {
          const float gx = a.grid_xy[2 * g], gy = a.grid_xy[2 * g + 1];
          if (-a.ko_back <= gy && gy <= a.ko_front && fabsf(gx) <= a.ko_half) ban |= 1u << i;
        }
      }
    }
    if (a.rules & IM_EDGES) {
      const int n = min(max(a.n_records[ms], 0), a.rec_cap);
      const float* rec = a.records + (size_t)ms * a.rec_cap * RM_REC;
      for (int r0 = 0; r0 < n; r0 += IM_TILE) {
        const int nt = min(n - r0, IM_TILE);
        __syncthreads();
        for (int k = tid; k < nt; k += IM_NT) {
          const float4 p0 = *reinterpret_cast<const float4*>(rec + (size_t)(r0 + k) * RM_REC);
          const float4 p1 = *reinterpret_cast<const float4*>(rec + (size_t)(r0 + k) * RM_REC + 4);
          const float2 m = im_rot((p0.x - ex) + p0.z, (p0.y - ey) + p0.w, cs, sn);
          const float2 u = im_rot(p1.x, p1.y, cs, sn);
          float* t = tile + k * IM_F;
          t[0] = m.x; t[1] = m.y; t[2] = u.x; t[3] = u.y; t[4] = p1.w < 0.f ? -1.0f : p1.z;
        }
        __syncthreads();
        for (int i = 0; w + 4 * i < nchunk; ++i) {
          const int g = 64 * (w + 4 * i) + lane;
          if (g >= a.G) continue;
          const float gx = a.grid_xy[2 * g], gy = a.grid_xy[2 * g + 1];
          bool hit = false;
          for (int k = 0; k < nt; ++k) {
            const float* t = tile + k * IM_F;
            const float hl = t[4];
            if (hl < 0.f) continue;
            const float dx = gx - t[0], dy = gy - t[1];
            const float al = dx * t[2] + dy * t[3], ac = dy * t[2] - dx * t[3];
            const float ox = fmaxf(fabsf(al) - hl, 0.f);
            hit = hit || sqrtf(ox * ox + ac * ac) < a.edge_clearance;
          }
          if (hit) ban |= 1u << i;
        }
      }
    }
    if (a.rules & IM_LANES) {
      const int n = min(max(a.n_map[ms], 0), a.M_cap);
      const float d2max = a.lane_dist * a.lane_dist;
      unsigned near = 0;
      for (int m0 = 0; m0 < n; m0 += IM_TILE) {
        const int nt = min(n - m0, IM_TILE);
        __syncthreads();
        for (int k = tid; k < nt; k += IM_NT) {
          const size_t at = (size_t)ms * a.M_cap + m0 + k;
          const long long ty = a.map_type[at];
          const bool lane_ty = ty >= 0 && ty < 32 && ((a.lane_types >> (int)ty) & 1u);
          const float2 q = im_rot(a.map_pos[2 * at] - ex, a.map_pos[2 * at + 1] - ey, cs, sn);
          float* t = tile + k * IM_F;
          t[0] = q.x; t[1] = q.y; t[2] = lane_ty ? 1.0f : 0.f;
        }
        __syncthreads();
        for (int i = 0; w + 4 * i < nchunk; ++i) {
          const int g = 64 * (w + 4 * i) + lane;
          if (g >= a.G) continue;
          const float gx = a.grid_xy[2 * g], gy = a.grid_xy[2 * g + 1];
          bool hit = false;
          for (int k = 0; k < nt; ++k) {
            const float* t = tile + k * IM_F;
            const float dx = gx - t[0], dy = gy - t[1];
            hit = hit || (t[2] != 0.f && dx * dx + dy * dy <= d2max);
          }
          if (hit) near |= 1u << i;
        }
      }
      ban |= ~near;
    }
    if (a.rules & IM_ZONES) {
      const int n = min(max(a.n_zones[ms], 0), a.Z);
      const float* zn = a.zones + (size_t)ms * a.Z * 4;
      unsigned inside = 0;
      bool any_allow = false;
      for (int z0 = 0; z0 < n; z0 += IM_TILE) {
        const int nt = min(n - z0, IM_TILE);
        __syncthreads();
        for (int k = tid; k < nt; k += IM_NT) {
          const float4 z = *reinterpret_cast<const float4*>(zn + (size_t)(z0 + k) * 4);
          const float2 q = im_rot(z.x - ex, z.y - ey, cs, sn);
          const bool live = z.z > 0.f && z.z < __builtin_inff() && (z.w == 0.f || z.w == 1.0f);
          float* t = tile + k * IM_F;
          t[0] = q.x; t[1] = q.y; t[2] = z.z * z.z; t[3] = live ? z.w : -1.0f;
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k) any_allow = any_allow || tile[k * IM_F + 3] == 1.0f;
        for (int i = 0; w + 4 * i < nchunk; ++i) {
          const int g = 64 * (w + 4 * i) + lane;
          if (g >= a.G) continue;
          const float gx = a.grid_xy[2 * g], gy = a.grid_xy[2 * g + 1];
          for (int k = 0; k < nt; ++k) {
            const float* t = tile + k * IM_F;
            const float dx = gx - t[0], dy = gy - t[1];
            if (t[3] >= 0.f && dx * dx + dy * dy <= t[2]) {
              if (t[3] == 0.f) ban |= 1u << i;
              else inside |= 1u << i;
            }
          }
        }
      }
      if (any_allow) ban |= ~inside;
    }
  } else {
    const unsigned* sb = a.static_bits + (size_t)s * a.W;
    for (int i = 0; w + 4 * i < nchunk; ++i) {
      const int g = 64 * (w + 4 * i) + lane;
      if (!((sb[g >> 5] >> (g & 31)) & 1u)) ban |= 1u << i;
    }
  }
  if (a.static_pass == 1) {
    unsigned* sb = a.static_bits + (size_t)s * a.W;
    for (int i = 0; w + 4 * i < nchunk; ++i) {
      const int chunk = w + 4 * i, g = 64 * chunk + lane;
      const unsigned long long bal = __ballot(g < a.G && !((ban >> i) & 1u));
      if (lane == 0) *reinterpret_cast<uint2*>(sb + 2 * chunk) = make_uint2((unsigned)bal, (unsigned)(bal >> 32));
    }
  }

  // the scene's boxes at column c in the ego frame, staged once: centre, heading direction, half length, half width (-1: not in the scene)
  const int nA = min(max(a.n_agents[s], 0), a.A_cap);
  int live = 0;                                              // wave-uniform: the rows of this wave's staging rounds
  __syncthreads();
  for (int j0 = 0; j0 < nA; j0 += IM_NT) {
    const int j = j0 + tid;
    const bool in_scene = j < nA && a.state[col + j] != IM_INVALID;
    live += (int)__popcll(__ballot(in_scene));
    if (j < nA && (a.rules & IM_CLEARANCE)) {
      float* t = tile + j * IM_F;
      if (in_scene) {
        const float2 q = im_rot(a.pos[2 * (col + j)] - ex, a.pos[2 * (col + j) + 1] - ey, cs, sn);
        const float hj = a.head[col + j];
        const float2 u = im_rot(cosf(hj), sinf(hj), cs, sn);
        const float* sh = a.shape + 3 * ((size_t)s * a.A_cap + j);
        t[0] = q.x; t[1] = q.y; t[2] = u.x; t[3] = u.y; t[4] = fmaxf(0.5f * sh[0], 0.f); t[5] = fmaxf(0.5f * sh[1], 0.f);
      } else {
        t[4] = -1.0f;
      }
    }
  }
  __syncthreads();
  int count = 0;                                             // wave-uniform: allowed cells of this wave's chunks
  unsigned* out = a.allowed + (size_t)s * a.W;
  for (int i = 0; w + 4 * i < nchunk; ++i) {
    const int chunk = w + 4 * i, g = 64 * chunk + lane;
    bool ok = g < a.G && !((ban >> i) & 1u);
    if (ok && (a.rules & IM_CLEARANCE)) {
      const float gx = a.grid_xy[2 * g], gy = a.grid_xy[2 * g + 1];
      for (int j = 0; j < nA; ++j) {
        const float* t = tile + j * IM_F;
        const float hl = t[4], hw = t[5];
        if (hl < 0.f) continue;
        const float dx = gx - t[0], dy = gy - t[1];
        const float rr = (hl + hw) + a.clearance;            // the circle test: no point of the box is farther than hl + hw from its centre
        if (dx * dx + dy * dy >= rr * rr) continue;
        const float lx = dx * t[2] + dy * t[3], ly = dy * t[2] - dx * t[3];
        const float ox = fmaxf(fabsf(lx) - hl, 0.f), oy = fmaxf(fabsf(ly) - hw, 0.f);
        if (sqrtf(ox * ox + oy * oy) < a.clearance) { ok = false; break; }
      }
    }
    const unsigned long long bal = __ballot(ok);
    count += (int)__popcll(bal);
    if (lane == 0) *reinterpret_cast<uint2*>(out + 2 * chunk) = make_uint2((unsigned)bal, (unsigned)(bal >> 32));
  }
  if (lane == 0) { red[w] = count; red[4 + w] = live; }
  __syncthreads();
  if (tid == 0) {
    const int n = (red[0] + red[1]) + (red[2] + red[3]);
    a.allowed_count[s] = n;
    a.live[s] = (red[4] + red[5]) + (red[6] + red[7]);
    if (a.count_log) a.count_log[(size_t)s * a.count_stride] = n;
  }
}

}  // namespace ig
