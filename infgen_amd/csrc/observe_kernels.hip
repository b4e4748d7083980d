// Observations (include/infgen_hip.h, "observations"): what a controller reads per commanded row - the row's own
// features, its K nearest live agents and its Km nearest map tokens, all in the row's own frame - in one launch with no host read.
//
// k_observe_rows          one wave per observed row, OB_WAVES rows per workgroup:
//   0. the row named by obs_row[n] (or n itself), its scene slot and whether it is live; a row that is not gets zeros, -1 and 0;
//   1. lane 0 writes the row's own eight features (two 16-byte stores);
//   2. the neighbour scan: lane l looks at rows l, l + 64, ... of the slot.  d2 is formed from the stored coordinates
//      (pos[j] - pos[i], squared and summed in fp32), the candidates inside the radius are counted (ballot + popcount) and their
//      64-bit keys (bits of d2) << 32 | j compacted into the wave's LDS list - d2 >= 0, so its bits order as an unsigned integer and
//      the key carries the tie rule;
//   3. select_k: K rounds of a wave arg-min over the lanes' running best of their list slots; the lane that owned the winner blanks
//      its slot and looks at its slots again; lane r keeps the r-th key.  A list that could overflow at the next 64 candidates is
//      first cut down to its K best in the same way (they become its head), so any number of candidates goes through OB_LIST slots;
//   4. lane r recomputes entry r's features from the stored values and writes them (8-byte stores); lanes found .. K - 1 write the
//      unused entries;
//   5. the map scan, selection and write: the same three steps over map scene s / copies.
// The map's positions are read from global memory by every row - rows of one workgroup need not share a scene (obs_row names any
// rows; an ego-only session observes one row per scene), so there is nothing to stage per workgroup; a scene's positions (8 bytes a
// token) stay in L2 for the rows that follow.
// No atomics, every output entry has one writer, no reduction depends on an order.  fp32 throughout, no fused multiply-add (the
// build's -ffp-contract=off).
#include "kernels.h"
#include "rider.cuh"

namespace ig {

constexpr unsigned long long OB_NONE = ~0ull;               // no key: the bits of d2 would be a NaN's, and a NaN is never inside a radius

__device__ __forceinline__ float observe_wrap(float a) {    // wrap to [-pi, pi) of a heading difference (the step scores', signed)
  const float PI_F = 3.14159274f, TWO_PI_F = 6.28318548f;
  float r = fmodf(a + PI_F, TWO_PI_F);
  if (r < 0.f) r += TWO_PI_F;
  return r - PI_F;
}

// the wave's writes to its list are seen by its later reads: the LDS serves a wave's accesses in order, this keeps the compiler to it
__device__ __forceinline__ void observe_list_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long observe_wave_min(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// the k smallest keys of list[0 .. m): lane r returns the r-th (OB_NONE beyond `found`).  The list's selected slots are blanked.
__device__ __forceinline__ unsigned long long select_k(unsigned long long* list, int m, int k, int lane, int& found) {
  unsigned long long best = OB_NONE, sel = OB_NONE;
  int slot = 0;
  for (int q = lane; q < m; q += 64) {
    const unsigned long long key = list[q];
    if (key < best) { best = key; slot = q; }
  }
  found = 0;
  for (int r = 0; r < k; ++r) {                                                  // (uniform: the minimum is the wave's)
    const unsigned long long w = observe_wave_min(best);
    if (w == OB_NONE) break;
    if (lane == r) sel = w;
    if (best == w) {                                                             // keys are distinct: one lane
      list[slot] = OB_NONE;
      best = OB_NONE;
      for (int q = lane; q < m; q += 64) {
        const unsigned long long key = list[q];
        if (key < best) { best = key; slot = q; }
      }
    }
    ++found;
  }
  return sel;
}

// the lanes with `in` set append their key to the list of m entries; the caller has made room for 64
__device__ __forceinline__ void observe_put(bool in, unsigned long long key, unsigned long long* list, int& m, int& count, int lane) {
  const unsigned long long bal = __ballot(in);
  if (in) list[m + __popcll(bal & ((1ull << lane) - 1ull))] = key;
  const int n = (int)__popcll(bal);
  m += n;
  count += n;
}

// room for the next 64 candidates: a list that could overflow keeps its k best
__device__ __forceinline__ void observe_room(unsigned long long* list, int& m, int k, int lane) {
  if (m + 64 <= OB_LIST) return;                                                 // (uniform)
  observe_list_sync();
  int found;
  const unsigned long long sel = select_k(list, m, k, lane, found);
  observe_list_sync();
  if (lane < found) list[lane] = sel;
  m = found;
}

__device__ __forceinline__ void store_f2(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }

__global__ __launch_bounds__(64 * OB_WAVES) void k_observe_rows(ObserveArgs a) {
  __shared__ unsigned long long lists[OB_WAVES][OB_LIST];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * OB_WAVES + wave;
  if (n >= a.N) return;                                                          // (uniform per wave; no workgroup barrier below)
  unsigned long long* const list = lists[wave];
  const int A_cap = a.A_cap, c = a.c, K = a.K, Km = a.Km;
  const long long rows = (long long)a.S * A_cap;

  // 0. the row, its slot, live or not
  const int row = a.obs_row ? a.obs_row[n] : n;
  const bool in_range = row >= 0 && row < rows;
  const int s = in_range ? row / A_cap : 0, i = in_range ? row - s * A_cap : 0;
  const int na = scene_rows(a.n_agents, nullptr, s, A_cap);
  const size_t col = ((size_t)s * a.T + c) * A_cap;                              // row 0 of column c
  const size_t prev = col - (c >= 1 ? A_cap : 0);                                // ... of column c - 1 (read only when c >= 1)
  const bool live = in_range && i < na && a.state[col + i] != INVALID;

  float* const nf = a.nbr_feat + (size_t)n * K * OBS_NBR;
  float* const mf = a.map_feat + (size_t)n * Km * OBS_MAP;
  if (!live) {                                                                   // (uniform)
    if (lane < OBS_SELF) a.self_feat[(size_t)n * OBS_SELF + lane] = 0.f;
    if (lane < K) {
#pragma unroll
      for (int f = 0; f < OBS_NBR; f += 2) store_f2(nf + lane * OBS_NBR + f, 0.f, 0.f);
      a.nbr_index[(size_t)n * K + lane] = -1;
    }
    if (lane < Km) {
#pragma unroll
      for (int f = 0; f < OBS_MAP; f += 2) store_f2(mf + lane * OBS_MAP + f, 0.f, 0.f);
      a.map_index[(size_t)n * Km + lane] = -1;
    }
    if (lane == 0) {
      if (a.nbr_count) a.nbr_count[n] = 0;
      if (a.map_count) a.map_count[n] = 0;
    }
    return;
  }

  const float px = a.pos[2 * (col + i)], py = a.pos[2 * (col + i) + 1], ph = a.head[col + i];
  const float ci = cosf(ph), si = sinf(ph);
  const float dt = a.dt;
  const bool has_prev = c >= 1;                                                  // column c - 1 exists

  // 1. the row's own features
  if (lane == 0) {
    float vx = 0.f, vy = 0.f, yaw = 0.f, hp = 0.f;
    if (has_prev && a.state[prev + i] != INVALID) {
      const float ux = (px - a.pos[2 * (prev + i)]) / dt, uy = (py - a.pos[2 * (prev + i) + 1]) / dt;
      vx = ux * ci + uy * si; vy = uy * ci - ux * si;
      yaw = observe_wrap(ph - a.head[prev + i]) / dt;
      hp = 1.0f;
    }
    float4* const out = reinterpret_cast<float4*>(a.self_feat + (size_t)n * OBS_SELF);
    out[0] = make_float4(1.0f, vx, vy, yaw);
    out[1] = make_float4(a.shape[3 * (size_t)row], a.shape[3 * (size_t)row + 1], (float)clamp_type(a.type[row]), hp);
  }

  // 2. - 4. the neighbours
  if (a.nbr_count) {                                                             // (uniform)
    const float r2 = a.radius * a.radius;
    int m = 0, count = 0;
    for (int base = 0; base < na; base += 64) {
      observe_room(list, m, K, lane);
      const int j = base + lane;
      bool in = j < na && j != i && a.state[col + j] != INVALID;
      unsigned long long key = OB_NONE;
      if (in) {
        const float dx = a.pos[2 * (col + j)] - px, dy = a.pos[2 * (col + j) + 1] - py;
        const float d2 = dx * dx + dy * dy;
        in = d2 <= r2;
        key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j;
      }
      observe_put(in, key, list, m, count, lane);
    }
    if (lane == 0) a.nbr_count[n] = count;
    if (K > 0) {                                                                 // (uniform)
      observe_list_sync();
      int found;
      const unsigned long long sel = select_k(list, m, K, lane, found);
      observe_list_sync();                                                       // (the map scan writes the list next)
      if (lane < K) {
        float* const o = nf + lane * OBS_NBR;
        if (lane < found) {
          const int j = (int)(unsigned)sel;
          const size_t rj = (size_t)s * A_cap + j;
          const float xj = a.pos[2 * (col + j)], yj = a.pos[2 * (col + j) + 1];
          const float dx = xj - px, dy = yj - py;
          const float hj = a.head[col + j];
          const float cj = cosf(hj), sj = sinf(hj);
          float vx = 0.f, vy = 0.f;
          if (has_prev && a.state[prev + j] != INVALID) {
            const float ux = (xj - a.pos[2 * (prev + j)]) / dt, uy = (yj - a.pos[2 * (prev + j) + 1]) / dt;
            vx = ux * ci + uy * si; vy = uy * ci - ux * si;
          }
          store_f2(o, dx * ci + dy * si, dy * ci - dx * si);
          store_f2(o + 2, cj * ci + sj * si, sj * ci - cj * si);
          store_f2(o + 4, vx, vy);
          store_f2(o + 6, a.shape[3 * rj], a.shape[3 * rj + 1]);
          store_f2(o + 8, (float)clamp_type(a.type[rj]), 1.0f);
          a.nbr_index[(size_t)n * K + lane] = j;
        } else {
#pragma unroll
          for (int f = 0; f < OBS_NBR; f += 2) store_f2(o + f, 0.f, 0.f);
          a.nbr_index[(size_t)n * K + lane] = -1;
        }
      }
    }
  }

  // 5. the map tokens of map scene s / copies
  if (a.map_count) {                                                             // (uniform)
    const int ms = s / a.copies;
    const int nm = a.map_pos ? min(max(a.n_map[ms], 0), a.M_cap) : 0;
    const size_t mbase = (size_t)ms * a.M_cap;
    const float r2 = a.map_radius * a.map_radius;
    int m = 0, count = 0;
    for (int base = 0; base < nm; base += 64) {
      observe_room(list, m, Km, lane);
      const int t = base + lane;
      bool in = t < nm;
      unsigned long long key = OB_NONE;
      if (in) {
        const float dx = a.map_pos[2 * (mbase + t)] - px, dy = a.map_pos[2 * (mbase + t) + 1] - py;
        const float d2 = dx * dx + dy * dy;
        in = d2 <= r2;
        key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)t;
      }
      observe_put(in, key, list, m, count, lane);
    }
    if (lane == 0) a.map_count[n] = count;
    if (Km > 0) {                                                                // (uniform)
      observe_list_sync();
      int found;
      const unsigned long long sel = select_k(list, m, Km, lane, found);
      if (lane < Km) {
        float* const o = mf + lane * OBS_MAP;
        if (lane < found) {
          const int t = (int)(unsigned)sel;
          const float dx = a.map_pos[2 * (mbase + t)] - px, dy = a.map_pos[2 * (mbase + t) + 1] - py;
          const float ho = a.map_orient[mbase + t];
          const float cm = cosf(ho), sm = sinf(ho);
          store_f2(o, dx * ci + dy * si, dy * ci - dx * si);
          store_f2(o + 2, cm * ci + sm * si, sm * ci - cm * si);
          store_f2(o + 4, (float)a.map_type[mbase + t], 1.0f);
          a.map_index[(size_t)n * Km + lane] = t;
        } else {
#pragma unroll
          for (int f = 0; f < OBS_MAP; f += 2) store_f2(o + f, 0.f, 0.f);
          a.map_index[(size_t)n * Km + lane] = -1;
        }
      }
    }
  }
}

}  // namespace ig
