// What the kernels that ride on a decode step share: k_collision_mask, k_road_mask (the row skeleton of a mask kernel) and
// k_step_score (the road-record entry).  DESIGN 5.12 to 5.14.
//
// A mask kernel gives one wave to a row.  The wave
//   1. loads the row's base words (lane l owns the 32-token words l, l + 64 of the set) and its box: base_words, row_box;
//   2. walks its obstacle source 64 at a time - the kernel's own part - and hands every lane's candidate entry, already moved into
//      the ROW's frame (translated by pos[c][i] first, then rotated by -head[c][i]: magnitudes stay at tens of metres wherever the
//      scene lies), to list_put, which compacts them - ballot + popcount - into the wave's LDS list of RIDER_LIST entries of two
//      float4; a full list takes a pass over the tokens and starts again;
//   3. token_pass: for each of a word's tokens still allowed a circle reject, then the separating-axis test (sat.cuh), of the end box
//      and (road masks with sweep) the path rectangle against the list; the word is assembled in a register.  A row with an empty
//      list never reads a token;
//   4. row_store: the fallback's "any token left?" is a wave reduction of the words' OR, the count one of their popcounts; one store
//      per word.
// fp32 throughout, no fused multiply-add (the build's -ffp-contract=off): the order of the operations is part of the results' bits.
#pragma once
#include "kernels.h"
#include "sat.cuh"

namespace ig {

constexpr int INVALID = 0;              // valid_state_type id of 'invalid' (edge_kernels.hip)

__device__ __forceinline__ int clamp_type(int ty) { return ty < 0 || ty > 2 ? 0 : ty; }
// types[ty] of an argument struct, without indexing it
__device__ __forceinline__ int type_ruled(const int (&types)[3], int ty) { return ty == 0 ? types[0] : ty == 1 ? types[1] : types[2]; }

// the rows of scene s that are in the scene during this step: rows >= first_new[s] were appended inside it
__device__ __forceinline__ int scene_rows(const int* n_agents, const int* first_new, int s, int A_cap) {
  int n = n_agents[s];
  if (first_new) n = min(n, first_new[s]);
  return min(n, A_cap);
}

// the lane's words of the row's static set; returns the set (nullptr: every token)
__device__ __forceinline__ const unsigned* base_words(unsigned (&cur)[RIDER_WPL], const TokenMaskCtl& base, int row, int words, int lane) {
  const unsigned* bset = base.bits ? token_mask_set(base, row, words) : nullptr;
#pragma unroll
  for (int q = 0; q < RIDER_WPL; ++q) {
    const int w = lane + 64 * q;
    cur[q] = w < words ? (bset ? bset[w] : 0xffffffffu) : 0u;
  }
  return bset;
}

// row i of column `col` (row = s * A_cap + i, of type ty): world position, cos / sin of the heading, half extents, enclosing radius,
// the distance its tokens can reach at all and the type's end poses
struct RowBox { float px, py, ci, si, hla, hwa, ra, reach; const float4* pose; };
__device__ __forceinline__ RowBox row_box(const float* pos, const float* head, const float* shape, const float* end_pose, int token_size,
                                          size_t col, int row, int i, int ty) {
  RowBox b;
  b.px = pos[2 * (col + i)]; b.py = pos[2 * (col + i) + 1];
  const float ph = head[col + i];
  b.ci = cosf(ph); b.si = sinf(ph);
  b.hla = 0.5f * shape[3 * (size_t)row]; b.hwa = 0.5f * shape[3 * (size_t)row + 1];
  b.ra = sqrtf(b.hla * b.hla + b.hwa * b.hwa);
  b.reach = b.ra + end_pose[(size_t)3 * token_size * 4 + ty];
  b.pose = reinterpret_cast<const float4*>(end_pose) + (size_t)ty * token_size;
  return b;
}

// the tokens first .. first + 31 of word `cur` (bits still allowed) of the row against the n list entries of the wave: returns the
// word without the tokens that hit one.  SWEEP: the path rectangle of path[] is tested too where `sweep` is set
template <bool SWEEP>
__device__ __forceinline__ unsigned word_pass(unsigned cur, int first, const RowBox& r, const float4* __restrict__ path, const float4* la,
                                              const float4* lb, int n, int sweep) {
  unsigned out = cur;
  for (int b = 0; b < 32; ++b) {
    if (!((cur >> b) & 1u)) continue;
    const float4 p = r.pose[first + b];                                        // dx, dy, cos, sin of the end box in the row's frame
    float4 w = make_float4(1.0f, 0.f, 0.f, 0.f);
    if constexpr (SWEEP)
      if (sweep) w = path[first + b];                                          // cos, sin, half length of the path rectangle
    const bool swept = w.z > 0.f;
    const float mx = 0.5f * p.x, my = 0.5f * p.y, rp = w.z + r.hwa;            // its centre and a radius that encloses it
    bool hit = false;
    for (int e = 0; e < n && !hit; ++e) {
      const float4 o = la[e];                                                  // centre, cos, sin of the obstacle in the row's frame
      const float4 q = lb[e];                                                  // half length, half width, radius
      const float ddx = o.x - p.x, ddy = o.y - p.y;
      const float rr = r.ra + q.z;
      if (ddx * ddx + ddy * ddy <= rr * rr) hit = sat_sep(ddx, ddy, p.z, p.w, r.hla, r.hwa, o.z, o.w, q.x, q.y) < 0.f;
      if constexpr (SWEEP)
        if (!hit && swept) {
          const float ex = o.x - mx, ey = o.y - my;
          const float rs = rp + q.z;
          if (ex * ex + ey * ey <= rs * rs) hit = sat_sep(ex, ey, w.x, w.y, w.z, r.hwa, o.z, o.w, q.x, q.y) < 0.f;
        }
    }
    if (hit) out &= ~(1u << b);
  }
  return out;
}

// one pass of the lane's words over the m list entries
template <bool SWEEP>
__device__ __forceinline__ void token_pass(unsigned (&cur)[RIDER_WPL], int lane, const RowBox& r, const float4* path, const float4* la,
                                           const float4* lb, int m, int sweep) {
#pragma unroll
  for (int q = 0; q < RIDER_WPL; ++q)
    if (cur[q]) cur[q] = word_pass<SWEEP>(cur[q], 32 * (lane + 64 * q), r, path, la, lb, m, sweep);
}

// the wave's lanes with `in` set append their entry (ea, eb) to the list of m entries; pass(m) runs token_pass when the list is full
template <class Pass>
__device__ __forceinline__ void list_put(bool in, float4 ea, float4 eb, float4* list_a, float4* list_b, int& m, int lane, Pass pass) {
  unsigned long long bal = __ballot(in);
  while (bal) {                                                                // (uniform: at most two rounds per 64 candidates)
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    const bool put = in && ((bal >> lane) & 1ull) && m + before < RIDER_LIST;
    if (put) { list_a[m + before] = ea; list_b[m + before] = eb; }
    const unsigned long long done = __ballot(put);
    m += (int)__popcll(done);
    bal &= ~done;
    if (bal) {                                                                 // the list is full: a pass over the tokens, then go on
      __builtin_amdgcn_wave_barrier();
      pass(m);
      __builtin_amdgcn_wave_barrier();
      m = 0;
    }
  }
}

// the row's set leaves: cur, or base(i) when no token is left (the fallback); out_count (optional): the size before the fallback
__device__ __forceinline__ void row_store(const unsigned (&cur)[RIDER_WPL], const unsigned* bset, unsigned* out_bits, int* out_count, int row,
                                          int words, int lane) {
  unsigned any = 0u;
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < RIDER_WPL; ++q) { any |= cur[q]; cnt += __popc(cur[q]); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { any |= __shfl_xor(any, off, 64); cnt += __shfl_xor(cnt, off, 64); }
  if (out_count && lane == 0) out_count[row] = cnt;
  const bool fallback = any == 0u;
  unsigned* const out = out_bits + (size_t)row * words;
#pragma unroll
  for (int q = 0; q < RIDER_WPL; ++q) {
    const int w = lane + 64 * q;
    if (w < words) out[w] = fallback ? (bset ? bset[w] : 0xffffffffu) : cur[q];
  }
}

// a road record (r0 = anchor x, y, offset x, y; r1 = cos, sin, half length, radius) seen from a row at (px, py): its midpoint relative
// to the row - world coordinates enter through the exact difference (anchor - pos) only - and the half length and enclosing radius
// of its obstacle rectangle, whose half width is the margin
struct RoadRel { float rx, ry, hlo, orad; };
__device__ __forceinline__ RoadRel road_rel(float4 r0, float4 r1, float px, float py, float margin) {
  RoadRel e;
  e.rx = (r0.x - px) + r0.z; e.ry = (r0.y - py) + r0.w;
  e.hlo = r1.z + margin;
  e.orad = sqrtf(e.hlo * e.hlo + margin * margin);
  return e;
}
// ... rotated into the frame of the row (heading ci, si): `at` = midpoint, cos, sin there.  Returns the separating-axis value of the
// obstacle rectangle and the row's own box (the identity pose of that frame): < 0, the row is astride the record
__device__ __forceinline__ float road_own_sep(const RoadRel& e, float4 r1, float ci, float si, float hla, float hwa, float margin, float4* at) {
  *at = make_float4(e.rx * ci + e.ry * si, e.ry * ci - e.rx * si, r1.x * ci + r1.y * si, r1.y * ci - r1.x * si);
  return sat_sep(at->x, at->y, 1.0f, 0.f, hla, hwa, at->z, at->w, e.hlo, margin);
}

}  // namespace ig
