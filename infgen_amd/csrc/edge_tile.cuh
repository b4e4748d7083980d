// The blocks around the per-edge arithmetic (edge_attn.cuh: EdgeAcc) that the fused edge-attention kernels share: k_edge_fused
// (edge_fused.hip), k_edge_fused3 (edge_fused3.hip: its edge loop is its own) and the sublayer of k_layers_p (layers_p.hip) do the
// same three things to a tile of 16 destination rows -
//   u-GEMM    u_h = q_h W'_kr,h       wave = head, K = 16, three-term fp16 split, -> the U tile in LDS
//   row loop  one wave per destination row over its edge list (EdgeAcc), then agg / z / sigma of the row -> LDS
//   z-GEMM    W'_vr,h z_h             wave = head, K = 32, static prescale; the caller adds agg and b'_h sigma_h
// - and rank the tile's rows by edge count first.  ONE copy of each lives here: a change to the split arithmetic, the packed rhat
// row format or the softmax finalisation is made once, and the kernels stay bit-identical to each other by construction
// (tests/test_ops_gpu.py::test_edge_fused_instantiations_give_the_same_bits).  The helpers only compute; WHERE a kernel requests its
// weight fragments relative to its barriers and its other loads is that kernel's decision and stays at its call sites.
#pragma once
#include "kernels.h"
#include "layout.h"
#include "tile.cuh"
#include "split.cuh"
#include "edge_attn.cuh"

namespace ig {

// XCD-aware tile order: consecutive workgroups go to consecutive XCDs (b % 8), each with its own L2.  With tps tiles per
// scene, workgroups b, b + 8, ..., b + 8 (tps - 1) - one XCD - take the tiles of ONE scene, so that the scene's K / V rows
// (agent set: read by every row of the scene) are fetched into one L2 instead of tps of them.
__device__ __forceinline__ int xcd_tile(int tile, int tiles_per_scene) {
  if (tiles_per_scene > 1) {
    const int tps = tiles_per_scene, grp = 8 * tps;
    const int bq = tile / grp, br = tile % grp;
    tile = bq * grp + (br % 8) * tps + br / 8;
  }
  return tile;
}

// Rank of row rl among the n rows of a tile by edge count, longest first (ties in row order: the ranks are a permutation of
// 0 .. n - 1); lane k < n holds row k's count in cnt.  Longest rows first: the agent set's lists run from a few to 60+ edges, and
// dealt in index order a long row that comes last is the tile's tail while the other waves wait at the barrier.  Only the ORDER in
// which rows are picked changes - every row is still summed edge by edge by one wave, results are bitwise the same.
// READLANE: the counts through v_readlane (no LDS round trip like __shfl; needs n <= 16 so that hipcc keeps the 16 scalars)
template <bool READLANE>
__device__ __forceinline__ int rank_by_count(int cnt, int rl, int n) {
  int rank = 0;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const int ck = READLANE ? __builtin_amdgcn_readlane(cnt, k) : __shfl(cnt, k, 64);
    rank += (ck > cnt || (ck == cnt && k < rl)) ? 1 : 0;
  }
  return rank;
}

// ---- weight fragments of the two GEMMs (A operands straight from L2): address + load only
// W'_kr of head h: `pre` = the pack's AH_PRE part, eight 16-column tiles, hi / lo
__device__ __forceinline__ void load_wkr(const unsigned short* pre, int h, int lane, v4h (&ah)[8], v4h (&al)[8]) {
  const unsigned short* Wk = pre + (size_t)(4 + (h >> 1)) * QUARTER + (size_t)((h & 1) * 8) * 2 * 256 + lane * 4;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    ah[ct] = *reinterpret_cast<const v4h*>(Wk + (ct * 2) * 256);
    al[ct] = *reinterpret_cast<const v4h*>(Wk + (ct * 2 + 1) * 256);
  }
}
// W'_vr of head h: `post` = the pack's AH_POST part, four k-steps, hi / lo
__device__ __forceinline__ void load_wvr(const unsigned short* post, int h, int lane, v8h (&wh)[4], v8h (&wl)[4]) {
  const unsigned short* Wv = post + (size_t)(h >> 1) * QUARTER + (size_t)((h & 1) * 4) * 2 * 512 + lane * 8;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    wh[s] = *reinterpret_cast<const v8h*>(Wv + (s * 2) * 512);
    wl[s] = *reinterpret_cast<const v8h*>(Wv + (s * 2 + 1) * 512);
  }
}

// the largest of the four lanes j, j + 16, j + 32, j + 48 (one row's 16 query values of a head): through __shfl_xor, or through the
// gfx950 row / half swaps (split.cuh)
struct MaxShfl {
  __device__ __forceinline__ float operator()(float m) const {
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    return fmaxf(m, __shfl_xor(m, 32, 64));
  }
};
struct MaxSwap {
  __device__ __forceinline__ float operator()(float m) const { return xor_lanes_max(m); }
};

// ---- u-GEMM: u_h = q_h W'_kr,h (K = 16: v_mfma_f32_16x16x16_f16; B fragment = the head's 16 query values of row j = lane & 15, this
// lane's four in q), three-term fp16 split like k_attn_h (split.cuh): per (row, head) power-of-two scale into the fp16 range, as
// frags_scaled does per row, products in the order hi hi, hi lo, lo hi.  hdr = the pack's header (hdr[1]: the u scale); urow = this lane's
// first float of the U row (row j, head h, column 4 (lane >> 4); the eight results are 16 columns apart)
template <class MAX4>
__device__ __forceinline__ void u_gemm(f32x4 q, const v4h (&ah)[8], const v4h (&al)[8], const float* hdr, float* urow, MAX4 max4) {
  float m = fmaxf(fmaxf(fabsf(q[0]), fabsf(q[1])), fmaxf(fabsf(q[2]), fabsf(q[3])));
  m = max4(m);
  unsigned ebits = __float_as_uint(m) >> 23;
  ebits = min(max(ebits, 15u), 253u);
  const float sc = __uint_as_float((268u - ebits) << 23), inv = __uint_as_float((ebits - 14u) << 23);
  u32x2 qh, ql;
  {
    unsigned hi, lo;
    split_pair(q[0] * sc, q[1] * sc, hi, lo); qh[0] = hi; ql[0] = lo;
    split_pair(q[2] * sc, q[3] * sc, hi, lo); qh[1] = hi; ql[1] = lo;
  }
  const v4h vqh = __builtin_bit_cast(v4h, qh), vql = __builtin_bit_cast(v4h, ql);
  const float cq = inv * hdr[1];
  f32x4 acc[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah[ct], vqh, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah[ct], vql, acc[ct], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(al[ct], vqh, acc[ct], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)
    *reinterpret_cast<float4*>(urow + 16 * ct) = make_float4(acc[ct][0] * cq, acc[ct][1] * cq, acc[ct][2] * cq, acc[ct][3] * cq);
}

// ---- z-GEMM: W'_vr,h z_h * c (k_attn_h's z-GEMM: |z| <= sqrt(127), static prescale 1024; c = the pack header's z scale, hdr[4]).
// zrow = this lane's first float of the Z row (row j, head h, column 8 (lane >> 4)); the caller adds agg and b'_h sigma_h (agg_out)
__device__ __forceinline__ f32x4 z_gemm(const float* zrow, const v8h (&wh)[4], const v8h (&wl)[4], float c) {
  const float zs = 1024.0f, zinv = c * (1.0f / 1024.0f);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float4 z0 = *reinterpret_cast<const float4*>(zrow + 32 * s);
    const float4 z1 = *reinterpret_cast<const float4*>(zrow + 32 * s + 4);
    u32x4 bh, bl;
    unsigned hi, lo;
    split_pair(z0.x * zs, z0.y * zs, hi, lo); bh[0] = hi; bl[0] = lo;
    split_pair(z0.z * zs, z0.w * zs, hi, lo); bh[1] = hi; bl[1] = lo;
    split_pair(z1.x * zs, z1.y * zs, hi, lo); bh[2] = hi; bl[2] = lo;
    split_pair(z1.z * zs, z1.w * zs, hi, lo); bh[3] = hi; bl[3] = lo;
    const v8h vbh = __builtin_bit_cast(v8h, bh), vbl = __builtin_bit_cast(v8h, bl);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], vbh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], vbl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[s], vbh, acc, 0, 0, 0);
  }
  f32x4 wz;
#pragma unroll
  for (int r = 0; r < 4; ++r) wz[r] = acc[r] * zinv;      // (four scalar products: a vector one becomes v_pk_mul_f32)
  return wz;
}
// agg' = agg + (W'_vr z + b' sigma), in this order
__device__ __forceinline__ f32x4 agg_out(f32x4 ag, f32x4 wz, f32x4 bvr, float sg) {
  f32x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = ag[r] + (wz[r] + bvr[r] * sg);
  return o;
}

// ---- row loads of the edge loop: lane l takes columns (2 l, 2 l + 1) of a 128-wide fp32 row
__device__ __forceinline__ pk2 ld8(const float* base, bool nt, int lane) {
  return ea_ld(reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + 8u * (unsigned)lane), nt);
}
// packed 24-bit rhat row e (kernels.h): this lane's two columns = one dword of the 16-bit plane + one short of the 8-bit plane
__device__ __forceinline__ pk2 ld_r24(const float* rhat, size_t e, int lane) {
  const char* rowp = reinterpret_cast<const char*>(rhat) + e * R24_ROW_BYTES;
  const unsigned hi = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(rowp + 4 * lane));
  const unsigned lo = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(rowp + R24_LO_PLANE + 2 * lane));
  return pk2{__uint_as_float((hi << 16) | ((lo & 0xffu) << 8)), __uint_as_float((hi & 0xffff0000u) | (lo & 0xff00u))};
}

// ---- the vector edge loop of one destination row: edges e_base .. e_base + E - 1 in list order into acc (q and u loaded, reset).
// sv = the source indices of the first (up to) 64 edges, one per lane (lists beyond 64 edges: the next chunk is loaded here).
// G edges per trip: all their K / V / rhat rows are requested at the top of the trip (index clamped at the end of the list: no
// branch around the loads, the waits are counted ones) and consumed in turn; nothing is carried in registers from trip to trip
// (edge_attn.cuh explains why), the trip's fill latency is hidden by the SIMD's other waves.  (A tail trip of exactly the
// remaining length was tried: same time on lists of any raggedness - the loop is bound by its gathers, DESIGN.md section 9 - and
// ten spilled registers.)  R24: rhat rows in the packed 24-bit format.
template <int G, bool R24>
__device__ __forceinline__ void edge_row_loop(EdgeAcc<true>& acc, const EdgeSet& es, const float* Ksrc, const float* Vsrc, bool kv_once,
                                              int E, int e_base, int sv, int lane) {
  const bool b3 = lane & 8;
  for (int c0 = 0; c0 < E; c0 += 64) {
    const int mc = min(64, E - c0);
    if (c0 > 0) sv = es.src[e_base + c0 + min(lane, mc - 1)];
    for (int i0 = 0; i0 < mc; i0 += G) {
      pk2 kb[G], vb[G], rb[G];
#pragma unroll
      for (int s = 0; s < G; ++s) {
        const int ic = min(i0 + s, mc - 1);
        const int sj = __builtin_amdgcn_readlane(sv, ic);
        kb[s] = ld8(Ksrc + (size_t)sj * D, kv_once, lane);
        vb[s] = ld8(Vsrc + (size_t)sj * D, kv_once, lane);
        if constexpr (R24) rb[s] = ld_r24(es.rhat, (size_t)(e_base + c0 + ic), lane);
        else rb[s] = ld8(es.rhat + (size_t)(e_base + c0 + ic) * D, true, lane);
      }
#pragma unroll
      for (int s = 0; s < G; ++s) acc.step(kb[s], vb[s], rb[s], i0 + s < mc, b3);
    }
  }
}

// the row's results into the LDS tile: agg over the row's q (ag_row), the normalised z_h = sum_e a_e,h rhat_e over the row's own u
// (uz), sigma_h (sg_row); PyG's softmax denominator + 1e-16 (a row without edges: exact zeros)
__device__ __forceinline__ void edge_row_finish(const EdgeAcc<true>& acc, float* uz, float* ag_row, float* sg_row, int lane) {
  const float inv = 1.0f / (acc.lsum + 1e-16f);
  *reinterpret_cast<float2*>(ag_row + 2 * lane) = make_float2(acc.ag[0] * inv, acc.ag[1] * inv);
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const float ih = readlane_f(inv, 8 * hd);
    *reinterpret_cast<float2*>(uz + hd * D + 2 * lane) = make_float2(acc.zz[hd][0] * ih, acc.zz[hd][1] * ih);
  }
  if ((lane & 7) == 0) sg_row[lane >> 3] = acc.lsum * inv;
}

}  // namespace ig
