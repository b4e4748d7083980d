// k_edge_fused: the edge side of one AttentionLayer (reference infgen/modules/layers.py:78-99,109) for a tile of 16
// destination rows with the absorbed relative-position query U and the aggregate Z kept on chip:
//
//   phase 1 (matrix pipe)  u_h = q_h W'_kr,h for the 16 rows, wave w = head w; three-term fp16 split like k_attn_h
//                          (split.cuh), weights straight from L2 as MFMA A fragments; result -> LDS tile [16][8][128];
//                          the q tile is parked in LDS as well (in the buffer that later takes agg)
//   phase 2 (vector pipe)  the edge loop (edge_attn.cuh: EdgeAcc - online softmax with PyG's + 1e-16, one wave per row,
//                          rows dealt to the 8 waves through an LDS counter), u and q read from LDS, the normalised
//                          z_h = sum_e a_e,h rhat_e written back over the row's own u
//   phase 3 (matrix pipe)  agg' = agg + W'_vr,h z_h + b'_h sigma_h, wave w = head w, -> global AGG
//
// so that the node kernel (k_attn_h / k_attn_post with has_pos = 0) never sees U, Z or SIG: per row and sublayer 512 B of
// q in and 512 B of agg' out instead of 9.2 KB (4 KB of U in, 4 KB of Z out, q, agg, sigma) here and 8 KB in the node
// kernel.  The GEMM arithmetic (operand scaling, split, order of the products) is that of k_attn_h's z-GEMM and u-GEMM.
// 1024 threads = 16 waves = two 16-row halves (wave w: head w & 7 of half w >> 3 in the matrix phases), 150 KB of LDS: ONE
// workgroup per CU.  Two co-resident 8-wave workgroups (75 KB each) were ~5 % faster and WRONG: the workgroup that is not the
// first on its CU got single rows off by ~1e-2, different rows every run (tools/determinism_probe2.py; never with one
// workgroup per CU - the "bring-up scare" of fourier_h.hip again, now reproducible: DESIGN.md section 5.1).
#include "kernels.h"
#include "layout.h"
#include "tile.cuh"
#include "split.cuh"
#include "edge_attn.cuh"
#include "edge_tile.cuh"

namespace ig {

constexpr int EF_HALVES = 2;                // 16-row halves per workgroup (the N dimension of the 16x16 MFMAs is 16 rows)
constexpr int EF_WAVES = 8 * EF_HALVES;     // one per (head, half) in the matrix phases
constexpr int EF_NT = 64 * EF_WAVES;
constexpr int EF_ROWS = 16 * EF_HALVES;
constexpr int EF_LDU = H * D + 4;           // row stride of the U / Z tile in floats (+4: conflict-free b128 column writes)
constexpr int EF_LDA = D + 4;

// G = edges per trip of the edge loop (their K / V / rhat rows are requested together); R24: rhat rows in the packed 24-bit
// format (kernels.h); HALVES = 16-row groups per workgroup: 2 when the launch fills the chip, 1 for small launches (up to 256
// groups = 4 k rows: twice the workgroups, and the 16 waves take ONE row each in the edge loop instead of two - the loop of a
// small launch is the latency of its longest rows; the 8 waves without a (head, half) idle in the matrix phases)
// WAVES = 16: one 1024-thread workgroup per CU; WAVES = 8 (HALVES = 1 only, 75 KB of LDS): two co-resident workgroups per CU, whose
// matrix phases run under each other's edge loops - the configuration that gave wrong rows in round 2 and is exact since the
// loop's per-lane broadcasts are real register pairs (edge_attn.cuh: bc_v)
// timing experiment (build with -DIG_EF_TRACE=1, run with INFGEN_EDGE_DBG bit 7): s_memtime of wave 0 of workgroup 2600 -> a.dbgbuf
#ifndef IG_EF_TRACE
#define IG_EF_TRACE 0
#endif
#if IG_EF_TRACE
#define EF_STAMP(i) do { if ((a.dbg & 128) && blockIdx.x == 2600 && threadIdx.x == 0) reinterpret_cast<unsigned long long*>(a.dbgbuf)[i] = __builtin_readcyclecounter(); } while (0)
#else
#define EF_STAMP(i) do {} while (0)
#endif
template <int G, bool R24, int HALVES, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 4) void k_edge_fused(EdgeFusedArgs a) {
  static_assert(WAVES == 16 || (WAVES == 8 && HALVES == 1), "8-wave workgroups take one 16-row group");
  constexpr int ROWS = 16 * HALVES;
  __shared__ __attribute__((aligned(16))) float UZ[ROWS * EF_LDU];
  __shared__ __attribute__((aligned(16))) float AG[ROWS * EF_LDA];     // q tile (phase 1 -> 2), then agg (phase 2 -> 3)
  __shared__ float SG[ROWS * H];
  __shared__ int next_row;
  const int ngroups = a.groups ? *a.n_groups : (a.rows + 15) / 16;        // 16-row groups; a tile takes HALVES of them
  const int ntiles = (ngroups + HALVES - 1) / HALVES;
  if (HALVES == 1 && WAVES == 16 && warm_l2(a.warm, blockIdx.x, threadIdx.x, 64 * WAVES)) return;       // kernels.h: WarmArgs
  const int tile = xcd_tile(blockIdx.x, a.tiles_per_scene);      // (edge_tile.cuh: a scene's tiles share an L2)
  if (tile >= ntiles) return;
  EF_STAMP(0);
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int h = w & 7, half = w >> 3;
  // first row of each half (-1: no such group)
  int r0h[HALVES];
#pragma unroll
  for (int b = 0; b < HALVES; ++b) {
    const int gi = HALVES * tile + b;
    r0h[b] = gi < ngroups ? 16 * (a.groups ? a.groups[gi] : gi) : -1;
  }
  const bool mat = half < HALVES;                  // this wave has a (head, half) of the matrix phases
  const int r0 = (HALVES > 1 && half) ? r0h[HALVES - 1] : r0h[0];
  const int jl = 16 * half + j;                    // this lane's row of the LDS tiles in the matrix phases
  const int row = r0 + j;
  const bool valid = mat && r0 >= 0 && row < a.rows;
  const float* hdr = a.pack + AH_HDR;
  if (threadIdx.x == 0) next_row = 0;
  // Longest rows first (edge_tile.cuh: rank_by_count): the last wave ranks the rows (a load of ROWS counts, ROWS compares) while
  // phase 1 runs.
  constexpr bool SORT_ROWS = !(HALVES == 1 && WAVES == 16);            // (one row per wave: nothing to order)
  __shared__ unsigned char row_order[ROWS];
  if (SORT_ROWS && w == WAVES - 1) {
    const int rl = lane & (ROWS - 1);
    const int rb = (HALVES > 1 && (rl >> 4)) ? r0h[HALVES - 1] : r0h[0];
    const int dr = rb + (rl & 15);
    const int cnt = (rb >= 0 && dr < a.rows) ? a.es.cnt[dr] : 0;
    const int rank = rank_by_count<false>(cnt, rl, ROWS);
    if (lane < ROWS) row_order[rank] = (unsigned char)rl;
  }

  EF_STAMP(1);
  // ---- phase 1: u_h = q_h W'_kr,h (K = 16: v_mfma_f32_16x16x16_f16; B fragment = the head's 16 query values of row j)
  if (mat) {
    float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) qv = *reinterpret_cast<const float4*>(a.Q + (size_t)row * D + DH * h + 4 * g);
    v4h ah[8], al[8];
    load_wkr(reinterpret_cast<const unsigned short*>(a.pack + AH_PRE), h, lane, ah, al);
    *reinterpret_cast<float4*>(AG + jl * EF_LDA + DH * h + 4 * g) = qv;
    u_gemm(f32x4{qv.x, qv.y, qv.z, qv.w}, ah, al, hdr, UZ + jl * EF_LDU + h * D + 4 * g, MaxShfl());
  }
  EF_STAMP(2);
  __syncthreads();
  EF_STAMP(3);

  // ---- phase 2: edge loop, one wave per destination row
  {
    const bool kv_once = a.kv_once != 0;
    // rows are dealt to the waves through an LDS counter (the agent set's lists vary in length)
    auto take_row = [&]() {
      int r = 0;
      if (lane == 0) { r = atomicAdd(&next_row, 1); if (SORT_ROWS && r < ROWS) r = row_order[r]; }
      return __builtin_amdgcn_readfirstlane(r);
    };
    for (int rl = take_row(); rl < ROWS; rl = take_row()) {
      const int rbase = (HALVES > 1 && (rl >> 4)) ? r0h[HALVES - 1] : r0h[0];
      const int drow = rbase + (rl & 15);
      const bool live = rbase >= 0 && drow < a.rows && !(a.dbg & 1);
      const int E = live ? __builtin_amdgcn_readfirstlane(a.es.cnt[drow]) : 0;
      const int e_base = live ? __builtin_amdgcn_readfirstlane(a.es.off[drow]) : 0;
      int sv = E > 0 ? a.es.src[e_base + min(lane, E - 1)] : 0;            // source indices of up to 64 edges in one register
      float* uz = UZ + rl * EF_LDU;
      EdgeAcc<true> acc;
      acc.q = *reinterpret_cast<const float2*>(AG + rl * EF_LDA + 2 * lane);
      acc.load_u(uz, lane);
      acc.reset();
      edge_row_loop<G, R24>(acc, a.es, a.Ksrc, a.Vsrc, kv_once, E, e_base, sv, lane);
      edge_row_finish(acc, uz, AG + rl * EF_LDA, SG + rl * H, lane);
    }
  }
  EF_STAMP(4);
  // (phase 3's weight fragments are requested BEFORE the barrier: a wave that has finished its rows waits there anyway, and the
  // fragments' L2 latency runs under that wait)
  v8h p3h[4], p3l[4];
  if (mat) load_wvr(reinterpret_cast<const unsigned short*>(a.pack + AH_POST), h, lane, p3h, p3l);
  EF_STAMP(5);
  __syncthreads();
  EF_STAMP(6);

  // ---- phase 3: agg' = agg + W'_vr,h z_h + b'_h sigma_h  (k_attn_h's z-GEMM: |z| <= sqrt(127), static prescale 1024)
  if (mat) {
    const f32x4 wz = z_gemm(UZ + jl * EF_LDU + h * D + 8 * g, p3h, p3l, hdr[4]);
    if (valid) {
      const float sg = SG[jl * H + h];
      const f32x4 bvr = lds4(a.pack + AL_BVR + DH * h + 4 * g);
      const f32x4 o = agg_out(lds4(AG + jl * EF_LDA + DH * h + 4 * g), wz, bvr, sg);
      *reinterpret_cast<float4*>(a.AGG + (size_t)row * D + DH * h + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  EF_STAMP(7);
}

template __global__ void k_edge_fused<4, false, 2, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<6, false, 2, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<8, false, 2, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<4, true, 2, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<6, true, 2, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<8, true, 2, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<6, false, 1, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<6, true, 1, 16>(EdgeFusedArgs);
template __global__ void k_edge_fused<6, false, 1, 8>(EdgeFusedArgs);
template __global__ void k_edge_fused<6, true, 1, 8>(EdgeFusedArgs);

}  // namespace ig
