// Small MLP chains on the fp16 matrix pipe (three-term split, split.cuh), register resident per 16-row wave like
// k_attn_h: 4 waves per workgroup (64-row tiles), three quarter buffers, two workgroups per CU.
//   k_mlpemb_h  MLPEmbedding (reference infgen/modules/layers.py:163-179) with a K0 = 128 j input:
//               Linear(K0,128) LN ReLU Linear(128,128) LN ReLU Linear(128,128)   - the fusion embedding of the raw
//               per-column feature (agent_decoder.py:2265-2287), three k_linear launches before
//   k_heads_h   token_predict_head / state_predict_head + greedy arg-max (agent_decoder.py:2161-2167), k_heads before;
//               LP = true: also the full-softmax log-probability of the arg-max token (log-sum-exp beside the running arg-max)
//               KS > 0: top-k sampling (agent_decoder.py:2162-2163, 2194-2195) instead of the arg-max - a running top-KS per lane
//               beside the running arg-max, merged over the row's four lanes after the last chunk, then k_sample_topk's inverse CDF
//               MK: a per-row allowed-token set (TokenMaskCtl); a banned column counts as -inf for the arg-max, the top-KS and the draw
#include "kernels.h"
#include "layout.h"
#include "tile.cuh"
#include "split.cuh"

namespace ig {

__device__ __forceinline__ void mh_load_row(f32x4 (&v)[8], const float* row, int rg) {
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row) x = *reinterpret_cast<const float4*>(row + 16 * t + 4 * rg);
    v[t] = f32x4{x.x, x.y, x.z, x.w};
  }
}
__device__ __forceinline__ void mh_zero(f32x4 (&v)[8]) {
#pragma unroll
  for (int t = 0; t < 8; ++t) v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void mh_scale_bias(f32x4 (&v)[8], float s, const float* bias, int rg) {
  const f32x4 s4 = splat4(s);
#pragma unroll
  for (int t = 0; t < 8; ++t) v[t] = fma4(v[t], s4, lds4(bias + 16 * t + 4 * rg));
}

constexpr int MH_NT = 256, MH_TILE = 64, MH_RING = 3;

template <int TERMS>
__global__ __launch_bounds__(MH_NT, 2) void k_mlpemb_h(MlpEmbHArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short Wb[MH_RING][QUARTER];
  __shared__ __attribute__((aligned(16))) float Vt[16 + 7 * 128];      // hdr | b0 g0 be0 | b1 g1 be1 | b2
  __shared__ const unsigned short* seg_ptr[1];
  __shared__ int seg_n[1];
  const int ntiles = (a.rows + MH_TILE - 1) / MH_TILE;
  if ((int)blockIdx.x >= ntiles) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, rg = lane >> 4;
  const int nchunk = a.K0 / 128;
  const float* P = a.pack;
  const int o2 = a.K0 * 128 + 3 * 128, o3 = o2 + 16384 + 3 * 128, oh = o3 + 16384 + 128;   // fp32 stages, then the split section
  if (tid == 0) { seg_ptr[0] = reinterpret_cast<const unsigned short*>(P + oh + 16); seg_n[0] = 4 * (nchunk + 2); }
  if (tid < 16) Vt[tid] = P[oh + tid];
  for (int i = tid; i < 384; i += MH_NT) {
    Vt[16 + i] = P[a.K0 * 128 + i];
    Vt[16 + 384 + i] = P[o2 + 16384 + i];
  }
  for (int i = tid; i < 128; i += MH_NT) Vt[16 + 768 + i] = P[o3 + 16384 + i];
  __syncthreads();
  QuarterStream<MH_NT, MH_RING> qs;
  qs.init(seg_ptr, seg_n, 1, (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x, Wb, tid);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row = tile * MH_TILE + w * 16 + j;
    const bool valid = row < a.rows;
    u32x4 Bh[4], Bl[4];
    f32x4 h[8];
    mh_zero(h);
    for (int c = 0; c < nchunk; ++c) {
      f32x4 xc[8];
      mh_load_row(xc, valid ? a.X + (size_t)row * a.ldx + 128 * c : nullptr, rg);
      const float inv = frags_scaled(xc, Bh, Bl) * Vt[0];
      f32x4 part[8];
      mh_zero(part);
#pragma unroll
      for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(part, qs.take(), Bh[s], Bl[s], lane);
#pragma unroll
      for (int t = 0; t < 8; ++t) h[t] = fma4(part[t], splat4(inv), h[t]);
    }
    mh_scale_bias(h, 1.0f, Vt + 16, rg);
    ln_regs<true, true>(h, Vt + 16 + 128, Vt + 16 + 256, rg);
    {
      const float inv = frags_scaled(h, Bh, Bl) * Vt[1];
      mh_zero(h);
#pragma unroll
      for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(h, qs.take(), Bh[s], Bl[s], lane);
      mh_scale_bias(h, inv, Vt + 16 + 384, rg);
      ln_regs<true, true>(h, Vt + 16 + 512, Vt + 16 + 640, rg);
    }
    {
      const float inv = frags_scaled(h, Bh, Bl) * Vt[2];
      mh_zero(h);
#pragma unroll
      for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(h, qs.take(), Bh[s], Bl[s], lane);
      mh_scale_bias(h, inv, Vt + 16 + 768, rg);
    }
    if (valid) {
      float* o = a.Y + (size_t)row * a.ldy;
#pragma unroll
      for (int t = 0; t < 8; ++t)
        *reinterpret_cast<float4*>(o + 16 * t + 4 * rg) = make_float4(h[t][0], h[t][1], h[t][2], h[t][3]);
    }
  }
}

// One lane's running top-KS for k_heads_h<TERMS, LP, KS>: (value, column) pairs in k_sample_topk's total order (value descending,
// then column ascending), statically indexed registers.  A lane meets its columns in ascending order, so a new pair goes behind the
// entries of equal value: the first strictly smaller entry takes it and every later entry moves down by one (the last one drops out).
// Only the first k (= sample_k, wave-uniform) slots are kept: the rest stay (-inf, none), which is what the merge shifts in.
template <int KS> __device__ __forceinline__ void topk_insert(float (&tv)[KS], int (&ti)[KS], int k, float v, int col) {
  bool sw = false;
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    if (j < k) {
      sw = sw || v > tv[j];
      const float ov = tv[j];
      const int oi = ti[j];
      tv[j] = sw ? v : ov;  ti[j] = sw ? col : oi;
      v = sw ? ov : v;      col = sw ? oi : col;
    }
  }
}

template <int TERMS, bool LP, int KS, bool MK>
__global__ __launch_bounds__(MH_NT, 2) void k_heads_h(ArgsFor<HeadsArgs, MK> a) {
  __shared__ __attribute__((aligned(16))) unsigned short Wb[MH_RING][QUARTER];
  // token head: hdr | b0 g0 be0 ; state head: hdr | b0 g0 be0 | W3 [3][128] | b3 [3]
  __shared__ __attribute__((aligned(16))) float Vt[16 + 384 + 16 + 384 + 384 + 16];
  __shared__ const unsigned short* seg_ptr[3];
  __shared__ int seg_n[3];
  const int ntiles = (a.rows + MH_TILE - 1) / MH_TILE;
  if ((int)blockIdx.x >= ntiles) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, rg = lane >> 4;
  const int nchunk = a.token_size / 128;
  const float* PT = a.tok_pack;
  const float* PS = a.st_pack;
  const int W3T = 16768;                                            // P(128, token_size), then b3
  const int oht = W3T + 128 * a.token_size + a.token_size;          // split section of the token head pack
  const int ohs = 16768 + 3 * 128 + 3;                              // ... of the state head pack (W3 [3][128] row-major, b3 [3])
  const int ohs_al = (ohs + 3) & ~3;
  float* VS = Vt + 16 + 384;
  if (tid == 0) {
    const unsigned short* qt = reinterpret_cast<const unsigned short*>(PT + oht + 16);
    seg_ptr[0] = qt;                                                              seg_n[0] = 4;           // token W0
    seg_ptr[1] = reinterpret_cast<const unsigned short*>(PS + ohs_al + 16);       seg_n[1] = 4;           // state W0
    seg_ptr[2] = qt + 4 * QUARTER;                                                seg_n[2] = 4 * nchunk;  // token W3 chunks
  }
  if (tid < 16) { Vt[tid] = PT[oht + tid]; VS[tid] = PS[ohs_al + tid]; }
  for (int i = tid; i < 384; i += MH_NT) {
    Vt[16 + i] = PT[16384 + i];
    VS[16 + i] = PS[16384 + i];
    VS[16 + 384 + i] = PS[16768 + i];
  }
  if (tid < 3) VS[16 + 768 + tid] = PS[16768 + 384 + tid];
  __syncthreads();
  QuarterStream<MH_NT, MH_RING> qs;
  qs.init(seg_ptr, seg_n, 3, (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x, Wb, tid);
  const float* b3 = PT + W3T + (size_t)128 * a.token_size;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row = tile * MH_TILE + w * 16 + j;
    const bool valid = row < a.rows;
    u32x4 Bh[4], Bl[4];
    f32x4 x[8], ht[8], hs[8];
    mh_load_row(x, valid ? a.X + (size_t)row * D : nullptr, rg);
    const float inv_x = frags_scaled(x, Bh, Bl);
    mh_zero(ht); mh_zero(hs);
#pragma unroll
    for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(ht, qs.take(), Bh[s], Bl[s], lane);
#pragma unroll
    for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(hs, qs.take(), Bh[s], Bl[s], lane);
    mh_scale_bias(ht, inv_x * Vt[0], Vt + 16, rg);
    ln_regs<true, true>(ht, Vt + 16 + 128, Vt + 16 + 256, rg);
    mh_scale_bias(hs, inv_x * VS[0], VS + 16, rg);
    ln_regs<true, true>(hs, VS + 16 + 128, VS + 16 + 256, rg);
    // state head: three outputs, plain dot products over the lane's 32 features, then the four lanes of the row
    {
      float best = -INFINITY;
      int bi = 0;
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        f32x4 acc = splat4(0.f);
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = fma4(hs[t], lds4(VS + 16 + 384 + o * 128 + 16 * t + 4 * rg), acc);
        const float sdot = xor_lanes((acc[0] + acc[1]) + (acc[2] + acc[3])) + VS[16 + 768 + o];
        if (sdot > best) { best = sdot; bi = o; }
      }
      if (valid && rg == 0) a.next_state[row] = bi;
    }
    // token head: logits in 128-wide chunks, running arg-max (first maximum)
    const float inv_h = frags_scaled(ht, Bh, Bl) * Vt[1];
    float bv = -INFINITY;
    int bidx = 0x7fffffff;
    // MK: the row's set (NULL: unconstrained).  Per chunk the lane reads the chunk's four words once and keeps the 32 bits of its own
    // columns (bit 4 t + e: column 128 c + 16 t + 4 rg + e) in one register.  Under a mask the arg-max value is no longer the
    // maximum, so LP carries the true running maximum rmax for the log-sum-exp (without a mask bv IS it)
    const unsigned* mset = nullptr;
    if constexpr (MK) { if (valid) mset = token_mask_set(a.mask, row, a.token_size / 32); }
    float rmax = -INFINITY;
    // LP: sum of exp(v - bv) over the lane's columns so far (bv, the running arg-max value, is their maximum); rescaled once per
    // 128-wide chunk, whose 32 logits of the lane wait in lg until the chunk's maximum is known
    float lse = 0.f;
    // KS: the lane's KS best (value, column) pairs so far (topk_insert); thr, refreshed once per chunk, is the largest sample_k-th
    // best value among the row's four lanes: a logit below it has sample_k better ones in that lane alone and is skipped (one equal
    // to it may still win its tie by column and goes through the insertion, which leaves a list it does not beat as it is).  Past
    // the first chunks few logits pass, so the wave-divergent insertion is rare
    float tv[KS > 0 ? KS : 1], thr = -INFINITY;
    int ti[KS > 0 ? KS : 1];
    if constexpr (KS > 0) {
#pragma unroll
      for (int q = 0; q < KS; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
    }
    for (int c = 0; c < nchunk; ++c) {
      f32x4 lg[8];
      mh_zero(lg);
      const float m_prev = MK ? rmax : bv;
      unsigned lm = 0xffffffffu;
      if constexpr (MK) {
        if (mset) {
          const uint4 mw = *reinterpret_cast<const uint4*>(mset + 4 * c);
          const int sh = 4 * rg;
          lm = ((mw.x >> sh) & 0xfu) | (((mw.x >> (16 + sh)) & 0xfu) << 4) | (((mw.y >> sh) & 0xfu) << 8) |
               (((mw.y >> (16 + sh)) & 0xfu) << 12) | (((mw.z >> sh) & 0xfu) << 16) | (((mw.z >> (16 + sh)) & 0xfu) << 20) |
               (((mw.w >> sh) & 0xfu) << 24) | (((mw.w >> (16 + sh)) & 0xfu) << 28);
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(lg, qs.take(), Bh[s], Bl[s], lane);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int col = 128 * c + 16 * t + 4 * rg;
        const float4 bb = *reinterpret_cast<const float4*>(b3 + col);
        const float v0 = lg[t][0] * inv_h + bb.x, v1 = lg[t][1] * inv_h + bb.y;
        const float v2 = lg[t][2] * inv_h + bb.z, v3 = lg[t][3] * inv_h + bb.w;
        if (a.logits && valid)
          *reinterpret_cast<float4*>(a.logits + (size_t)row * a.token_size + col) = make_float4(v0, v1, v2, v3);
        if constexpr (!MK) {
          if (v0 > bv) { bv = v0; bidx = col; }
          if (v1 > bv) { bv = v1; bidx = col + 1; }
          if (v2 > bv) { bv = v2; bidx = col + 2; }
          if (v3 > bv) { bv = v3; bidx = col + 3; }
          if constexpr (LP) lg[t] = f32x4{v0, v1, v2, v3};
          if constexpr (KS > 0) {
            if (v0 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v0, col);
            if (v1 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v1, col + 1);
            if (v2 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v2, col + 2);
            if (v3 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v3, col + 3);
          }
        } else {
          // the same comparisons in the same order, a banned column's logit read as -inf (it never beats bv, and never enters a list)
          const unsigned nb = lm >> (4 * t);
          const bool a0 = nb & 1u, a1 = nb & 2u, a2 = nb & 4u, a3 = nb & 8u;
          if (a0 && v0 > bv) { bv = v0; bidx = col; }
          if (a1 && v1 > bv) { bv = v1; bidx = col + 1; }
          if (a2 && v2 > bv) { bv = v2; bidx = col + 2; }
          if (a3 && v3 > bv) { bv = v3; bidx = col + 3; }
          if constexpr (LP) {
            lg[t] = f32x4{v0, v1, v2, v3};
            rmax = fmaxf(fmaxf(rmax, fmaxf(v0, v1)), fmaxf(v2, v3));
          }
          if constexpr (KS > 0) {
            if (a0 && v0 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v0, col);
            if (a1 && v1 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v1, col + 1);
            if (a2 && v2 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v2, col + 2);
            if (a3 && v3 >= thr) topk_insert<KS>(tv, ti, a.sample_k, v3, col + 3);
          }
        }
      }
      if constexpr (KS > 0) {
        float kth = tv[0];
#pragma unroll
        for (int q = 1; q < KS; ++q) kth = q < a.sample_k ? tv[q] : kth;
        thr = fmaxf(kth, __shfl_xor(kth, 16, 64));
        thr = fmaxf(thr, __shfl_xor(thr, 32, 64));
      }
      if constexpr (LP) {
        const float mx = MK ? rmax : bv;
        lse *= expf(m_prev - mx);                    // (first chunk: exp(-inf) = 0 times 0)
#pragma unroll
        for (int t = 0; t < 8; ++t)
          lse += (expf(lg[t][0] - mx) + expf(lg[t][1] - mx)) + (expf(lg[t][2] - mx) + expf(lg[t][3] - mx));
      }
    }
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bidx, off, 64);
      if constexpr (LP && !MK) {                     // the row's four lanes in a fixed order: xor 16, then 32
        const float os = __shfl_xor(lse, off, 64);
        const float m = fmaxf(bv, ov);
        lse = lse * expf(bv - m) + os * expf(ov - m);
      }
      if constexpr (LP && MK) {                      // the same merge around the lanes' true maxima
        const float os = __shfl_xor(lse, off, 64);
        const float om = __shfl_xor(rmax, off, 64);
        const float m = fmaxf(rmax, om);
        lse = lse * expf(rmax - m) + os * expf(om - m);
        rmax = m;
      }
      if (ov > bv || (ov == bv && oi < bidx)) { bv = ov; bidx = oi; }
    }
    if constexpr (KS == 0) {
      // (MK: a set without a token breaks the table's contract; such a row emits token 0, never an index beyond the vocabulary)
      if constexpr (MK) bidx = bidx == TOPK_NONE ? 0 : bidx;
      if (valid && rg == 0) a.next_token[row] = bidx;
      if constexpr (LP && !MK) {
        // best - (max + log(sum)) with best == max by construction (the arg-max value IS the maximum): -log(sum), one rounding less
        if (valid && rg == 0) a.token_logprob[row] = -logf(lse);
      }
      if constexpr (LP && MK) {
        // where the allowed arg-max is the row's maximum this is the unmasked kernel's -log(sum), bit for bit
        if (valid && rg == 0) a.token_logprob[row] = bv == rmax ? -logf(lse) : bv - (rmax + logf(lse));
      }
    } else {
      // the row's top-KS from its four lanes' lists: KS rounds, each takes the best head under the total order (the lanes' columns
      // are disjoint, so the winner is the lane whose head has the winning column) and that lane's list moves up by one
      float mv[KS];
      int mi[KS];
#pragma unroll
      for (int r = 0; r < KS; ++r) {
        mv[r] = -INFINITY; mi[r] = 0x7fffffff;
        if (r < a.sample_k) {                        // (wave-uniform: only the first sample_k results are read)
          float wv = tv[0];
          int wi = ti[0];
#pragma unroll
          for (int off = 16; off < 64; off <<= 1) {
            const float ov = __shfl_xor(wv, off, 64);
            const int oi = __shfl_xor(wi, off, 64);
            if (ov > wv || (ov == wv && oi < wi)) { wv = ov; wi = oi; }
          }
          mv[r] = wv; mi[r] = wi;
          const bool won = wi == ti[0];
#pragma unroll
          for (int q = 0; q + 1 < KS; ++q) { tv[q] = won ? tv[q + 1] : tv[q]; ti[q] = won ? ti[q + 1] : ti[q]; }
          tv[KS - 1] = won ? -INFINITY : tv[KS - 1];
          ti[KS - 1] = won ? 0x7fffffff : ti[KS - 1];
        }
      }
      float sum, it = 1.0f, top_p = 1.0f;
      int m;
      if (valid) sampling_row(a.ctl, row, &it, &top_p);
      int pick;
      if constexpr (MK) pick = topk_inverse_cdf_masked<KS>(mv, mi, a.sample_k, valid ? a.uniform[row] : 0.f, it, top_p, &sum, &m);
      else pick = topk_inverse_cdf<KS>(mv, a.sample_k, valid ? a.uniform[row] : 0.f, it, top_p, &sum, &m);
      float pv = mv[0];
      int pi = mi[0];
#pragma unroll
      for (int q = 1; q < KS; ++q) { pv = q == pick ? mv[q] : pv; pi = q == pick ? mi[q] : pi; }
      if constexpr (MK) pi = pi == TOPK_NONE ? 0 : pi;
      if (valid && rg == 0) {
        a.next_token[row] = pi;
        if (a.sample_logprob) a.sample_logprob[row] = (pv - mv[0]) * it - logf(sum);
        if constexpr (LP) a.token_logprob[row] = pv - ((MK ? rmax : bv) + logf(lse));
      }
    }
  }
}

// top-10 of one MAP_HEAD_N-logit row on one wave (map_decoder.py:120-121: topk of the softmax, which is monotone, so the logits
// are ranked): 16 logits per lane (columns 256 i + 4 lane + c), ten rounds of a wave arg-max over the logits not yet taken.
// Equal values take the lower index first, like k_heads_h's arg-max.
__device__ __forceinline__ void map_topk_row(const float* lg, long long* top, int lane) {
  float v[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 x = *reinterpret_cast<const float4*>(lg + 256 * i + 4 * lane);
    v[4 * i] = x.x; v[4 * i + 1] = x.y; v[4 * i + 2] = x.z; v[4 * i + 3] = x.w;
  }
  unsigned taken = 0;
#pragma unroll
  for (int r = 0; r < MAP_TOPK; ++r) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 16; ++k)          // (ascending column order: the first of equal values stays)
      if (!((taken >> k) & 1u) && (bi == 0x7fffffff || v[k] > bv)) { bv = v[k]; bi = 256 * (k >> 2) + 4 * lane + (k & 3); }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (((bi & 255) >> 2) == lane) taken |= 1u << (4 * (bi >> 8) + (bi & 3));
    if (lane == 0) top[r] = bi;
  }
}

// the map encoder's token_predict_head (map_decoder.py:119-121): rows gather[k] of X -> Linear(128,128) LN ReLU Linear(128,1024),
// the logits stored, then every wave ranks its own 16 rows (map_topk_row) from what it just stored
template <int TERMS>
__global__ __launch_bounds__(MH_NT, 2) void k_map_head_h(MapHeadArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short Wb[MH_RING][QUARTER];
  __shared__ __attribute__((aligned(16))) float Vt[16 + 384];      // hdr | b0 g0 be0
  __shared__ const unsigned short* seg_ptr[2];
  __shared__ int seg_n[2];
  const int ntiles = (a.rows + MH_TILE - 1) / MH_TILE;
  if ((int)blockIdx.x >= ntiles) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, rg = lane >> 4;
  constexpr int nchunk = MAP_HEAD_N / 128;
  const float* P = a.pack;
  const int W3 = 16768;                                      // P(128, MAP_HEAD_N), then b3
  const int oh = W3 + 128 * MAP_HEAD_N + MAP_HEAD_N;         // split section
  if (tid == 0) {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(P + oh + 16);
    seg_ptr[0] = q;                seg_n[0] = 4;             // W0
    seg_ptr[1] = q + 4 * QUARTER;  seg_n[1] = 4 * nchunk;    // W3 chunks
  }
  if (tid < 16) Vt[tid] = P[oh + tid];
  for (int i = tid; i < 384; i += MH_NT) Vt[16 + i] = P[16384 + i];
  __syncthreads();
  QuarterStream<MH_NT, MH_RING> qs;
  qs.init(seg_ptr, seg_n, 2, (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x, Wb, tid);
  const float* b3 = P + W3 + (size_t)128 * MAP_HEAD_N;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row = tile * MH_TILE + w * 16 + j;
    const bool valid = row < a.rows;
    u32x4 Bh[4], Bl[4];
    f32x4 h[8];
    mh_load_row(h, valid ? a.X + (size_t)a.gather[row] * a.ldx : nullptr, rg);
    const float inv_x = frags_scaled(h, Bh, Bl);
    mh_zero(h);
#pragma unroll
    for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(h, qs.take(), Bh[s], Bl[s], lane);
    mh_scale_bias(h, inv_x * Vt[0], Vt + 16, rg);
    ln_regs<true, true>(h, Vt + 16 + 128, Vt + 16 + 256, rg);
    const float inv_h = frags_scaled(h, Bh, Bl) * Vt[1];
    for (int c = 0; c < nchunk; ++c) {
      f32x4 lg[8];
      mh_zero(lg);
#pragma unroll
      for (int s = 0; s < 4; ++s) gemm_quarter<TERMS>(lg, qs.take(), Bh[s], Bl[s], lane);
      if (valid) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int col = 128 * c + 16 * t + 4 * rg;
          const float4 bb = *reinterpret_cast<const float4*>(b3 + col);
          *reinterpret_cast<float4*>(a.logits + (size_t)row * MAP_HEAD_N + col) =
              make_float4(lg[t][0] * inv_h + bb.x, lg[t][1] * inv_h + bb.y, lg[t][2] * inv_h + bb.z, lg[t][3] * inv_h + bb.w);
        }
      }
    }
    // the wave's stores complete before its lanes read each other's columns back (one CU: no cache maintenance needed)
    __threadfence_block();
    const int r0 = tile * MH_TILE + w * 16;
    for (int rr = 0; rr < 16 && r0 + rr < a.rows; ++rr)
      map_topk_row(a.logits + (size_t)(r0 + rr) * MAP_HEAD_N, a.top + (size_t)(r0 + rr) * MAP_TOPK, lane);
  }
}

#if !IG_BF16_OPERANDS
// the ranking alone, one row per wave: the fp32-MFMA path of infgen_map_token_head (k_linear wrote the logits)
__global__ __launch_bounds__(256) void k_map_topk(MapHeadArgs a) {
  const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (row >= a.rows) return;
  map_topk_row(a.logits + (size_t)row * MAP_HEAD_N, a.top + (size_t)row * MAP_TOPK, threadIdx.x & 63);
}
#endif

#if !IG_BF16_OPERANDS
template __global__ void k_map_head_h<3>(MapHeadArgs);
#endif
template __global__ void k_map_head_h<1>(MapHeadArgs);
#if !IG_BF16_OPERANDS
template __global__ void k_mlpemb_h<3>(MlpEmbHArgs);
#endif
template __global__ void k_mlpemb_h<1>(MlpEmbHArgs);
#if !IG_BF16_OPERANDS
template __global__ void k_heads_h<3, false, 0>(HeadsArgs);
template __global__ void k_heads_h<3, true, 0>(HeadsArgs);
template __global__ void k_heads_h<3, false, HEADS_KS>(HeadsArgs);
template __global__ void k_heads_h<3, true, HEADS_KS>(HeadsArgs);
#endif
template __global__ void k_heads_h<1, false, 0>(HeadsArgs);
template __global__ void k_heads_h<1, true, 0>(HeadsArgs);
template __global__ void k_heads_h<1, false, HEADS_KS>(HeadsArgs);
template __global__ void k_heads_h<1, true, HEADS_KS>(HeadsArgs);
// the masked variants (HeadsArgs.mask)
#if !IG_BF16_OPERANDS
template __global__ void k_heads_h<3, false, 0, true>(Masked<HeadsArgs>);
template __global__ void k_heads_h<3, true, 0, true>(Masked<HeadsArgs>);
template __global__ void k_heads_h<3, false, HEADS_KS, true>(Masked<HeadsArgs>);
template __global__ void k_heads_h<3, true, HEADS_KS, true>(Masked<HeadsArgs>);
#endif
template __global__ void k_heads_h<1, false, 0, true>(Masked<HeadsArgs>);
template __global__ void k_heads_h<1, true, 0, true>(Masked<HeadsArgs>);
template __global__ void k_heads_h<1, false, HEADS_KS, true>(Masked<HeadsArgs>);
template __global__ void k_heads_h<1, true, HEADS_KS, true>(Masked<HeadsArgs>);

}  // namespace ig
