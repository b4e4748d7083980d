// Validation-step bookkeeping of the reference (infgen/utils/metrics.py) and the open-loop loss, on the device:
//   k_state_accuracy   StateAccuracy.update / NumInsertAccuracy.update (:499-543, :632-676): one wave per row, ballots for the
//                      first enter / first (part 2: last) exit column, popcounts for the slices
//   k_grid_overlap     GridOverlapRate.update (:574-591): one workgroup per (group, step), two LDS bitmaps over the grid cells
//   k_traj_error       minADE.update (:441-464) and minFDE.update (:378-387) in one pass
//   k_multi_traj_error minMultiADE.update (:403-424) and minMultiFDE.update (:349-361) in one pass, with valid_filter and topk
//   k_masked_ce        pred[mask] + torch.nn.CrossEntropyLoss (weights, label smoothing) without the gather: one wave per row
//   k_token_cls        TokenCls.update (:326-333)
//   k_vm_sum           AverageMeter.update (:477-479)
// Every kernel ADDS into a caller-owned accumulator, so a sequence of updates needs no host round trip.  Counters are int64 and
// added with integer atomics (order-free).  Floating sums are float64 and have a fixed order: a lane walks its rows in ascending
// order, the lanes of a workgroup are combined by a tree, each workgroup stores one partial and k_vm_finish - one workgroup -
// adds the partials to the accumulator.  No float atomics: two runs give the same bits.
#include "kernels.h"

namespace ig {

namespace {

template <bool W> __device__ __forceinline__ long long ld_idx(const void* p, size_t i) {
  if constexpr (W) return ((const long long*)p)[i];
  else return (long long)((const int*)p)[i];
}

__device__ __forceinline__ int popc64(unsigned long long m) { return __popcll(m); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// tree over the 256 threads of a workgroup (fixed order); the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int off = 128; off; off >>= 1) {
    if (tid < off) s[tid] += s[tid + off];
    __syncthreads();
  }
  return s[0];
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------- StateAccuracy
// Part 1, the Python slices of one row with bos = first enter, eos = first exit:
//   [:bos] (only if an enter exists) and [eos + 1:] (only if an exit exists) count invalid_state into `invalid`,
//   [bos + 1 : eos] with the defaults bos = 0, eos = T - 1 counts valid_state into `valid`; empty when eos <= bos + 1.
// Part 2 (mask given) on the row rolled by one column (column T - 1 becomes column 0), bos = first enter, eos = LAST exit:
//   mask[:bos] == 0 and mask[eos + 1:] != 0 into `invalid`; over [bos : eos + 1] the mismatches (state > 0) != mask, split by
//   mask == 0 (`invalid`) and mask == 1 (`valid`).
template <bool I64>
__global__ __launch_bounds__(256) void k_state_accuracy(StateAccArgs a) {
  __shared__ long long s_cnt[4][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, T = a.T;
  long long c_valid = 0, c_vcount = 0, c_inv = 0, c_icount = 0;       // wave-uniform
  for (long long row = (long long)blockIdx.x * 4 + wv; row < a.N; row += (long long)gridDim.x * 4) {
    const size_t base = (size_t)row * (size_t)a.ld;
    int bos = -1, eos = -1;
    for (int t0 = 0; t0 < T && (bos < 0 || eos < 0); t0 += 64) {
      const int t = t0 + lane;
      const bool in = t < T;
      const long long v = in ? ld_idx<I64>(a.state, base + t) : 0;
      const unsigned long long be = __ballot(in && v == a.enter_state), bx = __ballot(in && v == a.exit_state);
      if (bos < 0 && be) bos = t0 + __ffsll((long long)be) - 1;
      if (eos < 0 && bx) eos = t0 + __ffsll((long long)bx) - 1;
    }
    {
      const bool hb = bos >= 0, he = eos >= 0;
      const int b = hb ? bos : 0, e = he ? eos : T - 1;
      if (hb) c_icount += bos;
      if (he) c_icount += T - 1 - eos;
      if (e > b + 1) c_vcount += e - b - 1;
      for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const long long v = in ? ld_idx<I64>(a.state, base + t) : 0;
        const bool inv = in && v == a.invalid_state;
        c_inv += popc64(__ballot(inv && hb && t < bos)) + popc64(__ballot(inv && he && t > eos));
        c_valid += popc64(__ballot(in && t > b && t < e && v == a.valid_state));
      }
    }
    if (a.mask) {
      const unsigned char* m = a.mask + (size_t)row * (size_t)a.ldm;
      int b2 = -1, e2 = -1;
      for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const long long r = in ? ld_idx<I64>(a.state, base + (t == 0 ? T - 1 : t - 1)) : 0;
        const unsigned long long be = __ballot(in && r == a.enter_state), bx = __ballot(in && r == a.exit_state);
        if (b2 < 0 && be) b2 = t0 + __ffsll((long long)be) - 1;
        if (bx) e2 = t0 + 63 - __clzll((long long)bx);
      }
      const bool hb = b2 >= 0, he = e2 >= 0;
      const int b = hb ? b2 : 0, e = he ? e2 : T - 1;
      if (hb) c_icount += b2;
      if (he) c_icount += T - 1 - e2;
      for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const long long r = in ? ld_idx<I64>(a.state, base + (t == 0 ? T - 1 : t - 1)) : 0;
        const int mv = in ? (int)m[t] : 0;
        c_inv += popc64(__ballot(in && hb && t < b2 && mv == 0)) + popc64(__ballot(in && he && t > e2 && mv != 0));
        const bool inr = in && t >= b && t <= e;
        const bool differs = (r > 0 ? 1 : 0) != mv;
        c_inv += popc64(__ballot(inr && mv == 0 && differs));
        c_icount += popc64(__ballot(inr && mv == 0));
        c_valid += popc64(__ballot(inr && mv == 1 && differs));
        c_vcount += popc64(__ballot(inr && mv == 1));
      }
    }
  }
  if (lane == 0) { s_cnt[wv][0] = c_valid; s_cnt[wv][1] = c_vcount; s_cnt[wv][2] = c_inv; s_cnt[wv][3] = c_icount; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const long long v = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
    if (v) atomicAdd(a.acc + threadIdx.x, (unsigned long long)v);
  }
}
template __global__ void k_state_accuracy<false>(StateAccArgs);
template __global__ void k_state_accuracy<true>(StateAccArgs);

// --------------------------------------------------------------------------------------------------------- GridOverlapRate
// The reference pops the inserted rows' cells one by one, counts a cell that is already in the occupied set and adds it to the set.
// Whatever the order: of k inserted rows in one cell all k overlap when a non-enter in-range row holds the cell, else k - 1, so
//   overlap = (#inserted in-range rows) - (#distinct cells of inserted rows that no non-enter in-range row occupies).
template <bool S64, bool G64>
__global__ __launch_bounds__(256) void k_grid_overlap(GridOverlapArgs a) {
  __shared__ unsigned s_ins[GO_MAX_CELLS / 32], s_occ[GO_MAX_CELLS / 32];
  __shared__ int s_n[4][3];
  const int t = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const int words = (a.grid_size + 31) >> 5;
  for (int i = tid; i < words; i += 256) { s_ins[i] = 0u; s_occ[i] = 0u; }
  __syncthreads();
  long long r0 = a.ptr ? a.ptr[g] : 0, r1 = a.ptr ? a.ptr[g + 1] : a.N;
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > a.N ? a.N : r1;
  int n_tot = 0, n_ins = 0;
  for (long long row = r0 + tid; row < r1; row += 256) {
    const long long cell = ld_idx<G64>(a.grid, (size_t)row * (size_t)a.ldg + t);
    if (cell == -1) continue;
    ++n_tot;
    const bool ins = ld_idx<S64>(a.state, (size_t)row * (size_t)a.lds + t) == a.enter_state;
    n_ins += ins;
    if (cell >= 0 && cell < a.grid_size) atomicOr((ins ? s_ins : s_occ) + (cell >> 5), 1u << (cell & 31));
  }
  __syncthreads();
  int n_free = 0;
  for (int i = tid; i < words; i += 256) n_free += __popc(s_ins[i] & ~s_occ[i]);
  n_tot = wave_sum(n_tot); n_ins = wave_sum(n_ins); n_free = wave_sum(n_free);
  if ((tid & 63) == 0) { s_n[tid >> 6][0] = n_tot; s_n[tid >> 6][1] = n_ins; s_n[tid >> 6][2] = n_free; }
  __syncthreads();
  if (tid == 0) {
    const int tot = s_n[0][0] + s_n[1][0] + s_n[2][0] + s_n[3][0], ni = s_n[0][1] + s_n[1][1] + s_n[2][1] + s_n[3][1];
    const int nf = s_n[0][2] + s_n[1][2] + s_n[2][2] + s_n[3][2];
    const size_t S = (size_t)a.num_step;
    if (ni - nf) atomicAdd(a.acc + t, (unsigned long long)(ni - nf));
    if (ni) atomicAdd(a.acc + S + t, (unsigned long long)ni);
    if (tot) atomicAdd(a.acc + 2 * S + t, (unsigned long long)tot);
    if (ni >= a.seed_size) atomicAdd(a.acc + 3 * S + t, 1ull);
  }
}
template __global__ void k_grid_overlap<false, false>(GridOverlapArgs);
template __global__ void k_grid_overlap<false, true>(GridOverlapArgs);
template __global__ void k_grid_overlap<true, false>(GridOverlapArgs);
template __global__ void k_grid_overlap<true, true>(GridOverlapArgs);

// ----------------------------------------------------------------------------------------------------------- minADE / minFDE
// As written in the reference: E = min(70, T); ADE row = sum_{t < E} |pred - target| * valid / T (T, not the valid count), counted
// when any column below E is valid; FDE = the single column E - 2 weighted by its valid flag (T = 1: the slice [-1:0] is empty and
// the count reads column -1 = T - 1).
__global__ __launch_bounds__(256) void k_traj_error(TrajErrArgs a) {
  __shared__ double s_red[256];
  __shared__ long long s_c[4][2];
  const int tid = threadIdx.x, T = a.T, E = T < 70 ? T : 70, F = E - 2;
  double ade = 0.0, fde = 0.0;
  int ca = 0, cf = 0;
  for (long long row = (long long)blockIdx.x * 256 + tid; row < a.N; row += (long long)gridDim.x * 256) {
    const float* p = a.pred + (size_t)row * T * 2;
    const float* q = a.target + (size_t)row * T * 2;
    const unsigned char* v = a.valid + (size_t)row * T;
    double s = 0.0;
    bool any = false;
    for (int t = 0; t < E; ++t) {
      const double dx = (double)p[2 * t] - (double)q[2 * t], dy = (double)p[2 * t + 1] - (double)q[2 * t + 1];
      s += sqrt(dx * dx + dy * dy) * (double)v[t];
      any = any || v[t] != 0;
    }
    ade += s / (double)T;
    ca += any;
    if (F >= 0) {
      const double dx = (double)p[2 * F] - (double)q[2 * F], dy = (double)p[2 * F + 1] - (double)q[2 * F + 1];
      fde += sqrt(dx * dx + dy * dy) * (double)v[F];
      cf += v[F];
    } else {
      cf += v[T + F];
    }
  }
  const double ade_b = block_sum(ade, s_red);
  const double fde_b = block_sum(fde, s_red);
  ca = wave_sum(ca); cf = wave_sum(cf);
  if ((tid & 63) == 0) { s_c[tid >> 6][0] = ca; s_c[tid >> 6][1] = cf; }
  __syncthreads();
  if (tid == 0) {
    a.partials[(size_t)blockIdx.x * 2] = ade_b;
    a.partials[(size_t)blockIdx.x * 2 + 1] = fde_b;
    const long long na = s_c[0][0] + s_c[1][0] + s_c[2][0] + s_c[3][0], nf = s_c[0][1] + s_c[1][1] + s_c[2][1] + s_c[3][1];
    if (a.ade_count && na) atomicAdd(a.ade_count, (unsigned long long)na);
    if (a.fde_count && nf) atomicAdd(a.fde_count, (unsigned long long)nf);
  }
}

// --------------------------------------------------------------------------------------------------- minMultiFDE / minMultiADE
// minMultiFDE.update (:349-361) and minMultiADE.update (:403-424) in one pass, k_traj_error's accumulation scheme.  A row takes part
// if any step is valid (keep_invalid_final_step) or if its last step is (valid_filter :115-140).  The guesses are the G largest
// prob in (prob descending, index ascending) order - torch.topk leaves ties open, this pins them - or the first G modes without
// prob (topk :43-76); last = the last valid step (argmax of valid * arange(1..T)).  FDE = the minimum over the guesses of the
// distance at `last`; ADE = the masked mean distance of the guess with the smallest FDE (first minimum in guess order), or
// (ade_by_ade) the minimum over the guesses of the masked mean.
__global__ __launch_bounds__(256) void k_multi_traj_error(MultiTrajErrArgs a) {
  __shared__ double s_red[256];
  __shared__ long long s_c[4];
  const int tid = threadIdx.x, T = a.T, M = a.M, G = a.G;
  double ade = 0.0, fde = 0.0;
  int cnt = 0;
  for (long long row = (long long)blockIdx.x * 256 + tid; row < a.N; row += (long long)gridDim.x * 256) {
    const unsigned char* v = a.valid + (size_t)row * T;
    int last = -1, nv = 0;
    for (int t = 0; t < T; ++t)
      if (v[t]) { last = t; ++nv; }
    if (a.keep_invalid_final_step ? nv == 0 : v[T - 1] == 0) continue;
    const float* q = a.target + (size_t)row * T * 2;
    const float* pr = a.prob ? a.prob + (size_t)row * M : nullptr;
    const bool pick = pr && G < M;
    unsigned long long taken = 0ull;
    double best_f = 0.0, ade_of_best_f = 0.0, best_a = 0.0;
    for (int gi = 0; gi < G; ++gi) {
      int m = gi;
      if (pick) {
        m = -1;
        float pm = 0.f;
        for (int j = 0; j < M; ++j)
          if (!((taken >> j) & 1ull) && (m < 0 || pr[j] > pm)) { m = j; pm = pr[j]; }
        taken |= 1ull << m;
      }
      const float* p = a.pred + ((size_t)row * M + m) * T * 2;
      double s = 0.0, f = 0.0;
      for (int t = 0; t < T; ++t) {
        const double dx = (double)p[2 * t] - (double)q[2 * t], dy = (double)p[2 * t + 1] - (double)q[2 * t + 1];
        const double d = sqrt(dx * dx + dy * dy);
        if (v[t]) s += d;
        if (t == last) f = d;
      }
      const double mean = s / (double)nv;
      if (gi == 0 || f < best_f) { best_f = f; ade_of_best_f = mean; }
      if (gi == 0 || mean < best_a) best_a = mean;
    }
    fde += best_f;
    ade += a.ade_by_ade ? best_a : ade_of_best_f;
    ++cnt;
  }
  const double ade_b = block_sum(ade, s_red);
  const double fde_b = block_sum(fde, s_red);
  cnt = wave_sum(cnt);
  if ((tid & 63) == 0) s_c[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    a.partials[(size_t)blockIdx.x * 2] = ade_b;
    a.partials[(size_t)blockIdx.x * 2 + 1] = fde_b;
    const long long n = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    if (a.ade_count && n) atomicAdd(a.ade_count, (unsigned long long)n);
    if (a.fde_count && n) atomicAdd(a.fde_count, (unsigned long long)n);
  }
}

// ------------------------------------------------------------------------------------------------------- masked cross-entropy
// Row i (mask != 0, target inside [0, C)): lse = max + log(sum exp(x - max)); -log p_c = lse - x_c.  Sums over the selected rows:
//   S1 = sum w_y (lse - x_y),  S2 = sum_i sum_c w_c (lse - x_c) (label smoothing only),  S3 = sum w_y
// A masked-out row is skipped before any of its logits is read.  A target outside [0, C) is skipped like torch's ignore_index.
template <bool T64>
__global__ __launch_bounds__(256) void k_masked_ce(MaskedCeArgs a) {
  __shared__ double s_w[4][3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, C = a.C;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;                           // wave-uniform
  for (long long row = (long long)blockIdx.x * 4 + wv; row < a.R; row += (long long)gridDim.x * 4) {
    if (!a.mask[row]) continue;
    const long long y = ld_idx<T64>(a.target, (size_t)row);
    if (y < 0 || y >= C) continue;
    const float* x = a.logits + (size_t)row * (size_t)a.ld;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, x[c]);
    for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    double se = 0.0;
    for (int c = lane; c < C; c += 64) se += exp((double)x[c] - (double)mx);
    se = wave_sum(se);
    const double lse = (double)mx + log(se);
    const double wy = a.weight ? (double)a.weight[y] : 1.0;
    s1 += wy * (lse - (double)x[y]);
    s3 += wy;
    if (a.smooth) {
      double sm = 0.0;
      for (int c = lane; c < C; c += 64) sm += (a.weight ? (double)a.weight[c] : 1.0) * (lse - (double)x[c]);
      s2 += wave_sum(sm);
    }
  }
  if (lane == 0) { s_w[wv][0] = s1; s_w[wv][1] = s2; s_w[wv][2] = s3; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    a.partials[(size_t)blockIdx.x * 3 + k] = ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k];
  }
}
template __global__ void k_masked_ce<false>(MaskedCeArgs);
template __global__ void k_masked_ce<true>(MaskedCeArgs);

// ------------------------------------------------------------------------------------------------------------------ TokenCls
// acc = (pred[:, :max_guesses] == target[:, None]).any(1) * mask; sum += acc.sum(); count += mask.sum()
template <bool P64, bool T64>
__global__ __launch_bounds__(256) void k_token_cls(TokenClsArgs a) {
  __shared__ long long s_c[4][2];
  const int tid = threadIdx.x;
  int hit = 0, cnt = 0;
  for (long long row = (long long)blockIdx.x * 256 + tid; row < a.R; row += (long long)gridDim.x * 256) {
    const int m = a.mask[row];
    if (!m) continue;
    const long long y = ld_idx<T64>(a.target, (size_t)row);
    bool any = false;
    for (int k = 0; k < a.n_guess; ++k) any = any || ld_idx<P64>(a.pred, (size_t)row * (size_t)a.ldp + k) == y;
    hit += any ? m : 0;
    cnt += m;
  }
  hit = wave_sum(hit); cnt = wave_sum(cnt);
  if ((tid & 63) == 0) { s_c[tid >> 6][0] = hit; s_c[tid >> 6][1] = cnt; }
  __syncthreads();
  if (tid < 2) {
    const long long v = s_c[0][tid] + s_c[1][tid] + s_c[2][tid] + s_c[3][tid];
    if (v) atomicAdd(a.acc + tid, (unsigned long long)v);
  }
}
template __global__ void k_token_cls<false, false>(TokenClsArgs);
template __global__ void k_token_cls<false, true>(TokenClsArgs);
template __global__ void k_token_cls<true, false>(TokenClsArgs);
template __global__ void k_token_cls<true, true>(TokenClsArgs);

// -------------------------------------------------------------------------------------------------------------- AverageMeter
__global__ __launch_bounds__(256) void k_vm_sum(const float* val, long long n, double* partials, unsigned long long* count) {
  __shared__ double s_red[256];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += (double)val[i];
  const double b = block_sum(s, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = b;
  if (threadIdx.x == 0 && blockIdx.x == 0) *count += (unsigned long long)n;      // (one writer: launches of a stream are ordered)
}

// one workgroup: dst_k += the nb partials of column k, thread i summing partials i, i + 256, ... and a tree over the threads
__global__ __launch_bounds__(256) void k_vm_finish(const double* partials, int nb, int K, double* dst0, double* dst1, double* dst2) {
  __shared__ double s_red[256];
  for (int k = 0; k < K; ++k) {
    double* dst = k == 0 ? dst0 : k == 1 ? dst1 : dst2;
    if (!dst) continue;
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += partials[(size_t)i * K + k];
    const double tot = block_sum(s, s_red);
    if (threadIdx.x == 0) *dst += tot;
  }
}

}  // namespace ig
