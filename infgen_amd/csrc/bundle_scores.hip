// Scoring of a whole validation batch (reference infgen/metrics/compute_metrics.py:891-1103, compute_scenario_metrics_for_bundle):
// per scenario, over the rows of ALL its rollouts (objects of rollout 0, then 1, ...), what scores.compute_scenario_metrics
// computes for one MetricFeatures with ~16 k_window_loglik launches and the torch arithmetic between them.
//   k_bundle_field   one workgroup per (field, scenario): the windowed histogram log-likelihoods of every (object, window)
//                    - summed over the valid steps in step order, exactly as k_window_loglik sums them -, exp(sum / count), the
//                    (0, 1] masked means over everything (scalar) and over the objects per window (long)
//   k_bundle_meta    one workgroup per scenario: the weighted meta-metric, its long form with the zero rule; workgroup 0 counts
//                    the scenarios with a placement / removement score
// The 256 threads of k_bundle_field form RT x WT lanes (WT = the power of two >= the window count, at most 256): lane (rl, wl)
// walks the rows rl, rl + RT, ... of window wl (+ WT per chunk when there are more than 256 windows), so neighbouring lanes read
// overlapping windows of one row.  Every sum has a fixed order - rows ascending inside a lane, then the RT lanes of a window in
// lane order through LDS, then a tree over the 256 lanes for the scalar -: no atomics, bitwise reproducible.
// The all-windows-empty rule (:759-760: every likelihood 0) needs no pass of its own: a window without a valid step is NaN, NaN is
// outside (0, 1], and masked means over nothing are 0 - the same 0 the rule produces.
#include "kernels.h"

namespace ig {

namespace {

struct Hist { const float* edges; const float* logp; int nb; };

// bin of k_window_loglik: edges[i] <= x < edges[i + 1], the last bin closed on the right, anything else (or NaN) bin 0
__device__ __forceinline__ float hist_logp(const Hist& h, float x) {
  int b = 0;
  if (x >= h.edges[0] && x <= h.edges[h.nb]) {
    int lo = 0, hi = h.nb;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (x >= h.edges[mid]) lo = mid; else hi = mid; }
    b = lo;
  }
  return h.logp[b];
}

__device__ __forceinline__ bool unit_interval(float v) { return v > 0.f && v <= 1.f; }

}  // namespace

__global__ __launch_bounds__(256) void k_bundle_field(BundleScoreArgs a) {
  __shared__ float s_edges[65], s_logp[64];
  __shared__ float s_f[256];
  __shared__ int s_i[256];
  __shared__ int s_j[256];
  const int f = blockIdx.x, sc = blockIdx.y, tid = threadIdx.x;
  const float* tab = a.table + (size_t)f * BS_TABLE_STRIDE;
  const int nb = min(max((int)tab[0], 1), 64);            // (the entry cannot read the device table: keep the LDS copy in bounds)
  const float lo = tab[1], hi = tab[2];
  for (int i = tid; i <= nb; i += 256) s_edges[i] = tab[4 + i];
  for (int i = tid; i < nb; i += 256) s_logp[i] = tab[69 + i];
  __syncthreads();
  const Hist h{s_edges, s_logp, nb};
  const int W = a.W;
  float* scal = a.scalars + (size_t)sc * (BS_FIELDS + 2);
  float* lng = a.lng + ((size_t)sc * (BS_FIELDS + 1) + f) * W;

  if (f == 7 || f == 8) {
    // num_placement / num_removement: one row per rollout, every step counts; scalar = exp(sum of all / number of all)
    const long long* src = f == 7 ? a.n_place : a.n_remove;
    float tsum = 0.f;
    int tcnt = 0;
    for (int it = tid; it < a.R * W; it += 256) {
      const int r = it / W, w = it % W;
      const long long* v = src + (size_t)(sc * a.R + r) * a.ldn + (size_t)w * a.step2;
      float sum = 0.f;
      for (int k = 0; k < a.size2; ++k) sum += hist_logp(h, (float)v[k]);
      const float e = expf(sum / (float)a.size2);
      a.long_rollout[((size_t)(sc * a.R + r) * 2 + (f - 7)) * W + w] = e;
      if (r == 0) lng[w] = e;
      tsum += sum;
      tcnt += a.size2;
    }
    s_f[tid] = tsum; s_i[tid] = tcnt;
    __syncthreads();
    for (int off = 128; off; off >>= 1) {
      if (tid < off) { s_f[tid] += s_f[tid + off]; s_i[tid] += s_i[tid + off]; }
      __syncthreads();
    }
    if (tid == 0) {
      const float e = expf(s_f[0] / (float)s_i[0]);
      scal[f] = unit_interval(e) ? e : 0.f;
    }
    return;
  }

  int WT = 1;
  while (WT < W && WT < 256) WT <<= 1;
  const int RT = 256 / WT, wl = tid % WT, rl = tid / WT;
  const bool token_rate = f >= 9;
  const int size = token_rate ? a.size2 : a.size, step = token_rate ? a.step2 : a.step;
  const int ld = token_rate ? a.ld2 : a.ld;
  const float* values = f < 4 ? a.feat[f] : f == 4 ? a.dist : f == 6 ? a.ttc : f == 9 ? a.d_place : f == 10 ? a.d_remove : nullptr;
  const int T = a.T;
  float tsum = 0.f;      // scalar: sum of the likelihoods in (0, 1] (collision: of the log-likelihoods)
  int tcnt = 0;          //         their number (collision: the number of (object, window) pairs)
  int thit = 0;          // collision: pairs with a valid colliding step
  for (int w0 = 0; w0 < W; w0 += WT) {
    const int w = w0 + wl;
    float lsum = 0.f;
    int lcnt = 0;
    if (w < W) {
      for (int rp = rl; rp < a.R * a.N; rp += RT) {
        const int r = rp / a.N, i = rp % a.N, b = sc * a.R + r;
        if (i >= a.n_rows[b]) continue;                              // padding rows are never evaluated
        const size_t row = (size_t)b * a.N + i;
        const unsigned char* ok = a.valid + row * a.ld;
        const int t0 = w * step;
        float like;
        if (f == 5) {
          const unsigned char* col = a.collision + row * a.ld + t0;
          bool hit = false;
          for (int k = 0; k < size; ++k) hit = hit || (ok[t0 + k] && col[k]);
          const float ll = hist_logp(h, hit ? 1.f : 0.f);
          tsum += ll; ++tcnt; thit += hit;
          like = expf(ll);
        } else {
          const float* v = values + row * ld + t0;
          float sum = 0.f;
          int cnt = 0;
          for (int k = 0; k < size; ++k) {
            const int t = t0 + k;
            const float x = v[k];
            bool use;
            if (f == 0 || f == 2) use = t >= 1 && t <= T - 2 && ok[t + 1] && ok[t - 1];                       // speed validity
            else if (f == 1 || f == 3) use = t >= 2 && t <= T - 3 && ok[t + 2] && ok[t] && ok[t - 2];         // acceleration validity
            else if (f == 4) use = ok[t] && x >= lo && x <= hi;
            else if (f == 6) use = ok[t] != 0;
            else use = ok[t * a.shift] && x > lo && x < hi;            // token rate: the object's validity at the token's first step
            if (!use) continue;
            sum += hist_logp(h, x);
            ++cnt;
          }
          like = expf(sum / (float)cnt);                              // 0 / 0 = NaN for a window without a valid step
          if (unit_interval(like)) { tsum += like; ++tcnt; }
        }
        if (unit_interval(like)) { lsum += like; ++lcnt; }
      }
    }
    s_f[tid] = lsum; s_i[tid] = lcnt;
    __syncthreads();
    if (rl == 0 && w < W) {
      float s = 0.f;
      int c = 0;
      for (int q = 0; q < RT; ++q) { s += s_f[q * WT + wl]; c += s_i[q * WT + wl]; }
      lng[w] = s / (float)(c > 1 ? c : 1);
    }
    __syncthreads();
  }
  s_f[tid] = tsum; s_i[tid] = tcnt; s_j[tid] = thit;
  __syncthreads();
  for (int off = 128; off; off >>= 1) {
    if (tid < off) { s_f[tid] += s_f[tid + off]; s_i[tid] += s_i[tid + off]; s_j[tid] += s_j[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    if (f == 5) {
      const float e = expf(s_f[0] / (float)s_i[0]);                   // exp(mean log-likelihood of all pairs)
      scal[5] = unit_interval(e) ? e : 0.f;
      scal[BS_FIELDS + 1] = (float)s_j[0] / (float)s_i[0];           // simulated_collision_rate
    } else {
      scal[f] = s_f[0] / (float)(s_i[0] > 1 ? s_i[0] : 1);
    }
  }
}

__global__ __launch_bounds__(256) void k_bundle_meta(BundleScoreArgs a) {
  const int sc = blockIdx.x, tid = threadIdx.x, W = a.W;
  float* scal = a.scalars + (size_t)sc * (BS_FIELDS + 2);
  float* lng = a.lng + (size_t)sc * (BS_FIELDS + 1) * W;
  for (int w = tid; w < W; w += 256) {
    float acc = 0.f;
    bool zero = false;
    for (int f = 0; f < BS_FIELDS; ++f) {
      const float v = lng[(size_t)f * W + w];
      acc = acc + a.table[(size_t)f * BS_TABLE_STRIDE + 3] * v;
      zero = zero || v == 0.f;
    }
    lng[(size_t)BS_FIELDS * W + w] = zero ? 0.f : acc;
  }
  if (tid == 0) {
    double m = 0.0;
    for (int f = 0; f < BS_FIELDS; ++f) m += (double)a.table[(size_t)f * BS_TABLE_STRIDE + 3] * (double)scal[f];
    scal[BS_FIELDS] = (float)m;
  }
  if (sc == 0 && tid == 0) {
    int place = 0, remove = 0;
    for (int s = 0; s < a.S; ++s) {
      place += a.scalars[(size_t)s * (BS_FIELDS + 2) + 9] > 0.f;
      remove += a.scalars[(size_t)s * (BS_FIELDS + 2) + 10] > 0.f;
    }
    a.counters[0] = a.S; a.counters[1] = place; a.counters[2] = remove;
  }
}

}  // namespace ig
