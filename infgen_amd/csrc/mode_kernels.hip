// Modes from a scene's rollouts: the reference's batch_nms / new_batch_nms (infgen/utils/metrics.py:198-256, :143-195) on the device.
//   k_select_modes     one wave per row (an agent), lane j = candidate j (that agent in copy j), N <= 64 candidates, K <= 16 picks
// The reference sorts and copies the whole [B, N, T, F] tensor, builds two [B, N, N] distance tensors and issues about 8 launches
// per returned mode.  The selection needs one goal per candidate and K distance tests per candidate: the goals live in two VGPRs
// per lane, the density count and the rank are N v_readlane broadcasts each, every pick is one wave arg-max (a 64-bit max over
// __shfl_xor), one broadcast of the pick's goal and one distance test per lane.  No N x N matrix, no LDS allocation, no atomics,
// no scratch; the only bulk traffic is the K winning trajectories, copied 16 B per lane where the addresses allow.
//
// Pinned by definition where the reference leaves it open ("modes" of include/infgen_hip.h):
//   order      score descending, then candidate index ascending (the reference's argsort leaves ties open)
//   pick       the largest value among the unselected valid candidates, value = score if not covered, else 0; ties to the earlier
//              candidate of the order (the reference's point_val arg-max, for scores >= 0)
//   distance   fp32: sqrt(dx * dx + dy * dy) < dist_thresh, products and sum rounded separately (the file is built with
//              -ffp-contract=off), division and square root correctly rounded
//   validity   an invalid candidate is never picked, covers nothing and counts in no density; a row with fewer than K valid
//              candidates fills the rest with index -1, score 0 and a zero trajectory (the reference has no mask)
#include "kernels.h"

namespace ig {

namespace {

__device__ __forceinline__ float lane_f(float v, int lane) {                  // lane: wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__device__ __forceinline__ bool near(float ax, float ay, float bx, float by, float thresh) {
  const float dx = ax - bx, dy = ay - by;
  const float xx = dx * dx, yy = dy * dy;
  return sqrtf(xx + yy) < thresh;        // (sqrtf is correctly rounded here; __fsqrt_rn maps to the 1-ulp native square root)
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_select_modes(SelectModesArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long b = (long long)blockIdx.x * 4 + wv;                       // wave-uniform
  if (b >= a.B) return;
  const int N = a.N, K = a.K;
  const long long g = b / a.rows_per_group, r = b - g * a.rows_per_group;
  const float* row = a.traj + g * a.group_stride + r * a.row_stride;
  const bool in = lane < N;
  bool valid = in;
  if (in && a.cand_valid) valid = a.cand_valid[b * N + lane] != 0;
  if (in && a.cand_state) {
    const float s = a.cand_state[g * a.state_group_stride + r * a.state_row_stride + (long long)lane * a.state_cand_stride + a.t_goal];
    valid = valid && s != a.state_invalid && s != a.state_enter;
  }
  if (a.row_limit) valid = valid && r < (long long)a.row_limit[g * a.limit_stride];
  float gx = 0.f, gy = 0.f;
  if (in) {
    const float* p = row + (long long)lane * a.cand_stride + (long long)a.t_goal * a.step_stride;
    gx = p[0];
    gy = p[1];
  }
  const unsigned long long vmask = __ballot(valid);                           // wave-uniform

  float score = 0.f;
  if (a.score) {
    if (in) score = a.score[(a.score_per_group ? g : b) * N + lane] + 0.f;    // (-0 -> +0: the key below orders by the bits)
  } else {
    int cnt = 0;
    for (int i = 0; i < N; ++i) {
      const float xi = lane_f(gx, i), yi = lane_f(gy, i);
      if (((vmask >> i) & 1ull) && near(gx, gy, xi, yi, a.dist_thresh)) ++cnt;
    }
    score = valid ? __fdiv_rn((float)cnt, (float)N) : 0.f;
  }
  int rank = 0;                                                               // position in (score descending, index ascending)
  for (int i = 0; i < N; ++i) {
    const float si = lane_f(score, i);
    rank += (si > score || (si == score && i < lane)) ? 1 : 0;
  }

  bool selected = false, covered = false;
  for (int k = 0; k < K; ++k) {
    // value in the high word (a non-negative float orders like its bits), 64 - rank in the low one: the maximum is the largest
    // value and, among equals, the earliest of the order; 0 = not a candidate (64 - rank >= 1 for every lane below N)
    unsigned long long key = 0ull;
    if (valid && !selected)
      key = ((unsigned long long)(unsigned)__float_as_int(covered ? 0.f : score) << 32) | (unsigned long long)(64 - rank);
    const unsigned long long best = wave_max(key);
    const unsigned long long who = __ballot(key == best);
    const bool none = best == 0ull;
    const int p = none ? 0 : __builtin_amdgcn_readfirstlane(__ffsll((long long)who) - 1);       // < N: only valid lanes hold a key
    float* dst = a.mode_traj ? a.mode_traj + (b * K + k) * (long long)a.T * a.F : nullptr;
    const long long n = (long long)a.T * a.F;
    if (none) {
      if (lane == 0) { a.mode_idx[b * K + k] = -1; a.mode_score[b * K + k] = 0.f; }
      if (dst) for (long long e = lane; e < n; e += 64) dst[e] = 0.f;
      continue;
    }
    const float px = lane_f(gx, p), py = lane_f(gy, p), ps = lane_f(score, p);
    if (lane == p) selected = true;
    if (valid && (lane == p || near(gx, gy, px, py, a.dist_thresh))) covered = true;
    if (lane == 0) { a.mode_idx[b * K + k] = p; a.mode_score[b * K + k] = ps; }
    if (dst) {
      const float* src = row + (long long)p * a.cand_stride;
      if (a.step_stride == a.F) {                                             // one contiguous run of T F floats
        if ((((unsigned long long)src | (unsigned long long)dst) & 15ull) == 0ull) {
          const long long n4 = n >> 2;
          for (long long e = lane; e < n4; e += 64) ((float4*)dst)[e] = ((const float4*)src)[e];
          for (long long e = (n4 << 2) + lane; e < n; e += 64) dst[e] = src[e];
        } else {
          for (long long e = lane; e < n; e += 64) dst[e] = src[e];
        }
      } else {
        for (long long e = lane; e < n; e += 64) {
          const long long t = e / a.F, f = e - t * a.F;
          dst[e] = src[t * a.step_stride + f];
        }
      }
    }
  }
}

}  // namespace ig
