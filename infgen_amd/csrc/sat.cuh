// The separating-axis value of two oriented rectangles, shared by the step riders (rider.cuh, k_step_score; include/infgen_hip.h,
// "collision masks" / "road masks" / "step scores"): the candidate A has the heading (ca, sa) and the half extents (hla, hwa), the obstacle B the heading (cb, sb)
// and the half extents (hlb, hwb); (ddx, ddy) is B's centre minus A's, all in one frame.  Returns the maximum over the four axes of
// |projected centre distance| - the sum of the projected half extents: the rectangles overlap iff the value is < 0.
// fp32, no fused multiply-add (the build's -ffp-contract=off): the order of the operations below is part of the definition's bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ig {

__device__ __forceinline__ float sat_sep(float ddx, float ddy, float ca, float sa, float hla, float hwa, float cb, float sb, float hlb,
                                         float hwb) {
  const float cc = fabsf(ca * cb + sa * sb), ss = fabsf(sb * ca - cb * sa);      // |cos|, |sin| of the relative heading
  const float s0 = fabsf(ddx * ca + ddy * sa) - (hla + (hlb * cc + hwb * ss));
  const float s1 = fabsf(ddy * ca - ddx * sa) - (hwa + (hlb * ss + hwb * cc));
  const float s2 = fabsf(ddx * cb + ddy * sb) - (hlb + (hla * cc + hwa * ss));
  const float s3 = fabsf(ddy * cb - ddx * sb) - (hwb + (hla * ss + hwa * cc));
  return fmaxf(fmaxf(s0, s1), fmaxf(s2, s3));
}

}  // namespace ig
