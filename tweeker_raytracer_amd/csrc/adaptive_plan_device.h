// How many samples a planned adaptive pass gives each launch index it samples (twk_adaptive_plan): the budget of one element from its
// luminance moments and sample count. The definition below is complete and is compiled once for the kernels
// (adaptive_plan_kernels.hip) and once for the host (twk_adaptive_plan_host, device_adaptive.hip); tests/adaptive_plan_restate.py
// restates it statement for statement in numpy float32. Built with -ffp-contract=off (csrc/Makefile), like adaptive_device.h, whose
// predicate decides who is in the plan at all.
//
// element i, m = (mean, M2, n, .) = moments[i], count = counts[i], the parameters of adaptiveSelected (adaptive_device.h) and
// minBatch, maxBatch (1 <= minBatch <= maxBatch <= 64: twk_launch_adaptive's own limit, a planned pass is never larger than a pass
// that call allows); c, e = noiseClassify(minSamples, darkFloor, m) (noise_device.h). The budget b of the element, in this order:
//   1. adaptiveSelected(k, m, count) is false  -> b = 0        (the planned list IS the select's list for the same parameters)
//   2. c == UNKNOWN                            -> b = minBatch (with minBatch = minSamples one pass makes the pixel classifiable)
//   3. c == VALID: e is the standard error of a mean of n samples and falls as 1 / sqrt(n), so the element reaches the target at
//      about n (e / target)^2 samples. In float32, every operation rounded once:
//        r = e / targetNoise;  q = r * r;  need = n * q;  extra = need - n
//        b = !(extra < (float) maxBatch) ? maxBatch : (uint32) ceilf(extra)      (the negated comparison sends inf and NaN to maxBatch)
//        b = max(b, minBatch)
//      e > targetNoise (test 4 of adaptiveSelected) makes r >= 1, q >= 1, need >= n, extra >= 0: the conversion is of a value in [0, 64).
//   4. b = min(b, maxSamples - count)          (>= 1: test 2 of adaptiveSelected has removed count >= maxSamples)
//
// The plan of numElements elements, every word an integer and a pure function of the input, whatever the grid:
//   active[k]      the i with b > 0, ascending (numpy's flatnonzero(b > 0)), numActive of them
//   pathOffset[k]  the exclusive prefix sum of b[active[.]], numActive + 1 words: pathOffset[numActive] = numPaths
// The paths of entry k of a planned pass are pathOffset[k] .. pathOffset[k + 1] - 1, sample s at iteration count[active[k]] + s.
//
// What this is not: a guarantee. It assumes e falls as 1 / sqrt(n); the estimate is low where samples are few
// (profiles/r12_noise.md), so early plans under-allocate and the loop's next plan corrects them. As the estimate it reads it is
// a statistic of the luminance, blind to bias, to colour and to what a denoiser makes of the picture.
#pragma once
#include "adaptive_device.h"

namespace twk {

// TwkAdaptivePlan (include/tweeker_hip.h)
struct AdaptivePlanConstants
{
  unsigned int minBatch, maxBatch;
};

#define TWK_ADAPTIVE_PLAN_MAX_BATCH 64u // twk_launch_adaptive's limit on the samples of a pass

TWK_HD unsigned int adaptiveBudget(const AdaptiveConstants& k, const AdaptivePlanConstants& plan, const float4& m, const unsigned int count)
{
  if (!adaptiveSelected(k, m, count)) return 0u;
  float e;
  const int c = noiseClassify(k.noise, m, e);
  unsigned int b = plan.minBatch;
  if (c == TWK_NOISE_VALID)
  {
    const float r = e / k.targetNoise;
    const float q = r * r;
    const float need = m.z * q;
    const float extra = need - m.z;
    b = !(extra < (float) plan.maxBatch) ? plan.maxBatch : (unsigned int) ceilf(extra);
    if (b < plan.minBatch) b = plan.minBatch;
  }
  const unsigned int left = k.maxSamples - count;
  return b < left ? b : left;
}

// Bytes of scratch of a plan of numElements elements (adaptive_plan_kernels.hip launchAdaptivePlan carves it in this order, every
// part aligned to 8): the ballot words; per tile the 64-bit offset of its first path; the two totals (numPaths, numActive) as 64-bit
// words; per tile its population count, its offset in the list and its budget sum (at most 64 x 1024); the budget of every element, a byte.
inline size_t adaptivePlanScratchBytes(size_t numElements)
{
  const size_t tiles = adaptiveTiles(numElements);
  const size_t words64 = tiles * TWK_ADAPTIVE_TILE_WAVES + tiles + 2;
  const size_t words32 = (tiles * 3 + 1) & ~(size_t) 1;
  return words64 * sizeof(unsigned long long) + words32 * sizeof(unsigned int) + ((numElements + 7) & ~(size_t) 7);
}

} // namespace twk
