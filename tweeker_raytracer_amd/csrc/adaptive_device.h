// Which launch indices an adaptive pass samples (twk_adaptive_select): the predicate over one element's luminance moments and sample
// count. The definition below is complete and is compiled once for the kernels (adaptive_kernels.hip) and once for the host
// (twk_adaptive_select_host, device_adaptive.hip); tests/adaptive_restate.py restates it statement for statement in numpy float32.
// Built with -ffp-contract=off (csrc/Makefile), like noise_device.h, whose classification it starts from.
//
// element i, (mean, M2, n, .) = moments[i], count = counts[i], parameters targetNoise (> 0, finite), minSamples (>= 2), darkFloor
// (> 0, finite), maxSamples (>= 1); c, e = noiseClassify(minSamples, darkFloor, moments[i]) (noise_device.h); the tests are applied
// in this order:
//   1. c == EMPTY             -> not selected  (the padding columns of a packed tile buffer, a pixel that was never sampled)
//   2. count >= maxSamples    -> not selected  (what ends a pixel that never becomes finite, and one that never meets the target)
//   3. c == UNKNOWN           -> selected      (too few samples to have an e, or a value that is not finite)
//   4. c == VALID             -> selected exactly when e > targetNoise (strict)
//
// The active list holds the selected i in ascending order: it equals numpy's flatnonzero of the predicate, whatever the grid.
//
// What this is not: a prediction of how many samples a pixel still needs (every selected pixel gets the same number per pass; the
// planned pass, adaptive_plan_device.h, starts from this predicate and adds that prediction), and, as the estimate it reads, it is blind to bias, to colour and to what a denoiser makes of the picture.
#pragma once
#include "noise_device.h"

namespace twk {

// TwkAdaptive (include/tweeker_hip.h) with the sample count as the float noiseClassify compares it as
struct AdaptiveConstants
{
  NoiseConstants noise; // (float) minSamples, darkFloor
  float targetNoise;
  unsigned int maxSamples;
};

TWK_HD bool adaptiveSelected(const AdaptiveConstants& k, const float4& m, const unsigned int count)
{
  float e;
  const int c = noiseClassify(k.noise, m, e);
  if (c == TWK_NOISE_EMPTY) return false;
  if (count >= k.maxSamples) return false;
  if (c == TWK_NOISE_UNKNOWN) return true;
  return e > k.targetNoise;
}

// The compaction (adaptive_kernels.hip) works on tiles of TWK_ADAPTIVE_TILE elements, one block of as many lanes per tile at a
// time: TWK_ADAPTIVE_TILE / 64 ballot words and one population count per tile.
#define TWK_ADAPTIVE_TILE 1024
#define TWK_ADAPTIVE_TILE_WAVES (TWK_ADAPTIVE_TILE / 64)

inline size_t adaptiveTiles(size_t numElements) { return (numElements + TWK_ADAPTIVE_TILE - 1) / TWK_ADAPTIVE_TILE; }
// Bytes of scan scratch for numElements elements: the ballot words, then per tile its count and its offset, then the total
inline size_t adaptiveScratchBytes(size_t numElements)
{
  const size_t tiles = adaptiveTiles(numElements);
  return tiles * TWK_ADAPTIVE_TILE_WAVES * sizeof(unsigned long long) + tiles * 2 * sizeof(unsigned int) + 4 * sizeof(unsigned int);
}

} // namespace twk
