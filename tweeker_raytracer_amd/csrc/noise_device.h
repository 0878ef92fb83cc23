// How noisy a frame still is, from the integrator's own samples: the relative standard error of every pixel's luminance mean,
// classified and summarised in integers (twk_estimate_noise). The input is the stream of luminance moments (mean, M2, n, .) that
// shade_device.h foldSamples accumulates per launch index (twk_enable_moments). The definition below is complete and is compiled
// for the kernel (noise_kernels.hip) and for the host helpers (device_post.hip); tests/noise_restate.py restates it statement for
// statement in numpy float32 and tests/test_gpu_noise.py compares every field. Built with -ffp-contract=off (csrc/Makefile): every
// operation rounds once, as written; the division and the square root are the correctly rounded IEEE operations, the ones
// denoise_device.h momentsFinish uses.
//
// element i, (mean, M2, n, .) = moments[i], parameters minSamples (>= 2, compared as a float) and darkFloor (> 0, finite); the
// tests are applied in this order:
//   1. n == 0                                                                   -> EMPTY    (the padding columns of a packed tile
//      buffer, a pixel whose samples were all dropped; -0 is 0)
//   2. mean, M2 or n not finite, or n < minSamples, or M2 < 0, or mean < 0      -> UNKNOWN  (a NaN n fails test 1 and lands here)
//   3. otherwise VALID:
//        d = (n - 1) * n;  v = M2 / d;  s = sqrtf(v);  e = s / (mean + darkFloor)
//      e not finite -> UNKNOWN. e is the relative standard error of the pixel's mean: v is the variance of the mean of n samples,
//      the same M2 / ((n - 1) n) twk_denoise_variance_sampled is guided by; darkFloor keeps a black pixel from dividing by 0.
//      n >= 2 makes d >= 2, M2 >= 0 makes v >= 0, mean >= 0 makes the divisor > 0: e >= 0. A M2 of -0 passes test 2 (-0 < 0 is
//      false) and would give e = -0; the sign bit of e is cleared, which changes no other value.
//
// The summary (TwkNoiseSummary, include/tweeker_hip.h) holds integers only, so it does not depend on the order the elements are
// reduced in:
//   valid, unknown, empty   counts; they sum to the number of elements
//   histogram[bin]          valid elements by bin = clamp((bits(e) >> 20) - ((127 - 16) << 3), 0, 255): the exponent and the top
//                           three mantissa bits of e, 8 bins per octave from 2^-16 to 2^16, monotonic in e, no logarithm
//   sumFixed                sum over the valid elements of (uint64) rintf(fminf(e, 65536.0f) * 1048576.0f): e in units of 2^-20,
//                           the product exact in f32 (a power of two; a denormal e stays on its grid), at most 2^36 per element
//   maxErrorBits            the largest bits(e): e >= 0, so the order of the bits is the order of the values
// The error map, where asked for, is one f32 per element: e for a VALID element, -1 for UNKNOWN, -2 for EMPTY.
//
// Two summaries of disjoint element sets merge by adding counts, histogram and sumFixed and taking the larger maxErrorBits
// (noiseMerge): devices reduce their own packed tile buffers and the host merges, no picture is assembled.
//
// The quantile q in (0, 1] of a summary with valid > 0 (noiseQuantileBin): the first bin at which the cumulative count reaches
// need = ceil(q * valid), the ceiling in exact integer arithmetic: q is a float, m * 2^x with m an integer below 2^24, so
// q * valid = (m * valid) * 2^x with x <= -23 and a product below 2^88 (unsigned __int128). What is returned is the bin's UPPER edge,
// asFloat((bin + 1 + ((127 - 16) << 3)) << 20): never below the true quantile, and at most 9/8 of it inside the histogram's range
// (a bin spans a factor of at most 9/8). Bin 255 holds everything from 2^15 * 15/8 up, its edge is 2^16: above 2^16 the edge is below the value.
//
// What this is not: an error against ground truth. It sees the spread of the samples the integrator kept, so it is blind to bias
// (clamped paths, a firefly clamp, a path length limit), it says nothing of a denoised picture, and it is a statistic of the
// luminance, not of the colour.
#pragma once
#include "denoise_device.h"
#include "device_types.h" // NoiseConstants; TwkNoiseSummary (include/tweeker_hip.h)

namespace twk {

#define TWK_NOISE_VALID   0
#define TWK_NOISE_UNKNOWN 1
#define TWK_NOISE_EMPTY   2
#define TWK_NOISE_BIN_BASE ((127 - 16) << 3)

// The class of one element and, for a VALID one, its e
TWK_HD int noiseClassify(const NoiseConstants& k, const float4& m, float& e)
{
  e = 0.0f;
  if (m.z == 0.0f) return TWK_NOISE_EMPTY;
  if (!finite1(m.x) || !finite1(m.y) || !finite1(m.z) || m.z < k.minSamples || m.y < 0.0f || m.x < 0.0f) return TWK_NOISE_UNKNOWN;
  const float d = (m.z - 1.0f) * m.z;
  const float v = m.y / d;
  const float s = sqrtf(v);
  e = asFloat(asUint(s / (m.x + k.darkFloor)) & 0x7fffffffu);
  if (!finite1(e)) { e = 0.0f; return TWK_NOISE_UNKNOWN; }
  return TWK_NOISE_VALID;
}

TWK_HD int noiseBin(float e)
{
  const int b = (int) (asUint(e) >> 20) - TWK_NOISE_BIN_BASE;
  return b < 0 ? 0 : (b > 255 ? 255 : b);
}

TWK_HD unsigned long long noiseFixed(float e) { return (unsigned long long) rintf(fminf(e, 65536.0f) * 1048576.0f); }

// What the error map holds for an element of class c
TWK_HD float noiseMapValue(int c, float e) { return c == TWK_NOISE_VALID ? e : (c == TWK_NOISE_UNKNOWN ? -1.0f : -2.0f); }

TWK_HD float noiseBinUpperEdge(int bin) { return asFloat((uint32_t) (bin + 1 + TWK_NOISE_BIN_BASE) << 20); }

// ---- host side: merge, mean, quantile ---------------------------------------------------------------------------------------
inline void noiseMerge(TwkNoiseSummary& into, const TwkNoiseSummary& other)
{
  into.valid += other.valid; into.unknown += other.unknown; into.empty += other.empty; into.sumFixed += other.sumFixed;
  if (other.maxErrorBits > into.maxErrorBits) into.maxErrorBits = other.maxErrorBits;
  for (int b = 0; b < 256; ++b) into.histogram[b] += other.histogram[b];
}

// sumFixed / 2^20 / valid in double, narrowed once (valid > 0)
inline float noiseMean(const TwkNoiseSummary& s) { return (float) ((double) s.sumFixed / 1048576.0 / (double) s.valid); }

// ceil(q * valid) for a float q in (0, 1], exactly (shift is in [-149, -23])
inline uint64_t noiseQuantileCount(float q, uint64_t valid)
{
  const uint32_t bits = asUint(q);
  const int exponent = (int) (bits >> 23);
  const uint64_t mantissa = exponent ? ((bits & 0x7fffffu) | 0x800000u) : (bits & 0x7fffffu); // q = mantissa * 2^shift
  const int shift = (exponent ? exponent : 1) - 150;
  const unsigned __int128 product = (unsigned __int128) mantissa * valid;
  if (-shift >= 128) return product ? 1 : 0;
  const unsigned __int128 whole = product >> -shift;
  const bool rest = (whole << -shift) != product;
  return (uint64_t) whole + (rest ? 1 : 0);
}

// The first bin at which the cumulative count reaches ceil(q * valid); q in (0, 1], valid > 0 and equal to the histogram's sum
inline int noiseQuantileBin(const TwkNoiseSummary& s, float q)
{
  const uint64_t need = noiseQuantileCount(q, s.valid);
  uint64_t seen = 0;
  for (int b = 0; b < 256; ++b)
  {
    seen += s.histogram[b];
    if (seen >= need) return b;
  }
  return 255;
}

} // namespace twk
