// The rectified temporal merge (twk_temporal_accumulate_rectified): temporal_device.h's merge with a per-pixel TRUST in its history.
// twk_update_light and twk_update_material leave the temporal history as it is, and the plain merge then blends up to maxHistory
// samples of the old lighting into every pixel. The merge measures history in SAMPLES, so the remedy is in samples too: decide per
// pixel how many of the history's samples are still worth having, and cap them there. Nothing of temporal_device.h changes; this
// header calls its functions (temporalGather, temporalHistory, temporalBlend) and adds only the trust between them. The definition
// below is complete and is compiled once for the kernels (temporal_rectify_kernels.hip) and once for the host
// (twk_temporal_rectify_host); tests/temporal_rectify_restate.py restates it statement for statement in numpy float32. All
// arithmetic is f32, every operation rounded once, in the order written (-ffp-contract=off, csrc/Makefile).
//
// Parameters (TwkTemporalRectify): radius R in 1..4, minTaps >= 2, gamma >= 0 and finite; g2 = gamma * gamma, once, on the host.
//
// ---- launch 1, reproject ----------------------------------------------------------------------------------------------------------
// pixel p: temporal_device.h's gather, temporalGather itself (temporalCandidate, temporalProject, the four taps in their order,
// temporalTapGeometry, temporalTap). With ws > 0 the quotients and the cap that open its merge, temporalHistory itself:
//   hx = sx / ws;  hy = sy / ws;  hz = sz / ws;  hmean = smean / ws;  hM2 = sM2 / ws;  hn = sn / ws
//   if hn > maxHistory:  hM2 = hM2 * (maxHistory / hn);  hn = maxHistory
// written to two f32 float4 scratch streams of the handle:  A[p] = (hx, hy, hz, 0);  B[p] = (hmean, hM2, hn, g.w)   (g.w: its bits)
// A pixel without history (no candidate, no projection, ws not > 0) gets A[p] = B[p] = (0, 0, 0, 0): hn = 0.
//
// ---- launch 2, test and merge -----------------------------------------------------------------------------------------------------
// Two words per pixel q, 0 outside the picture:
//   d_q   = mc_q.x - hmean_q                       the luminance means of the two moments streams: independent of the output format
//   key_q = the bits of g_q.w  if q is a candidate, hn_q > 0 and d_q is finite;  0 otherwise
//   (hn_q > 0 only where the gather ran, so "candidate" is implied, and the bits of g_q.w are B[q].w: the launch reads B and mc only)
// centre p with key_p != 0, the window of (2R+1)^2 taps q = p + (dx, dy), dy = -R..R outer, dx = -R..R inner (row-major); a tap
// COUNTS when key_q == key_p (the same instance; p counts itself; outside the picture key = 0 never counts):
//   pass 1:  m = number of counted taps;  S = S + d_q over them, from 0;   dbar = S / (float) m
//   pass 2:  ss = ss + (d_q - dbar) * (d_q - dbar) over them, in the same order, from 0
//   s2 = ss / (float) (m - 1);   b2 = dbar * dbar - g2 * (s2 / (float) m)
// trust t = 1 when key_p = 0, when m < minTaps (before any quotient), or when !(b2 > 0). Otherwise
//   rho = b2 / s2      (s2 = 0: +inf);      t = 1 / (1 + rho * (1 + hn / mc.z))      (rho = +inf: t = 0)
// hn' = hn * t;  hM2' = hM2 * t.
//   !(hn' > 0): the pixel PASSES THROUGH — colourOut[p] = colour[p] (its bits), historyOut[p] = cur, momentsOut[p] = mc — and
//     trustOut[p] = 0 if hn > 0 (the test, or the underflow of hn * t, took all of a history that was there), else t = 1 (nothing
//     was there and nothing was tested).
//   else the remaining statements of the plain merge, temporalBlend itself, with hn', hM2':
//     n = hn' + mc.z;  r = mc.z / n;  colour.k = h.k + (cur.k - h.k) * r;  d = mc.x - hmean;  mean = hmean + d * r;
//     M2 = (hM2' + mc.y) + (d * d) * (hn' * r);  outputs as temporal_device.h writes them;  trustOut[p] = t
// t = 1 gives hn' = hn and hM2' = hM2 exactly: where nothing is tested, every output has the bits of twk_temporal_accumulate.
// Two launches because the test at p needs the REPROJECTED history of p's neighbours, which only exists after every pixel gathered.
//
// Why the rule has this form.
//  * It is a paired test over the window. Frame and history look at the same surface: the difference d = frame - history cancels
//    the spatial structure (texture, shading gradients) the two share, so the window need not be flat, and what is left is the
//    noise of both plus any change of lighting. s2, the sample variance of d over the window, measures the noise of both at once:
//    s2 ~ sigma^2 (1 / n_c + 1 / hn), with sigma^2 the per-sample variance, n_c = mc.z the frame's samples and hn the history's.
//  * dbar is the mean difference, with standard error sqrt(s2 / m). b2 = dbar^2 - gamma^2 s2 / m is the squared bias that noise
//    cannot explain at gamma standard errors; where it is not positive the history is kept whole (t = 1).
//  * A history of hn samples that is biased by b has the mean squared error b^2 + sigma^2 / hn; the frame's mean is unbiased with
//    sigma^2 / n_c, and the two are independent. The weight w of the history that minimises the merged mean's squared error
//    w^2 (b^2 + sigma^2 / hn) + (1 - w)^2 sigma^2 / n_c is the inverse-error weight, which is the merge by count of a history of
//    hn' = sigma^2 / (b^2 + sigma^2 / hn) = hn / (1 + hn b^2 / sigma^2) samples. With sigma^2 recovered from s2,
//    hn b^2 / sigma^2 = (b2 / s2) (1 + hn / n_c) = rho (1 + hn / n_c): the t above.
//    M2 is scaled with the count, as the cap does, which leaves the history's sample variance M2 / n where it was.
// What it is not.
//  * Luminance only: d is a difference of luminance means. A hue change at equal luminance goes unseen.
//  * No temporal gradient that re-traces old seeds (Schied et al., "Gradient Estimation for Real-Time Adaptive Temporal Filtering",
//    A-SVGF): nothing is re-rendered, the test sees two independent noisy estimates, and it is BLIND below the window's noise — a
//    change smaller than gamma sqrt(s2 / m) keeps its stale history until the cap fades it.
//  * No colour clamp: the history's colour is never moved towards the neighbourhood's, only weighed less.
//  * The bias is taken as constant over the window and per instance: a shadow edge that moves inside one surface is averaged with
//    the unchanged part of the window around it.
#pragma once
#include "temporal_device.h"

namespace twk {

#define TWK_RECTIFY_MAX_RADIUS 4
#define TWK_RECTIFY_TILE_X 32
#define TWK_RECTIFY_TILE_Y 8

struct RectifyConstants
{
  int   radius, minTaps;
  float gamma2; // gamma * gamma
};

// Launch 1 at one pixel: the reprojected, capped history as the two scratch words A = (hx, hy, hz, 0), B = (hmean, hM2, hn, g.w).
// Moving: temporalGather's Moving build (temporal_motion_device.h); launch 2 is the same for both.
// Carried: temporalGather's Carried build (temporal_carry_device.h; carried: the plane's element of this pixel).
template<bool Moving = false, bool Carried = false>
TWK_HD void rectifyReproject(const TemporalConstants& k, const float4& cur, const float4& mc, const float4& g, const float4* historyColour, const float4* historyMoments,
                             const float4* historyGeometry, float4& A, float4& B, const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u,
                             const float4 carried = make_float4(0.0f, 0.0f, 0.0f, 0.0f))
{
  A = make_float4(0.0f, 0.0f, 0.0f, 0.0f); B = A;
  if (k.hasHistory == 0) return;
  TemporalSums s;
  temporalGather<Moving, Carried>(k, cur, mc, g, historyColour, historyMoments, historyGeometry, s, motion, numMotion, carried);
  if (!(s.ws > 0.0f)) return;
  const TemporalHistory h = temporalHistory(k, s);
  A.x = h.x; A.y = h.y; A.z = h.z;
  B = make_float4(h.mean, h.M2, h.n, g.w);
}

// The two staged words of pixel q from its moments and its scratch word B
TWK_HD void rectifyStage(const float4& mc, const float4& B, float& d, unsigned int& key)
{
  d = mc.x - B.x;
  key = (B.z > 0.0f && finite1(d)) ? asUint(B.w) : 0u;
}

// The trust of the centre at index `centre` of the staged words d, key, laid out in rows of `pitch` words with at least R words and
// R rows of halo around it. R > 0: the radius at compile time (the window loops unroll); R = 0: r.radius.
template<int R>
TWK_HD float rectifyTrust(const RectifyConstants& r, const float* d, const unsigned int* key, int pitch, int centre, float hn, float mcz)
{
  const unsigned int kp = key[centre];
  if (kp == 0u) return 1.0f;
  const int radius = R > 0 ? R : r.radius;
  int m = 0;
  float sum = 0.0f;
  for (int dy = -radius; dy <= radius; ++dy)
    for (int dx = -radius; dx <= radius; ++dx)
    {
      const int q = centre + dy * pitch + dx;
      if (key[q] == kp) { ++m; sum = sum + d[q]; }
    }
  if (m < r.minTaps) return 1.0f;
  const float fm = (float) m;
  const float dbar = sum / fm;
  float ss = 0.0f;
  for (int dy = -radius; dy <= radius; ++dy)
    for (int dx = -radius; dx <= radius; ++dx)
    {
      const int q = centre + dy * pitch + dx;
      if (key[q] == kp) { const float e = d[q] - dbar; ss = ss + e * e; }
    }
  const float s2 = ss / (float) (m - 1);
  const float b2 = dbar * dbar - r.gamma2 * (s2 / fm);
  if (!(b2 > 0.0f)) return 1.0f;
  const float rho = b2 / s2;
  return 1.0f / (1.0f + rho * (1.0f + hn / mcz));
}

// Launch 2's merge at one pixel, the trust t known: false = pass through (the caller writes the frame's bits); trust = trustOut[p]
TWK_HD bool rectifyMerge(float t, const float4& cur, const float4& mc, const float4& A, const float4& B, float4& colour, float4& moments, float& trust)
{
  TemporalHistory h;
  h.x = A.x; h.y = A.y; h.z = A.z; h.mean = B.x;
  h.n = B.z * t; h.M2 = B.y * t;
  if (!(h.n > 0.0f)) { trust = (B.z > 0.0f) ? 0.0f : t; return false; }
  temporalBlend(h, cur, mc, colour, moments);
  trust = t;
  return true;
}

} // namespace twk
