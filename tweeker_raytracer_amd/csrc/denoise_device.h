// The denoiser at the seam of Optix7Gui's optixDenoiserInvoke (apps/Optix7Gui/src/Application.cpp:942-1001): a CLASSICAL filter,
// the edge-avoiding a-trous wavelet of Dammertz, Sewtz, Hanika, Lensch, "Edge-Avoiding A-Trous Wavelet Transform for fast Global
// Illumination Filtering" (HPG 2010), guided by the albedo and camera-space normal AOVs. Nothing is learned and there is no
// network; the definition below is complete, and tests/test_gpu_denoise.py restates it statement for statement in numpy float32
// and compares bits. Built with -ffp-contract=off (csrc/Makefile): every operation below rounds once, as written.
//
// Streams, all f32, one float4 per pixel: colour (ping, pong), normal guide, albedo guide.
//
// prepare (pixel p):  b = widen(beauty[p]); a = widen(albedo[p]) (kinds with albedo); n = widen(normal[p]) (kind with normal)
//   demodulate:       d.k = fmaxf(a.k, 0.01f)  (a NaN albedo component gives 0.01);  c.k = b.k / d.k       k = x, y, z
//   otherwise:        c.k = b.k
//   colour[p] = (c.x, c.y, c.z, b.w);  the guides are stored as read (rgb, 0)
//
// level i, step s = 1 << i (pixel p = (x, y), colour in -> colour out):
//   cp = in[p]; if a component of cp.xyz, or of a guide in use at p (np.xyz, ap.xyz), is not finite: out[p] = cp, done
//   sum = (0, 0, 0); wsum = 0
//   for dy = -2 .. 2, for dx = -2 .. 2 (in this order, the centre included): q = (x + dx s, y + dy s), skipped when outside
//     cq = in[q]; skipped (weight 0) when a component of cq.xyz is not finite
//     e = cp - cq;            t = ((e.x e.x + e.y e.y) + e.z e.z) * invColor
//     normal in use:  e = np - nq;  t = t + ((e.x e.x + e.y e.y) + e.z e.z) * invNormal
//     albedo in use:  e = ap - aq;  t = t + ((e.x e.x + e.y e.y) + e.z e.z) * invAlbedo
//     w = (t <= 87) ? (h[dy + 2] * h[dx + 2]) * expP(-t) : 0          (NaN t: 0; expP(-t) is 0 beyond 87 anyway, one exp per tap)
//     sum.k = sum.k + w * cq.k;  wsum = wsum + w
//   out[p] = (sum.x / wsum, sum.y / wsum, sum.z / wsum, cp.w)
//   wsum >= 9/64: colour and guides of the centre are finite here, so its own tap has t = 0 (1 / sigma^2 is finite: twk_denoise
//   refuses a sigma whose square underflows) and weighs 9/64 exp(0). A tap whose guide is not finite has a NaN t: weight 0.
//   h = (1/16, 1/4, 3/8, 1/4, 1/16): every product h h is exact. invColor = 1.0f / (sigmaColor * sigmaColor), the same on
//   every level, invNormal and invAlbedo alike; computed once on the host in f32.
//
// finish (pixel p):  b = widen(beauty[p]);  c = colour[p] of the last level
//   demodulate: r.k = c.k * d.k with d as in prepare;  otherwise r.k = c.k
//   pass through, denoised[p] = beauty[p] (its bits), done, when a component is not finite of: b.xyz; a guide in use at p; r.xyz
//   (the last: a finite colour whose demodulated value b / d overflowed — it went through the levels as inf)
//   o.k = r.k + blendFactor * (b.k - r.k);  o.w = b.w;  denoised[p] = narrow(o) (RGBA16F: round to nearest even, once)
//
// iterations 0 or blendFactor 1: the host copies beauty to denoised, no kernel runs.
#pragma once
#include "device_math.h"

namespace twk {

struct DenoiseConstants
{
  int   width, height;
  float invColor, invNormal, invAlbedo; // 1 / sigma^2
  float blendFactor;
  int   demodulate;
};

TWK_HD bool finite3(const float4& c)
{
  // exponent field all ones = inf or NaN
  return ((asUint(c.x) & 0x7f800000u) != 0x7f800000u) && ((asUint(c.y) & 0x7f800000u) != 0x7f800000u) && ((asUint(c.z) & 0x7f800000u) != 0x7f800000u);
}

TWK_HD float distance2(const float4& a, const float4& b)
{
  const float ex = a.x - b.x, ey = a.y - b.y, ez = a.z - b.z;
  return (ex * ex + ey * ey) + ez * ez;
}

TWK_HD float stencilWeight(int d) // d = -2 .. 2: B3 spline 1/16, 1/4, 3/8, 1/4, 1/16
{
  return (d == 0) ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

TWK_HD float3 clampedAlbedo(const float4& a) { return make_float3(fmaxf(a.x, 0.01f), fmaxf(a.y, 0.01f), fmaxf(a.z, 0.01f)); }

// One tap of a level: folds colour cq at stencil offset (dx, dy) into sum / wsum. KIND: TWK_DENOISER_*
template<int KIND>
TWK_HD void denoiseTap(const DenoiseConstants& k, int dx, int dy, const float4& cp, const float4& np, const float4& ap,
                       const float4& cq, const float4& nq, const float4& aq, float& sx, float& sy, float& sz, float& wsum)
{
  if (!finite3(cq)) return;
  float t = distance2(cp, cq) * k.invColor;
  if (KIND >= 2) t = t + distance2(np, nq) * k.invNormal;
  if (KIND >= 1) t = t + distance2(ap, aq) * k.invAlbedo;
  if (!(t <= 87.0f)) return; // weight 0
  const float w = (stencilWeight(dy) * stencilWeight(dx)) * expP(-t);
  sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
  wsum = wsum + w;
}

} // namespace twk
