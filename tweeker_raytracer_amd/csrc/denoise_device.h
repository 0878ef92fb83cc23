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
//
// ---- the variance-guided mode (twk_denoise_variance) ------------------------------------------------------------------------
// The spatial-variance path of Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017, sections 4.2 and 4.4), used
// there when no temporal history exists: a per-pixel variance of the luminance estimated from the picture itself scales the
// colour edge-stop, and a clamp against the same estimate pulls fireflies down. Still nothing learned, and no per-sample variance:
// the estimate is spatial. tests/test_gpu_denoise_variance.py restates what follows in numpy float32 and compares bits.
// prepare and finish are the ones above; the variance rides in .w of the colour streams (finish takes alpha from beauty).
//
//   lum(c) = (0.2126f c.x + 0.7152f c.y) + 0.0722f c.z
//   finiteV(c): c.xyz finite and lum(c) finite (a finite colour near FLT_MAX can have an infinite luminance)
//
// moments (pixel p = (x, y), colour of prepare in -> colour out; runs once, before level 0; R = 3):
//   cp = in[p]; if !finiteV(cp), or a guide in use at p is not finite: out[p] = (cp.xyz, 0), done
//   s0 = s1 = s2 = 0
//   for dy = -3 .. 3, for dx = -3 .. 3 (in this order, the centre LEFT OUT): q = (x + dx, y + dy), skipped when outside
//     cq = in[q]; skipped when a component of cq.xyz is not finite
//     RGB_ALBEDO_NORMAL: t = distance2(np, nq) * invNormal + distance2(ap, aq) * invAlbedo;  RGB_ALBEDO: t = distance2(ap, aq) * invAlbedo
//     skipped unless t <= 87 (NaN t: a guide of q that is not finite);  g = expP(-t);            RGB: no t, g = 1
//     l = lum(cq);  s0 = s0 + g;  s1 = s1 + g * l;  s2 = s2 + g * (l * l)
//   no tap counted (s0 == 0): out[p] = (cp.xyz, 0), done (no variance, no clamp)
//   m1 = s1 / s0;  m2 = s2 / s0;  var = fmaxf(m2 - m1 * m1, 0)     (fmaxf: a NaN difference, inf - inf, gives 0)
//   fireflyThreshold > 0:  limit = m1 + fireflyThreshold * sqrtf(var);  lp = lum(cp)
//     if lp > limit and limit > 0:  f = limit / lp;  cp.k = cp.k * f   k = x, y, z
//   out[p] = (cp.xyz, var)
//
// level i, step s = 1 << i (colour in -> colour out), what differs from the level above:
//   cp = in[p]; passes through (out[p] = cp) also when lum(cp) is not finite;  lp = lum(cp)
//   vs = 0; bs = 0;  for dy = -1 .. 1, for dx = -1 .. 1 (in this order): q = (x + dx s, y + dy s), skipped when outside
//     cq = in[q]; skipped when a component of cq.xyz or cq.w is not finite
//     b = b3[dy + 1] * b3[dx + 1], b3 = (1/4, 1/2, 1/4);  vs = vs + b * cq.w;  bs = bs + b
//   vbar = (bs > 0) ? vs / bs : 0;   invL = 1.0f / (sigmaLuminance * sqrtf(vbar) + 1e-3f)        (epsilon = 1e-3f: in (0, 1000])
//   per tap, instead of the colour term:  t = fabsf(lp - lum(cq)) * invL;  then the guide terms, the cut-off and w as above
//     sum.k = sum.k + w * cq.k;  wsum = wsum + w;  vsum = vsum + (w * w) * cq.w
//   out[p] = (sum.x / wsum, sum.y / wsum, sum.z / wsum, vsum / (wsum * wsum))
//   wsum >= 9/64 still: the centre's own tap has t = 0 * invL = 0, lp being finite.
//
// ---- the sampled variance (twk_denoise_variance_sampled) -------------------------------------------------------------------
// SVGF's rule the other way round: where the integrator has seen enough samples of a pixel, the variance the levels are guided
// by is the MEASURED variance of the pixel's mean, from the luminance moments the accumulate kernels fold (shade_device.h
// foldSamples: one float4 (mean, M2, n, 0) per pixel, Welford over the luminance of the raw samples); elsewhere the spatial
// estimate above stays (SVGF section 4.2 falls back the same way). Everything is the variance-guided mode except the value the
// moments pass writes into .w. tests/test_gpu_denoise_sampled.py restates it in numpy float32 and compares bits.
//
// moments pass, SAMPLED build, for a pixel that reaches the sums (finiteV(cp) and finite guides; the early (cp.xyz, 0) stays):
//   var, and the clamp factor f, as above; f = 1 where no clamp applied, var = 0 and f = 1 where no tap counted (s0 == 0)
//   (mean, M2, n, .) = moments[p]                                                    (one more coalesced 16-byte load)
//   if n >= minSamples and mean, M2, n are finite and mean > 0:
//     v = M2 / ((n - 1) * n)                                   (variance of the mean of n samples; minSamples >= 2, so n - 1 >= 1)
//     demodulate:  rho = lum(cp) / mean  (cp BEFORE the clamp);  v = v * (rho * rho)       (into the demodulated space of the levels)
//     var = v * (f * f)                                                                  (the clamp scaled the colour by f)
//   out[p] = (cp.xyz clamped as above, var)
// The clamp itself stays spatial: a firefly raises its own sample variance and must not vouch for itself. A product that
// overflows gives an infinite (0 * inf: NaN) var, which the levels' variance blur skips like any other that is not finite.
//
// ---- the geometry guide (twk_denoise_geometry) -------------------------------------------------------------------------------
// The geometric half of SVGF's edge-stopping function (Schied et al. 2017, section 4.4) as a fourth guide of the three modes
// above, for inputKind RGB_ALBEDO_NORMAL only: a tap is weighed down by its distance from the centre's tangent plane, and, on
// request, cut off at another instance. tests/denoise_geometry_restate.py restates it in numpy float32 and compares bits.
// Further inputs: the geometry AOV, one float4 per pixel, always f32 and read where it lies (no staging copy in prepare):
// (world position, bits of instance + 1), a miss (0, 0, 0, bits 0); and the camera it was traced from, P, U, V, W.
//
// host, once per call, in f32:  Un, Vn, Wn = normalize(U), normalize(V), normalize(W) (device_math.h; shade_device.h writes the
//   normal AOV as (N.Un, N.Vn, -N.Wn) with the same three);  invPosition = 1.0f / (sigmaPosition * sigmaPosition)
//   (refused unless invPosition is a finite positive float and Un, Vn, Wn are finite)
//   dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z
//
// centre p, in the levels and in the moments pass, after the existing pass-through tests (np is finite here):
//   gp = geometry[p];  a miss centre (bits(gp.w) == 0): no plane term, N and invG are not used
//   a hit centre:  v = gp.xyz - P;  vv = dot3(v, v)
//     N.k = (Un.k * np.x + Vn.k * np.y) - Wn.k * np.z      k = x, y, z     (the world-space normal back from the normal guide; NOT
//       renormalised: an averaged normal shorter than 1 only weakens the stop)
//     invG = invPosition / vv
//     the pixel passes through the pass exactly as for a guide that is not finite (level: out[p] = cp; moments: out[p] =
//     (cp.xyz, 0)) when gp.xyz is not finite, when vv is zero or not finite, or when N or invG is not finite. prepare and finish
//     do not read the geometry: such a pixel's unfiltered colour goes through finish like any other.
//     (The last two are added to the first statement of this guide: a tiny vv makes invG inf and a huge finite np makes N inf,
//     and then the centre's own tap would have d = 0, (d * d) * invG = NaN or d = 0 * inf = NaN, weight 0, and wsum could be 0.
//     With them the centre's own tap adds exactly 0 and wsum >= 9/64 stands.)
//
// tap q, one more term in t after the albedo term and before the t <= 87 cut-off (denoiseTap, denoiseVarianceTap, momentsTap):
//   gq = geometry[q];  exactly one of bits(gp.w), bits(gq.w) is 0 (hit and miss never mix): weight 0
//   both 0: nothing is added
//   both hits:  instanceStop and bits(gp.w) != bits(gq.w): weight 0
//     e = gq.xyz - gp.xyz;  d = dot3(e, N);  t = t + (d * d) * invG          (a NaN t gives weight 0, as above)
// On a plane d is 0 at every step, so the term is not scaled by the level's step. sigmaPosition is a distance from the centre's
// tangent plane relative to the centre's distance from the camera: TwkTemporal::positionTolerance's convention.
// With a geometry of misses only, every tap adds nothing and the three modes compute the bits they compute without the guide.
//
// ---- where this is written down -----------------------------------------------------------------------------------------------
// The statements above exist once in C++, at the end of this file: denoisePreparePixel, denoiseMomentsPixel, denoiseLevelPixel and
// denoiseFinishPixel are what one pixel does in a pass, over the per-tap functions (denoiseTap, denoiseVarianceTap, momentsTap, ...).
// The level and the moments body read their taps through a tap source, which alone knows where a tap lies and which taps exist.
// Both builds of the level kernel and the moments kernel (denoise_kernels.hip: DenoiseGlobalTaps on the streams, DenoiseStagedTaps
// on a block's LDS arrays) and the host form twk_denoise_geometry_host (device_post.hip: DenoiseGlobalTaps on host pointers) call
// these same bodies; none restates a loop, a skip rule or a pass-through rule. The only other statements of the definition are
// the numpy ones of the tests: tests/test_gpu_denoise.py, test_gpu_denoise_variance.py, test_gpu_denoise_sampled.py and
// tests/denoise_geometry_restate.py.
#pragma once
#include "device_math.h"

namespace twk {

struct DenoiseConstants
{
  int   width, height;
  float invColor, invNormal, invAlbedo; // 1 / sigma^2
  float blendFactor;
  int   demodulate;
  float fireflyThreshold, sigmaLuminance; // the variance-guided mode only
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

TWK_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

TWK_HD bool finite1(float v) { return (asUint(v) & 0x7f800000u) != 0x7f800000u; }

// ---- the geometry guide ----
struct DenoiseGeometryConstants
{
  float P[3], Un[3], Vn[3], Wn[3]; // the camera the geometry AOV was traced from, U, V, W normalised
  float invPosition;               // 1 / sigmaPosition^2
  int   instanceStop;
};

// The host's part: cam = P, U, V, W (12 floats). False: the call is refused (sigmaPosition, or a camera vector that does not normalise).
TWK_HD bool denoiseGeometryConstants(const float* cam, float sigmaPosition, int instanceStop, DenoiseGeometryConstants& g)
{
  const V3 Un = normalize(v3(cam[3], cam[4], cam[5])), Vn = normalize(v3(cam[6], cam[7], cam[8])), Wn = normalize(v3(cam[9], cam[10], cam[11]));
  g.P[0] = cam[0]; g.P[1] = cam[1]; g.P[2] = cam[2];
  g.Un[0] = Un.x; g.Un[1] = Un.y; g.Un[2] = Un.z;
  g.Vn[0] = Vn.x; g.Vn[1] = Vn.y; g.Vn[2] = Vn.z;
  g.Wn[0] = Wn.x; g.Wn[1] = Wn.y; g.Wn[2] = Wn.z;
  g.invPosition = 1.0f / (sigmaPosition * sigmaPosition);
  g.instanceStop = instanceStop ? 1 : 0;
  bool ok = finite1(g.invPosition) && g.invPosition > 0.0f;
  for (int i = 0; i < 3; ++i) ok = ok && finite1(g.P[i]) && finite1(g.Un[i]) && finite1(g.Vn[i]) && finite1(g.Wn[i]);
  return ok;
}

// What a centre keeps for its taps, computed once per thread
struct DenoiseGeometryCentre
{
  float4 gp;
  float  nx, ny, nz, invG;
  int    instanceStop;
};

// False: the pixel passes through
TWK_HD bool denoiseGeometryCentre(const DenoiseGeometryConstants& g, const float4& gp, const float4& np, DenoiseGeometryCentre& c)
{
  c.gp = gp; c.nx = 0.0f; c.ny = 0.0f; c.nz = 0.0f; c.invG = 0.0f; c.instanceStop = g.instanceStop;
  if (asUint(gp.w) == 0u) return true; // a miss: no plane term
  if (!finite3(gp)) return false;
  const float vx = gp.x - g.P[0], vy = gp.y - g.P[1], vz = gp.z - g.P[2];
  const float vv = dot3(vx, vy, vz, vx, vy, vz);
  if (!finite1(vv) || vv == 0.0f) return false;
  c.nx = (g.Un[0] * np.x + g.Vn[0] * np.y) - g.Wn[0] * np.z;
  c.ny = (g.Un[1] * np.x + g.Vn[1] * np.y) - g.Wn[1] * np.z;
  c.nz = (g.Un[2] * np.x + g.Vn[2] * np.y) - g.Wn[2] * np.z;
  c.invG = g.invPosition / vv;
  return finite1(c.nx) && finite1(c.ny) && finite1(c.nz) && finite1(c.invG);
}

// The term of tap gq, added to t. False: weight 0
TWK_HD bool denoiseGeometryTap(const DenoiseGeometryCentre& c, const float4& gq, float& t)
{
  const uint32_t bp = asUint(c.gp.w), bq = asUint(gq.w);
  if ((bp == 0u) != (bq == 0u)) return false; // hit and miss never mix
  if (bp == 0u) return true;
  if (c.instanceStop && bp != bq) return false;
  const float d = dot3(gq.x - c.gp.x, gq.y - c.gp.y, gq.z - c.gp.z, c.nx, c.ny, c.nz);
  t = t + (d * d) * c.invG;
  return true;
}

TWK_HD float stencilWeight(int d) // d = -2 .. 2: B3 spline 1/16, 1/4, 3/8, 1/4, 1/16
{
  return (d == 0) ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

TWK_HD float3 clampedAlbedo(const float4& a) { return make_float3(fmaxf(a.x, 0.01f), fmaxf(a.y, 0.01f), fmaxf(a.z, 0.01f)); }

// One tap of a level: folds colour cq at stencil offset (dx, dy) into sum / wsum. KIND: TWK_DENOISER_*; GEO: the geometry guide
template<int KIND, bool GEO>
TWK_HD void denoiseTap(const DenoiseConstants& k, int dx, int dy, const float4& cp, const float4& np, const float4& ap,
                       const float4& cq, const float4& nq, const float4& aq, float& sx, float& sy, float& sz, float& wsum,
                       const DenoiseGeometryCentre& gc, const float4& gq)
{
  if (!finite3(cq)) return;
  float t = distance2(cp, cq) * k.invColor;
  if (KIND >= 2) t = t + distance2(np, nq) * k.invNormal;
  if (KIND >= 1) t = t + distance2(ap, aq) * k.invAlbedo;
  if (GEO) { if (!denoiseGeometryTap(gc, gq, t)) return; }
  if (!(t <= 87.0f)) return; // weight 0
  const float w = (stencilWeight(dy) * stencilWeight(dx)) * expP(-t);
  sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
  wsum = wsum + w;
}

// ---- the variance-guided mode ----
#define TWK_DENOISE_MOMENTS_RADIUS 3
#define TWK_DENOISE_LUMINANCE_EPSILON 1e-3f

TWK_HD float luminance(const float4& c) { return luminance3(c.x, c.y, c.z); } // (0.2126f c.x + 0.7152f c.y) + 0.0722f c.z

// One tap of the moments pass: folds the luminance lq of a tap with a finite colour into s0, s1, s2
template<int KIND, bool GEO>
TWK_HD void momentsTap(const DenoiseConstants& k, const float4& np, const float4& ap, float lq, const float4& nq, const float4& aq, float& s0, float& s1, float& s2,
                       const DenoiseGeometryCentre& gc, const float4& gq)
{
  float g = 1.0f;
  if (KIND >= 1)
  {
    float t = distance2(ap, aq) * k.invAlbedo;
    if (KIND >= 2) t = distance2(np, nq) * k.invNormal + t;
    if (GEO) { if (!denoiseGeometryTap(gc, gq, t)) return; }
    if (!(t <= 87.0f)) return;
    g = expP(-t);
  }
  s0 = s0 + g; s1 = s1 + g * lq; s2 = s2 + g * (lq * lq);
}

// The end of the moments pass: variance and firefly clamp of the centre cp from the sums; returns (cp.xyz clamped, var).
// SAMPLED: m = the pixel's luminance moments (mean, M2, n, .); the measured variance of the mean replaces var where n >= minSamples
template<bool SAMPLED>
TWK_HD float4 momentsFinish(const DenoiseConstants& k, float4 cp, float s0, float s1, float s2, const float4 m, float minSamples)
{
  float var = 0.0f, f = 1.0f;
  const float4 c0 = cp;
  if (s0 > 0.0f)
  {
    const float m1 = s1 / s0, m2 = s2 / s0;
    var = fmaxf(m2 - m1 * m1, 0.0f);
    if (k.fireflyThreshold > 0.0f)
    {
      const float limit = m1 + k.fireflyThreshold * sqrtf(var);
      const float lp = luminance(cp);
      if (lp > limit && limit > 0.0f)
      {
        f = limit / lp;
        cp.x = cp.x * f; cp.y = cp.y * f; cp.z = cp.z * f;
      }
    }
  }
  if (SAMPLED)
  {
    if (m.z >= minSamples && finite1(m.x) && finite1(m.y) && finite1(m.z) && m.x > 0.0f)
    {
      float v = m.y / ((m.z - 1.0f) * m.z);
      if (k.demodulate) { const float rho = luminance(c0) / m.x; v = v * (rho * rho); }
      var = v * (f * f);
    }
  }
  return make_float4(cp.x, cp.y, cp.z, var);
}

// One tap of the 3 x 3 binomial of the variance (dx, dy = -1 .. 1)
TWK_HD void varianceBlurTap(int dx, int dy, const float4& cq, float& vs, float& bs)
{
  if (!finite3(cq) || !finite1(cq.w)) return;
  const float b = ((dy == 0) ? 0.5f : 0.25f) * ((dx == 0) ? 0.5f : 0.25f);
  vs = vs + b * cq.w; bs = bs + b;
}

TWK_HD float inverseLuminanceSigma(const DenoiseConstants& k, float vs, float bs)
{
  const float vbar = (bs > 0.0f) ? vs / bs : 0.0f;
  return 1.0f / (k.sigmaLuminance * sqrtf(vbar) + TWK_DENOISE_LUMINANCE_EPSILON);
}

// One tap of a level of the variance-guided mode: like denoiseTap with the luminance edge-stop, and the variance filtered along
template<int KIND, bool GEO>
TWK_HD void denoiseVarianceTap(const DenoiseConstants& k, int dx, int dy, float lp, float invL, const float4& np, const float4& ap,
                               const float4& cq, const float4& nq, const float4& aq, float& sx, float& sy, float& sz, float& wsum, float& vsum,
                               const DenoiseGeometryCentre& gc, const float4& gq)
{
  if (!finite3(cq)) return;
  float t = fabsf(lp - luminance(cq)) * invL;
  if (KIND >= 2) t = t + distance2(np, nq) * k.invNormal;
  if (KIND >= 1) t = t + distance2(ap, aq) * k.invAlbedo;
  if (GEO) { if (!denoiseGeometryTap(gc, gq, t)) return; }
  if (!(t <= 87.0f)) return; // weight 0
  const float w = (stencilWeight(dy) * stencilWeight(dx)) * expP(-t);
  sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
  wsum = wsum + w;
  vsum = vsum + (w * w) * cq.w;
}

// ---- where the taps of a pixel come from ----
// A source names the centre and the taps of one pixel by an Index into its four arrays (colour, normal, albedo, geometry; an array
// the build does not use is never read): row(dy, r) names a row of taps and tap(r, dx, q) one tap of it; either is false
// where there is none, so a whole row is tested once, before its taps. luminance(q), for the moments pass: NaN where the colour is not finite.

// The picture where it lies, on the device or on the host: a tap outside the picture is absent
struct DenoiseGlobalTaps
{
  typedef int    Row;
  typedef size_t Index;
  const float4 *colour, *normal, *albedo, *geometry;
  int    width, height, x, y, step;
  size_t centre;

  TWK_HD DenoiseGlobalTaps(const float4* colour_, const float4* normal_, const float4* albedo_, const float4* geometry_, int width_, int height_, int x_, int y_, int step_)
    : colour(colour_), normal(normal_), albedo(albedo_), geometry(geometry_), width(width_), height(height_), x(x_), y(y_), step(step_), centre((size_t) y_ * width_ + x_) {}
  TWK_HD bool row(int dy, int& qy) const
  {
    qy = y + dy * step;
    return qy >= 0 && qy < height;
  }
  TWK_HD bool tap(int qy, int dx, size_t& q) const
  {
    const int qx = x + dx * step;
    if (qx < 0 || qx >= width) return false;
    q = (size_t) qy * width + qx;
    return true;
  }
  TWK_HD float luminance(size_t q) const { const float4 c = colour[q]; return finite3(c) ? twk::luminance(c) : asFloat(0x7fc00000u); }
};

// A block's taps staged densely, STRIDE entries per row (denoise_kernels.hip): every tap is present; what lies outside the picture
// was staged with a NaN colour. The arrays are given AT the centre's entry, so that a tap is a constant offset from it
// (one base register and the offset field of ds_read; by index the staged VAR builds took 15 VGPRs more: profiles/r21_denoise_one_body.md 3).
// Colour: float4, or float in the moments pass, which stages the luminance alone.
template<int STRIDE, typename Colour>
struct DenoiseStagedTaps
{
  typedef int Row;
  typedef int Index;
  static constexpr int centre = 0;
  const Colour* colour;
  const float4 *normal, *albedo, *geometry;

  TWK_HD bool  row(int dy, int& r) const { r = dy * STRIDE; return true; }
  TWK_HD bool  tap(int r, int dx, int& q) const { q = r + dx; return true; }
  TWK_HD float luminance(int q) const { return colour[q]; }
};

// ---- the four passes, one pixel each: the definition at the top of this file, statement for statement ----
template<typename Pixel>
TWK_HD void denoisePreparePixel(const DenoiseConstants& k, size_t p, const Pixel* beauty, const Pixel* albedo, const Pixel* normal, float4* colour, float4* guideNormal, float4* guideAlbedo)
{
  const float4 b = widen(beauty[p]);
  float4 c = b;
  if (albedo)
  {
    const float4 a = widen(albedo[p]);
    guideAlbedo[p] = make_float4(a.x, a.y, a.z, 0.0f);
    if (k.demodulate)
    {
      const float3 d = clampedAlbedo(a);
      c.x = b.x / d.x; c.y = b.y / d.y; c.z = b.z / d.z;
    }
  }
  if (normal)
  {
    const float4 n = widen(normal[p]);
    guideNormal[p] = make_float4(n.x, n.y, n.z, 0.0f);
  }
  colour[p] = c;
}

// SAMPLED: *m, the pixel's luminance moments, read once the sums are made. cp: the centre's colour (the staged source keeps luminances only)
template<int KIND, bool SAMPLED, bool GEO, typename Taps>
TWK_HD float4 denoiseMomentsPixel(const DenoiseConstants& k, const DenoiseGeometryConstants& g, const Taps& s, const float4 cp, const float4* m, float minSamples)
{
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 np = (KIND >= 2) ? s.normal[s.centre] : zero;
  const float4 ap = (KIND >= 1) ? s.albedo[s.centre] : zero;
  if (!finite3(cp) || !finite1(s.luminance(s.centre)) || !finite3(np) || !finite3(ap)) return make_float4(cp.x, cp.y, cp.z, 0.0f);
  DenoiseGeometryCentre gc = DenoiseGeometryCentre();
  if (GEO) { if (!denoiseGeometryCentre(g, s.geometry[s.centre], np, gc)) return make_float4(cp.x, cp.y, cp.z, 0.0f); }
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int dy = -TWK_DENOISE_MOMENTS_RADIUS; dy <= TWK_DENOISE_MOMENTS_RADIUS; ++dy)
  {
    typename Taps::Row   r;
    typename Taps::Index q;
    if (!s.row(dy, r)) continue;
#pragma unroll
    for (int dx = -TWK_DENOISE_MOMENTS_RADIUS; dx <= TWK_DENOISE_MOMENTS_RADIUS; ++dx)
    {
      if ((dx == 0 && dy == 0) || !s.tap(r, dx, q)) continue;
      const float lq = s.luminance(q);
      if ((asUint(lq) & 0x7fffffffu) > 0x7f800000u) continue; // NaN: a colour that is not finite
      const float4 nq = (KIND >= 2) ? s.normal[q] : zero;
      const float4 aq = (KIND >= 1) ? s.albedo[q] : zero;
      momentsTap<KIND, GEO>(k, np, ap, lq, nq, aq, s0, s1, s2, gc, GEO ? s.geometry[q] : zero);
    }
  }
  return momentsFinish<SAMPLED>(k, cp, s0, s1, s2, SAMPLED ? *m : zero, minSamples);
}

// VAR: the level of the variance-guided mode
template<int KIND, bool VAR, bool GEO, typename Taps>
TWK_HD float4 denoiseLevelPixel(const DenoiseConstants& k, const DenoiseGeometryConstants& g, const Taps& s)
{
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 cp = s.colour[s.centre];
  const float4 np = (KIND >= 2) ? s.normal[s.centre] : zero;
  const float4 ap = (KIND >= 1) ? s.albedo[s.centre] : zero;
  if (!finite3(cp) || !finite3(np) || !finite3(ap)) return cp;
  DenoiseGeometryCentre gc = DenoiseGeometryCentre();
  if (GEO) { if (!denoiseGeometryCentre(g, s.geometry[s.centre], np, gc)) return cp; }
  float lp = 0.0f, invL = 0.0f, vsum = 0.0f;
  if (VAR)
  {
    lp = luminance(cp);
    if (!finite1(lp)) return cp;
    float vs = 0.0f, bs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
    {
      typename Taps::Row   r;
      typename Taps::Index q;
      if (!s.row(dy, r)) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
      {
        if (s.tap(r, dx, q)) varianceBlurTap(dx, dy, s.colour[q], vs, bs);
      }
    }
    invL = inverseLuminanceSigma(k, vs, bs);
  }
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
  {
    typename Taps::Row   r;
    typename Taps::Index q;
    if (!s.row(dy, r)) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx)
    {
      if (!s.tap(r, dx, q)) continue;
      const float4 cq = s.colour[q];
      const float4 nq = (KIND >= 2) ? s.normal[q] : zero;
      const float4 aq = (KIND >= 1) ? s.albedo[q] : zero;
      const float4 gq = GEO ? s.geometry[q] : zero;
      if (VAR) denoiseVarianceTap<KIND, GEO>(k, dx, dy, lp, invL, np, ap, cq, nq, aq, sx, sy, sz, wsum, vsum, gc, gq);
      else     denoiseTap<KIND, GEO>(k, dx, dy, cp, np, ap, cq, nq, aq, sx, sy, sz, wsum, gc, gq);
    }
  }
  return make_float4(sx / wsum, sy / wsum, sz / wsum, VAR ? vsum / (wsum * wsum) : cp.w);
}

template<typename Pixel>
TWK_HD void denoiseFinishPixel(const DenoiseConstants& k, size_t p, const Pixel* beauty, const float4* colour, const float4* guideNormal, const float4* guideAlbedo, Pixel* denoised)
{
  const Pixel raw = beauty[p];
  const float4 b = widen(raw);
  float4 r = colour[p];
  bool through = !finite3(b);
  if (guideNormal) through = through || !finite3(guideNormal[p]);
  if (guideAlbedo)
  {
    const float4 a = guideAlbedo[p];
    through = through || !finite3(a);
    if (k.demodulate)
    {
      const float3 d = clampedAlbedo(a);
      r.x = r.x * d.x; r.y = r.y * d.y; r.z = r.z * d.z;
    }
  }
  if (through || !finite3(r)) { denoised[p] = raw; return; } // !finite3(r): the demodulated colour overflowed
  float4 o;
  o.x = r.x + k.blendFactor * (b.x - r.x);
  o.y = r.y + k.blendFactor * (b.y - r.y);
  o.z = r.z + k.blendFactor * (b.z - r.z);
  o.w = b.w;
  denoised[p] = pixelOf<Pixel>(o);
}

} // namespace twk
