// The firefly cascade (twk_enable_cascade, twk_cascade_resolve): every kept sample is split by its luminance over a few brightness
// layers as it is folded, and at resolve time a layer counts only as far as enough samples landed in it, in the pixel and its eight
// neighbours — the cascaded framebuffer of Zirr, Hanika and Dachsbacher, "Re-weighting firefly samples for improved finite-sample
// Monte Carlo estimates" (CGF 2018), reduced to its count criterion. The definition below is complete and is compiled once for the
// kernels (the CASCADE builds of the accumulate kernels in shade_kernels.hip; cascade_kernels.hip) and once for the host
// (twk_cascade_fold_host, twk_cascade_resolve_host, device_cascade.hip); tests/cascade_restate.py restates it statement for
// statement in numpy float32. All arithmetic is f32, every operation rounded once (-ffp-contract=off, csrc/Makefile).
//
// PARAMETERS  TwkCascade { layers K in 2..8, start > 0 finite, base > 1 finite }. Thresholds b[0] = start, b[j + 1] = b[j] * base,
// j + 1 < K, by repeated f32 multiplication ON THE HOST (cascadeConstants below); a table that reaches inf is refused. The device
// sees the table only: no pow, no log.
//
// STORAGE  K layers of float4, layer-major: layer j of launch index i is layers[j * stride + i], stride = launchWidth x height, i as
// the moments are indexed (the launch index, under twk_set_shared_frame as well). Always f32. .xyz: the layer's weighted radiance
// sum. layer 0 .w: n, the number of kept samples. layer K-1 .w: the number of kept samples that were rejected as not finite.
// Every other .w: 0.
//
// FOLD  per KEPT sample (the keep rule, the r.w == 0 skip and the iteration order are the running mean's and the moments':
// shade_device.h foldSample), on the radiance r = (rx, ry, rz) as it is folded (the false colour under debugExceptions):
//   iteration 0:  every sum, n and the rejected count = 0                   (the layers start afresh where the running mean does)
//   n = n + 1
//   rx, ry or rz not finite:  rejected = rejected + 1, nothing else
//   l = luminance3(rx, ry, rz)                                              (device_math.h)
//   j = 0; for i = 1 .. K-2 ascending: if (b[i] <= l) j = i                 (the largest such index; 0 when l < b[0])
//   lo = b[j]; hi = b[j + 1]
//   l <= lo:       wLo = 1, wHi = 0
//   else l < hi:   q = lo / hi;  wLo = (lo / l - q) / (1 - q);  wHi = 1 - wLo
//   else:          wLo = 0, wHi = hi / l                                    (energy above the top layer: the only clamp)
//   wLo != 0:  layer j   .xyz = .xyz + wLo * r     (component by component, product rounded, then the sum)
//   wHi != 0:  layer j+1 .xyz = .xyz + wHi * r
// A layer whose weight is 0 is not touched (adding a zero would turn a -0 sum into +0). For lo <= l < hi,
// wLo l / lo + wHi l / hi = 1: luminance(layer j) / b[j] counts samples.
//
// RESOLVE  TwkCascadeResolve { kappa > 0 finite }, per pixel p = (x, y) of a width x height grid whose element i = y * width + x:
//   lambda[j][i] = luminance3(layer j of i .xyz)                            (first launch: an f32 stream of K x width x height)
//   n = layer 0 of p .w;  n == 0 or not finite:  out = (0, 0, 0, 0)
//   for j = 1 .. K-1:
//     a_j(q) = (lambda[j-1][q] + lambda[j][q]) + lambda[j+1][q]             (the last term is left out for j = K-1)
//     S_j = 0;  for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = (x + dx, y + dy) inside the grid:  S_j = S_j + a_j(q)
//     c_j = S_j / b[j];   t = c_j / kappa;   w_j = (t < 1) ? t : 1
//   acc = layer 0 .xyz;  for j = 1 .. K-1 ascending:  acc = acc + w_j * layer j .xyz     (component by component)
//   sum = layer 0 .xyz;  for j = 1 .. K-1 ascending:  sum = sum + layer j .xyz
//   some c_j not finite:  out = (sum / n, 1)      (the plain quotient. A lambda of the window that is not finite makes its a_j, S_j
//                                                   and c_j not finite, as does a sum that overflows: this one test covers both)
//   else:                 out = (acc / n, 1)
// out is narrowed once to the output format. As the samples grow every c_j passes kappa, every w_j is 1, and out is the plain quotient.
//
// What this leaves out of the paper: its mixing of a local (per pixel) and a global (per layer) reliability — this is the 3x3 count
// alone; its variance term; and colour — the reliability is of the luminance only, one weight for the three components.
// What it is not: unbiased at finite n. The top-layer clamp and every w_j < 1 remove energy.
// Nor temporal by itself: the layers of a moved camera start afresh at iteration 0, and temporal_cascade_device.h carries them over
// (twk_temporal_enable_cascade, opt-in) — the layers are sums, so reprojected history sums plus a frame's are again a cascade.
#pragma once
#include "device_types.h"

namespace twk {

TWK_HD bool cascadeFinite(float v) { return (asUint(v) & 0x7f800000u) != 0x7f800000u; } // neither inf nor NaN (denoise_device.h finite1)

#define TWK_CASCADE_MAX_LAYERS 8
// The loops over layers and taps have constant trip counts and are unrolled, so that the small arrays they index live in registers
#ifdef __clang__
#define TWK_CASCADE_UNROLL _Pragma("unroll")
#else
#define TWK_CASCADE_UNROLL
#endif

// TwkCascade as the kernels take it: the number of layers and the threshold table
struct CascadeConstants
{
  int   layers;
  float b[TWK_CASCADE_MAX_LAYERS];
};

// The parameter rule of every entry point that takes a TwkCascade; nullptr: accepted, k is filled. Else the reason it is refused.
inline const char* cascadeConstants(const TwkCascade& c, CascadeConstants& k)
{
  if (c.layers < 2 || c.layers > TWK_CASCADE_MAX_LAYERS) return "layers must be in 2..8";
  if (!(c.start > 0.0f) || !cascadeFinite(c.start)) return "start must be > 0 and finite";
  if (!(c.base > 1.0f) || !cascadeFinite(c.base)) return "base must be > 1 and finite";
  k.layers = c.layers;
  float b = c.start;
  for (int j = 0; j < TWK_CASCADE_MAX_LAYERS; ++j)
  {
    k.b[j] = (j < c.layers) ? b : 0.0f;
    if (j < c.layers && !cascadeFinite(b)) return "the thresholds start * base^j reach inf";
    if (j + 1 < c.layers) b = b * c.base;
  }
  return nullptr;
}

// One launch index's layers while a pass folds into them: named registers, never an indexed array (the layer a sample falls into is
// known only at run time; an array indexed by it would live in scratch memory).
struct CascadeSums
{
  float x0, y0, z0, x1, y1, z1, x2, y2, z2, x3, y3, z3, x4, y4, z4, x5, y5, z5, x6, y6, z6, x7, y7, z7;
  float n, rejected;
};

// F(i) for every layer index, in ascending order
#define TWK_CASCADE_EACH(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)

TWK_HD void cascadeZero(CascadeSums& s)
{
#define TWK_CASCADE_ZERO(i) s.x##i = 0.0f; s.y##i = 0.0f; s.z##i = 0.0f;
  TWK_CASCADE_EACH(TWK_CASCADE_ZERO)
#undef TWK_CASCADE_ZERO
  s.n = 0.0f; s.rejected = 0.0f;
}

// The layers of element `index` as stored -> sums. Layers K and above are not read.
TWK_HD void cascadeLoad(const CascadeConstants& k, const float4* layers, const size_t stride, const size_t index, CascadeSums& s)
{
  cascadeZero(s);
#define TWK_CASCADE_LOAD(i) \
  if (i < k.layers) { const float4 v = layers[(size_t) i * stride + index]; s.x##i = v.x; s.y##i = v.y; s.z##i = v.z; if (i == 0) s.n = v.w; if (i == k.layers - 1) s.rejected = v.w; }
  TWK_CASCADE_EACH(TWK_CASCADE_LOAD)
#undef TWK_CASCADE_LOAD
}

TWK_HD void cascadeStore(const CascadeConstants& k, float4* layers, const size_t stride, const size_t index, const CascadeSums& s)
{
#define TWK_CASCADE_STORE(i) \
  if (i < k.layers) layers[(size_t) i * stride + index] = make_float4(s.x##i, s.y##i, s.z##i, (i == 0) ? s.n : ((i == k.layers - 1) ? s.rejected : 0.0f));
  TWK_CASCADE_EACH(TWK_CASCADE_STORE)
#undef TWK_CASCADE_STORE
}

// FOLD above, for one kept sample
TWK_HD void cascadeFoldSample(const CascadeConstants& k, CascadeSums& s, const unsigned int iteration, const float rx, const float ry, const float rz)
{
  if (iteration == 0) cascadeZero(s);
  s.n = s.n + 1.0f;
  if (!cascadeFinite(rx) || !cascadeFinite(ry) || !cascadeFinite(rz)) { s.rejected = s.rejected + 1.0f; return; }
  const float l = luminance3(rx, ry, rz);
  int j = 0; float lo = k.b[0], hi = k.b[1];
#define TWK_CASCADE_FIND(i) if (i >= 1 && i <= k.layers - 2 && k.b[i] <= l) { j = i; lo = k.b[i]; hi = k.b[(i + 1) & (TWK_CASCADE_MAX_LAYERS - 1)]; }
  TWK_CASCADE_EACH(TWK_CASCADE_FIND)
#undef TWK_CASCADE_FIND
  float wLo, wHi;
  if (l <= lo) { wLo = 1.0f; wHi = 0.0f; }
  else if (l < hi) { const float q = lo / hi; wLo = (lo / l - q) / (1.0f - q); wHi = 1.0f - wLo; }
  else { wLo = 0.0f; wHi = hi / l; }
#define TWK_CASCADE_ADD(i) \
  { const float w = (i == j) ? wLo : ((i == j + 1) ? wHi : 0.0f); if (w != 0.0f) { s.x##i = s.x##i + w * rx; s.y##i = s.y##i + w * ry; s.z##i = s.z##i + w * rz; } }
  TWK_CASCADE_EACH(TWK_CASCADE_ADD)
#undef TWK_CASCADE_ADD
}

TWK_HD float cascadeLambda(const float4& v) { return luminance3(v.x, v.y, v.z); }

// RESOLVE above, for pixel (x, y): layers and lambda are [K][stride] with stride >= width * height, element y * width + x
TWK_HD float4 cascadeResolvePixel(const CascadeConstants& k, const float kappa, const float4* layers, const float* lambda, const size_t stride,
                                  const int width, const int height, const int x, const int y)
{
  const size_t p = (size_t) y * width + x;
  const float4 first = layers[p];
  const float n = first.w;
  if (n == 0.0f || !cascadeFinite(n)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float S[TWK_CASCADE_MAX_LAYERS]; // indexed by unrolled loops only
TWK_CASCADE_UNROLL
  for (int j = 0; j < TWK_CASCADE_MAX_LAYERS; ++j) S[j] = 0.0f;
TWK_CASCADE_UNROLL
  for (int dy = -1; dy <= 1; ++dy)
  {
    const int qy = y + dy;
    if (qy < 0 || qy >= height) continue;
TWK_CASCADE_UNROLL
    for (int dx = -1; dx <= 1; ++dx)
    {
      const int qx = x + dx;
      if (qx < 0 || qx >= width) continue;
      const size_t q = (size_t) qy * width + qx;
      float lam[TWK_CASCADE_MAX_LAYERS];
TWK_CASCADE_UNROLL
      for (int j = 0; j < TWK_CASCADE_MAX_LAYERS; ++j) lam[j] = (j < k.layers) ? lambda[(size_t) j * stride + q] : 0.0f;
TWK_CASCADE_UNROLL
      for (int j = 1; j < TWK_CASCADE_MAX_LAYERS; ++j)
      {
        if (j >= k.layers) continue;
        float a = lam[j - 1] + lam[j];
        if (j < k.layers - 1) a = a + lam[(j + 1) & (TWK_CASCADE_MAX_LAYERS - 1)];
        S[j] = S[j] + a;
      }
    }
  }
  bool plain = false;
  float ax = first.x, ay = first.y, az = first.z; // acc
  float sx = first.x, sy = first.y, sz = first.z; // sum
TWK_CASCADE_UNROLL
  for (int j = 1; j < TWK_CASCADE_MAX_LAYERS; ++j)
  {
    if (j >= k.layers) continue;
    const float c = S[j] / k.b[j];
    if (!cascadeFinite(c)) plain = true;
    const float t = c / kappa;
    const float w = (t < 1.0f) ? t : 1.0f;
    const float4 v = layers[(size_t) j * stride + p];
    ax = ax + w * v.x; ay = ay + w * v.y; az = az + w * v.z;
    sx = sx + v.x; sy = sy + v.y; sz = sz + v.z;
  }
  if (plain) return make_float4(sx / n, sy / n, sz / n, 1.0f);
  return make_float4(ax / n, ay / n, az / n, 1.0f);
}

// What the CASCADE builds of the accumulate kernels take beside the launch parameters (shade_kernels.hip); stride = LaunchParams::numPixels
struct CascadeOn  { static constexpr bool on = true;  float4* layers; CascadeConstants k; };
struct CascadeOff { static constexpr bool on = false; };

} // namespace twk
