// The temporal half of the denoiser: the geometry AOV a frame is reprojected with, and the merge of the last frame's samples
// into this frame's through the previous camera — the temporal accumulation of Schied et al., "Spatiotemporal Variance-Guided
// Filtering" (HPG 2017, section 4.1), in front of the a-trous filter of denoise_device.h, which is unchanged: it is handed the
// merged colour as `beauty` and the merged moments (twk_denoise_variance_sampled). Nothing is learned. The definition below is
// complete; tests/test_gpu_temporal.py restates it statement for statement in numpy float32 and compares bits. Built with
// -ffp-contract=off (csrc/Makefile): every operation below rounds once, as written. Sums of three products are evaluated left to
// right, dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, and distance2 is denoise_device.h's.
//
// ---- the geometry AOV (twk_render_geometry) -------------------------------------------------------------------------------------
// One closest-hit ray per pixel (x, y) through the pixel's CENTRE: shade_device.h primaryRay's pinhole branch with sampleX =
// sampleY = 0.5f, the same operations in the same order (centreRay below), traced by trace_device.h traverse<false> from tmin =
// sceneEpsilon to tmax = RT_DEFAULT_MAX. One float4 per pixel, always f32:
//   hit:   (P.x + t d.x, P.y + t d.y, P.z + t d.z, bits of (unsigned) instance + 1)      P the camera position, d the direction
//   miss:  (0, 0, 0, bits 0)
//
// ---- the geometry AOV of a tile share (twk_render_geometry_tile) ---------------------------------------------------------------
// On a handle whose buffers are packed tile buffers (distribution 1, device `index` of `count` > 1), one element per launch index
// i = ly * launchWidth + lx, 0 <= lx < launchWidth, 0 <= ly < height:
//   x = distribute(lx, ly) of shade_device.h = twk_tile_column(lx, ly, tileSize, count, index) = assemble_device.h's map
//   x >= width:  padding, geometry[i] = (0, 0, 0, bits 0), no ray
//   else:        the ray centreRay(cam, x, ly, width, height), traced and written exactly as above, to geometry[i]
// so that assembling the shares (assemble_device.h; 16-byte elements, one layer) gives the picture-shaped AOV above, bit for bit.
// On any other handle the call is twk_render_geometry. The kernel is a second build of geometryKernel (temporal_kernels.hip).
//
// ---- the temporal merge (twk_temporal_accumulate) -------------------------------------------------------------------------------
// Streams, one element per pixel: the current frame's colour (the handle's output format, widened exactly), its luminance moments
// (mean, M2, n, .) as shade_device.h foldSamples accumulates them and its geometry AOV; the history's colour (f32, a previous
// call's historyOut), moments and geometry, and the camera (P', U', V', W') the history was rendered from.
//
// host, once per call, in f32 (temporalCamera below), cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x):
//   A = cross(V', W');  B = cross(W', U');  C = cross(U', V');  D = dot(U', A);  tol2 = tol * tol
//   (D zero or not finite: the previous camera is degenerate, the call is refused)
//   A pinhole ray of that camera is s (U' ndcX + V' ndcY + W'), s > 0, so for v = point - P':  dot(v, A) = s ndcX D,
//   dot(v, B) = s ndcY D, dot(v, C) = s D: the screen position is a quotient in which D cancels (no matrix inverse), and the
//   point lies in front of the camera where dot(v, C) D > 0.
//
// pixel p = (x, y):
//   cur = widen(colour[p]);  mc = moments[p];  g = geometry[p]
//   PASS THROUGH — colourOut[p] = colour[p] (its bits), historyOut[p] = cur, momentsOut[p] = mc — when there is no history
//   buffer, or the bits of g.w are 0 (a miss), or a component of g.xyz, cur.xyz or mc.xyz is not finite, or mc.z < 1;
//   and wherever "no history" is said below.
//   v = g.xyz - P';  a = dot(v, A);  b = dot(v, B);  c = dot(v, C);   no history unless c * D > 0
//   fx = ((a / c + 1) * 0.5f) * width - 0.5f;  fy = ((b / c + 1) * 0.5f) * height - 0.5f
//   no history unless -1 <= fx < width and -1 <= fy < height   (else all four taps lie outside the picture; NaN compares false)
//   x0 = floorf(fx);  tx = fx - x0;  y0 = floorf(fy);  ty = fy - y0
//   ws = 0; sc = (0, 0, 0); smean = sM2 = sn = 0
//   for dy = 0, 1, for dx = 0, 1 (in this order): q = (x0 + dx, y0 + dy), skipped when outside the picture
//     hg = historyGeometry[q]; skipped unless the bits of hg.w equal the bits of g.w
//     skipped unless distance2(hg, g) <= tol2 * dot(v, v)                                  (NaN: skipped)
//     hc = historyColour[q];  hm = historyMoments[q]; skipped unless hc.xyz and hm.xyz are finite and hm.z >= 1
//     w = (dx ? tx : 1 - tx) * (dy ? ty : 1 - ty)
//     sc.k = sc.k + w * hc.k;  smean = smean + w * hm.x;  sM2 = sM2 + w * hm.y;  sn = sn + w * hm.z;  ws = ws + w
//   no history unless ws > 0
//   hc.k = sc.k / ws;  hmean = smean / ws;  hM2 = sM2 / ws;  hn = sn / ws
//   cap:  if hn > maxHistory:  hM2 = hM2 * (maxHistory / hn);  hn = maxHistory                (maxHistory as a float)
//   merge (Chan's pairwise form of Welford, the history as one set of hn samples and the frame as one of mc.z):
//     n = hn + mc.z;  r = mc.z / n
//     colour.k = hc.k + (cur.k - hc.k) * r                                                  k = x, y, z
//     d = mc.x - hmean;  mean = hmean + d * r;  M2 = (hM2 + mc.y) + (d * d) * (hn * r)
//   colourOut[p] = narrow(colour.xyz, cur.w) (RGBA16F: round to nearest even, once);  historyOut[p] = (colour.xyz, cur.w) in f32;
//   momentsOut[p] = (mean, M2, n, 0)
// Each statement is written once below: temporalGather (from the candidate test to the last tap; its footprint x0, y0, tx, ty and the
// weight w are temporalFootprint and temporalTapWeight, which the cascade's merge shares), temporalHistory (the quotients and the
// cap), temporalBlend (the merge), and the store of the three outputs in temporal_store.h. The rectified merge
// (temporal_rectify_device.h) calls the same functions; it is not a second copy.
//
// What this approximates, and what it is not. The history is measured in SAMPLES: the cap scales M2 with n, which leaves the
// sample variance M2 / n of the history where it was and bounds its weight, so an old frame fades the way an exponential
// average with alpha = spp / (maxHistory + spp) does. The bilinear interpolation of M2 ignores the spread of the four taps'
// means (the exact pairwise merge of the taps would add it): across a luminance edge inside one surface the interpolated variance
// is too small by that spread. hn is a weighted mean of sample counts, not a count. A pixel that MISSED never has history: the
// environment would have to be reprojected by direction, which is left out. The lens is the pinhole: no fisheye or sphere. Objects
// move by one matrix per instance, in the Moving builds only (temporal_motion_device.h: twk_update_instance_transform keeps the
// history and the merges look it up where the instance was); the builds without it take the scene as static between the history's
// frame and this one. A deformed mesh (twk_update_geometry_vertices) is followed by the Carried builds, which take g' per pixel from
// the previous-position plane (temporal_carry_device.h). No motion blur. The merge itself works on whole pictures.
// A frame tiled over several devices is merged on ONE of them: every device traces the geometry of its own share (above), the
// shares and the planes are assembled there in one launch (twk_assemble_devices_with_geometry) and
// twk_temporal_accumulate_assembled runs this same merge on the assembled W x H buffers, with that handle's history. Nothing is
// scattered back to the tiles, and the merge does not read the packed tiles itself.
#pragma once
#include "denoise_device.h"
#include "temporal_carry_device.h" // temporalMove (temporal_motion_device.h) and temporalCarry

namespace twk {

struct TemporalConstants
{
  int   width, height;
  int   hasHistory;
  float maxHistory;   // (float) TwkTemporal::maxHistory
  float tol2;         // positionTolerance * positionTolerance
  float P[3], A[3], B[3], C[3];
  float D;
};

// dot3, the left-to-right dot product: denoise_device.h (the geometry guide of the denoiser uses the same one)

// The previous camera's part of the constants; cam = P', U', V', W' (12 floats). False: degenerate (D zero or not finite).
TWK_HD bool temporalCamera(const float* cam, TemporalConstants& k)
{
  const float Ux = cam[3], Uy = cam[4], Uz = cam[5], Vx = cam[6], Vy = cam[7], Vz = cam[8], Wx = cam[9], Wy = cam[10], Wz = cam[11];
  k.P[0] = cam[0]; k.P[1] = cam[1]; k.P[2] = cam[2];
  k.A[0] = Vy * Wz - Vz * Wy; k.A[1] = Vz * Wx - Vx * Wz; k.A[2] = Vx * Wy - Vy * Wx; // cross(V', W')
  k.B[0] = Wy * Uz - Wz * Uy; k.B[1] = Wz * Ux - Wx * Uz; k.B[2] = Wx * Uy - Wy * Ux; // cross(W', U')
  k.C[0] = Uy * Vz - Uz * Vy; k.C[1] = Uz * Vx - Ux * Vz; k.C[2] = Ux * Vy - Uy * Vx; // cross(U', V')
  k.D = dot3(Ux, Uy, Uz, k.A[0], k.A[1], k.A[2]);
  return finite1(k.D) && k.D != 0.0f;
}

// The ray through the centre of pixel (x, y): primaryRay's pinhole branch (shade_device.h; lens_shader.cu:40-52) with the jitter 0.5
TWK_HD V3 centreRay(const float* cam, int x, int y, int width, int height)
{
  const float screenX = float(width), screenY = float(height);
  const float pixelX  = float(x),     pixelY  = float(y);
  const float sampleX = 0.5f, sampleY = 0.5f;
  const V3 U = v3(cam[3], cam[4], cam[5]), V = v3(cam[6], cam[7], cam[8]), W = v3(cam[9], cam[10], cam[11]);
  const float ndcX = ((pixelX + sampleX) / screenX) * 2.0f - 1.0f;
  const float ndcY = ((pixelY + sampleY) / screenY) * 2.0f - 1.0f;
  return normalize(U * ndcX + V * ndcY + W);
}

// Whether pixel p can take history at all (before the projection): a hit, everything finite, at least one sample
TWK_HD bool temporalCandidate(const TemporalConstants& k, const float4& cur, const float4& mc, const float4& g)
{
  return k.hasHistory != 0 && asUint(g.w) != 0u && finite3(g) && finite3(cur) && finite3(mc) && !(mc.z < 1.0f);
}

// World position g through the previous camera: false = no history. vv = dot(v, v), the squared distance to that camera.
TWK_HD bool temporalProject(const TemporalConstants& k, const float4& g, float& fx, float& fy, float& vv)
{
  const float vx = g.x - k.P[0], vy = g.y - k.P[1], vz = g.z - k.P[2];
  const float a = dot3(vx, vy, vz, k.A[0], k.A[1], k.A[2]);
  const float b = dot3(vx, vy, vz, k.B[0], k.B[1], k.B[2]);
  const float c = dot3(vx, vy, vz, k.C[0], k.C[1], k.C[2]);
  vv = dot3(vx, vy, vz, vx, vy, vz);
  if (!(c * k.D > 0.0f)) return false;
  fx = ((a / c + 1.0f) * 0.5f) * float(k.width) - 0.5f;
  fy = ((b / c + 1.0f) * 0.5f) * float(k.height) - 0.5f;
  return fx >= -1.0f && fx < float(k.width) && fy >= -1.0f && fy < float(k.height);
}

// Whether the history's geometry hg at a tap belongs to the surface point g
TWK_HD bool temporalTapGeometry(const TemporalConstants& k, const float4& g, const float4& hg, float vv)
{
  return asUint(hg.w) == asUint(g.w) && distance2(hg, g) <= k.tol2 * vv;
}

// The four history pixels around the reprojected position (fx, fy), which temporalProject has bounded: the corner (x0, y0) in
// [-1, width - 1] x [-1, height - 1] and the fractions; tap (dx, dy) is pixel (x0 + dx, y0 + dy)
struct TemporalFootprint { int x0, y0; float tx, ty; };

TWK_HD TemporalFootprint temporalFootprint(float fx, float fy)
{
  const float fx0 = floorf(fx), fy0 = floorf(fy);
  TemporalFootprint f;
  f.tx = fx - fx0; f.ty = fy - fy0;
  f.x0 = (int) fx0; f.y0 = (int) fy0;
  return f;
}

// The bilinear weight of tap (dx, dy)
TWK_HD float temporalTapWeight(const TemporalFootprint& f, int dx, int dy)
{
  return (dx ? f.tx : 1.0f - f.tx) * (dy ? f.ty : 1.0f - f.ty);
}

struct TemporalSums { float x, y, z, mean, M2, n, ws; };

// One counted tap: the history's colour hc and moments hm with bilinear weight w
TWK_HD void temporalTap(const float4& hc, const float4& hm, float w, TemporalSums& s)
{
  if (!finite3(hc) || !finite3(hm) || !(hm.z >= 1.0f)) return;
  s.x = s.x + w * hc.x; s.y = s.y + w * hc.y; s.z = s.z + w * hc.z;
  s.mean = s.mean + w * hm.x; s.M2 = s.M2 + w * hm.y; s.n = s.n + w * hm.z;
  s.ws = s.ws + w;
}

// The gather at pixel p, from the candidate test to the last tap: s.ws > 0 says there is history. The history's geometry is read
// first; its colour and moments only at the taps that belong to the surface. (cur, mc and g by value: by reference the kernel's
// load of g is split into xyz and w and temporalKernel grows by 30 instructions.) Moving: the build that first carries g to where
// its instance was in the history's frame (temporal_motion_device.h temporalMove, with the table motion[numMotion]); otherwise the
// table is not read.
// Carried: the build that takes g' from the previous-position plane instead (temporal_carry_device.h temporalCarry; carried: the
// plane's element of this pixel); otherwise it is not read.
template<bool Moving = false, bool Carried = false>
TWK_HD void temporalGather(const TemporalConstants& k, const float4 cur, const float4 mc, const float4 g, const float4* historyColour, const float4* historyMoments,
                           const float4* historyGeometry, TemporalSums& s, const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u,
                           const float4 carried = make_float4(0.0f, 0.0f, 0.0f, 0.0f))
{
  s.x = 0.0f; s.y = 0.0f; s.z = 0.0f; s.mean = 0.0f; s.M2 = 0.0f; s.n = 0.0f; s.ws = 0.0f;
  float fx = 0.0f, fy = 0.0f, vv = 0.0f;
  if (!temporalCandidate(k, cur, mc, g)) return;
  float4 gp = g;
  if (Moving && !temporalMove(motion, numMotion, g, gp)) return;
  if (Carried && !temporalCarry(carried, g, gp)) return;
  if (!temporalProject(k, gp, fx, fy, vv)) return;
  const TemporalFootprint f = temporalFootprint(fx, fy);
#pragma unroll
  for (int dy = 0; dy <= 1; ++dy)
  {
    const int qy = f.y0 + dy;
    if (qy < 0 || qy >= k.height) continue;
#pragma unroll
    for (int dx = 0; dx <= 1; ++dx)
    {
      const int qx = f.x0 + dx;
      if (qx < 0 || qx >= k.width) continue;
      const size_t q = (size_t) qy * k.width + qx;
      if (!temporalTapGeometry(k, gp, historyGeometry[q], vv)) continue;
      temporalTap(historyColour[q], historyMoments[q], temporalTapWeight(f, dx, dy), s);
    }
  }
}

// The interpolated history of a pixel: colour, luminance mean and M2, and its count n in samples
struct TemporalHistory { float x, y, z, mean, M2, n; };

// The quotients by s.ws (> 0) and the cap of the count at maxHistory
TWK_HD TemporalHistory temporalHistory(const TemporalConstants& k, const TemporalSums& s)
{
  TemporalHistory h;
  h.x = s.x / s.ws; h.y = s.y / s.ws; h.z = s.z / s.ws;
  h.mean = s.mean / s.ws;
  h.M2 = s.M2 / s.ws; h.n = s.n / s.ws;
  if (h.n > k.maxHistory) { h.M2 = h.M2 * (k.maxHistory / h.n); h.n = k.maxHistory; }
  return h;
}

// The merge by count of a history h with the frame's cur, mc: the merged colour (alpha = cur.w) and moments
TWK_HD void temporalBlend(const TemporalHistory& h, const float4& cur, const float4& mc, float4& colour, float4& moments)
{
  const float n = h.n + mc.z;
  const float r = mc.z / n;
  colour.x = h.x + (cur.x - h.x) * r; colour.y = h.y + (cur.y - h.y) * r; colour.z = h.z + (cur.z - h.z) * r;
  colour.w = cur.w;
  const float d = mc.x - h.mean;
  moments.x = h.mean + d * r;
  moments.y = (h.M2 + mc.y) + (d * d) * (h.n * r);
  moments.z = n;
  moments.w = 0.0f;
}

// The merge of the interpolated history (s.ws > 0) with the frame's cur, mc
TWK_HD void temporalMerge(const TemporalConstants& k, const TemporalSums& s, const float4& cur, const float4& mc, float4& colour, float4& moments)
{
  temporalBlend(temporalHistory(k, s), cur, mc, colour, moments);
}

} // namespace twk
