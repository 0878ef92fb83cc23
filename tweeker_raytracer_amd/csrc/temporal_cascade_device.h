// The firefly cascade's layers through the temporal merge (twk_temporal_accumulate_cascade, twk_temporal_enable_cascade): the
// history's per-layer sums are reprojected through the previous camera exactly as temporal_device.h reprojects the plain mean, and
// added to this frame's. The cascade stores SUMS, so the merge is linear: interpolated, capped history sums plus the frame's sums are
// again a cascade, luminance(layer j) / b[j] still counts samples, and twk_cascade_resolve (cascade_device.h) runs on the result
// unchanged — with the counts of the history behind its weights instead of one frame's 1 - 4 samples. The definition below is
// complete and is compiled once for the kernel (temporal_cascade_kernels.hip) and once for the host (twk_temporal_cascade_host);
// tests/temporal_cascade_restate.py restates it statement for statement in numpy float32. All arithmetic is f32, every operation
// rounded once, in the order written (-ffp-contract=off, csrc/Makefile). The projection, the footprint with its weights and the
// test of a tap's geometry are temporal_device.h's own functions (temporalProject, temporalFootprint, temporalTapWeight,
// temporalTapGeometry), not restated; the test of a tap's counts, the w > 0 rule and the per-layer sums are this header's.
//
// Streams, per pixel p of a width x height grid: the current layers Lc[j] and the history layers H[j], [K][width x height] float4,
// layer-major as cascade_device.h stores them; the current geometry AOV g and the history's hg; the history camera (temporalCamera).
// nc = Lc[0][p].w (the frame's kept samples), rc = Lc[K-1][p].w (its rejected ones).
//
// PASS THROUGH — out[j][p] = Lc[j][p], its bits, for every layer — when there is no history buffer, or the bits of g.w are 0 (a
// miss), or a component of g.xyz is not finite, or nc is not finite or nc < 1; and wherever "no history" is said below.
//   (fx, fy, vv) = temporalProject(g): no history when it says so (behind the previous camera, outside its view)
//   x0 = floorf(fx);  tx = fx - x0;  y0 = floorf(fy);  ty = fy - y0
//   ws = sn = srej = 0;  s[j] = (0, 0, 0) for every layer
//   for dy = 0, 1, for dx = 0, 1 (in this order): q = (x0 + dx, y0 + dy), skipped when outside the grid
//     skipped unless temporalTapGeometry(g, hg[q], vv)
//     hn_q = H[0][q].w;  skipped unless hn_q is finite and hn_q >= 1;  skipped unless H[K-1][q].w is finite
//     w = (dx ? tx : 1 - tx) * (dy ? ty : 1 - ty);  skipped unless w > 0     (a weight of exactly 0 carries nothing: 0 x inf is no NaN)
//     s[j].k = s[j].k + w * H[j][q].k   (k = x, y, z, every layer);  sn = sn + w * hn_q;  srej = srej + w * H[K-1][q].w;  ws = ws + w
//   no history unless ws > 0
//   h[j].k = s[j].k / ws;  hn = sn / ws;  hrej = srej / ws
//   cap:  if hn > maxHistory:  f = maxHistory / hn;  h[j].k = h[j].k * f;  hrej = hrej * f;  hn = maxHistory
//   out[j].xyz = h[j].xyz + Lc[j].xyz;  out[0].w = hn + nc;  out[K-1].w = hrej + rc;  every other .w = 0
// The sums of a layer are NOT tested for finiteness: a history sum that is not finite propagates into that layer of the output, and
// the resolve's plain-quotient rule deals with it as it does with a frame's own. The merged layers are the next call's history and
// the resolve's input as they are; nothing is narrowed.
//
// What this approximates, and what it is not. n (layer 0 .w) becomes a weighted, capped count that is no integer; the cap scales
// every sum with it, which leaves each layer's mean contribution where it was and bounds the history's weight at maxHistory samples.
// The bilinear interpolation mixes the sums AND the counts of neighbouring pixels: a layer count c_j of the resolve then speaks of a
// neighbourhood one pixel wider than its 3x3 window. Alpha and the luminance moments are not here: they are the existing merge's
// business (temporal_device.h), which this leaves untouched. As there: objects move by one matrix per instance in the Moving builds
// only (temporal_motion_device.h; a candidate here is a hit with finite g.xyz and nc >= 1), no environment reprojection (a miss never
// has history), the pinhole lens only, one device, no tiles; the paper's variance term is not reprojected, and neither the noise
// estimate nor the adaptive passes see the merged layers.
//
// The TRUSTED build (twk_temporal_accumulate_cascade_trusted; temporal_rectify_device.h defines the trust): beside the streams above
// one float t per pixel, the trustOut of twk_temporal_accumulate_rectified. After the cap, and only there,
//   h[j].k = h[j].k * t;  hrej = hrej * t;  hn = hn * t
// and the last line runs on the results: out[0].w = hn * t + nc. The history is discounted in every layer by the factor its plain
// mean was discounted by; the merge stays linear, so twk_cascade_resolve runs unchanged on the result. A pass-through pixel does
// not read t. t = 1 gives the bits of the build without a trust (x * 1 is x); t = 0 leaves the frame's sums plus 0 — a history
// sum that is not finite gives NaN there, as it would have given inf.
#pragma once
#include "temporal_device.h"
#include "cascade_device.h"

namespace twk {

// Pixel p of Lc / geometry -> out; H, hGeometry: the history (H == nullptr: none; k.hasHistory says the same). Every buffer's layer
// stride is `stride` >= k.width * k.height. The loops over taps and layers have constant trip counts and are unrolled, the layer loop
// predicated by j < K, so that the small arrays live in registers (cascade_device.h).
// Trusted: the build that discounts the capped history by trust[p] (above); otherwise trust is not read.
// Moving: the build that carries g to where its instance was in the history's frame before the projection and the taps' test
// (temporal_motion_device.h temporalMove, with the table motion[numMotion]; g' not finite: no history); otherwise the table is not read.
// Carried: the build that takes g' from the previous-position plane instead (temporal_carry_device.h temporalCarry on plane[p]: no
// history unless its instance word is g's and it is finite); otherwise the plane is not read.
template<bool Trusted = false, bool Moving = false, bool Carried = false>
TWK_HD void temporalCascadePixel(const TemporalConstants& k, const CascadeConstants& c, const float4* Lc, const float4* geometry, const float4* H,
                                 const float4* hGeometry, const size_t stride, const size_t p, float4* out, const float* trust = nullptr,
                                 const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u, const float4* plane = nullptr)
{
  const int K = c.layers;
  const size_t top = (size_t) (K - 1) * stride;
  const float4 first = Lc[p], last = Lc[top + p];
  const float nc = first.w, rc = last.w;
  float  w[4];        // the counted taps' weights; 0: not counted. Tap t = 2 dy + dx is pixel q00 + dy width + dx of the history
  long long q00 = 0;
  float4 hFirst[4], hLast[4]; // layers 0 and K-1 of the counted taps: read for their counts, kept for their sums
  float  sn = 0.0f, srej = 0.0f, ws = 0.0f;
TWK_CASCADE_UNROLL
  for (int t = 0; t < 4; ++t) { w[t] = 0.0f; hFirst[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); hLast[t] = hFirst[t]; }
  if (k.hasHistory != 0)
  {
    const float4 g = geometry[p];
    float4 gp = g;
    float fx = 0.0f, fy = 0.0f, vv = 0.0f;
    if (asUint(g.w) != 0u && finite3(g) && cascadeFinite(nc) && !(nc < 1.0f) && (!Moving || temporalMove(motion, numMotion, g, gp)) &&
        (!Carried || temporalCarry(plane[p], g, gp)) && temporalProject(k, gp, fx, fy, vv))
    {
      const TemporalFootprint f = temporalFootprint(fx, fy);
      q00 = (long long) f.y0 * k.width + f.x0;
TWK_CASCADE_UNROLL
      for (int dy = 0; dy <= 1; ++dy)
      {
        const int qy = f.y0 + dy;
        if (qy < 0 || qy >= k.height) continue;
TWK_CASCADE_UNROLL
        for (int dx = 0; dx <= 1; ++dx)
        {
          const int qx = f.x0 + dx;
          if (qx < 0 || qx >= k.width) continue;
          const int t = 2 * dy + dx;
          const size_t qi = (size_t) qy * k.width + qx;
          if (!temporalTapGeometry(k, gp, hGeometry[qi], vv)) continue;
          const float4 h0 = H[qi];
          if (!cascadeFinite(h0.w) || !(h0.w >= 1.0f)) continue;
          const float4 h1 = H[top + qi];
          if (!cascadeFinite(h1.w)) continue;
          const float wt = temporalTapWeight(f, dx, dy);
          if (!(wt > 0.0f)) continue;
          w[t] = wt; hFirst[t] = h0; hLast[t] = h1;
          sn = sn + wt * h0.w; srej = srej + wt * h1.w; ws = ws + wt;
        }
      }
    }
  }
  if (!(ws > 0.0f))
  {
TWK_CASCADE_UNROLL
    for (int j = 0; j < TWK_CASCADE_MAX_LAYERS; ++j)
    {
      if (j >= K) continue;
      float4 cur; // (assigned, not chosen by ?: — a conditional between float4 lvalues takes their addresses and lands in scratch)
      if (j == 0) cur = first; else if (j == K - 1) cur = last; else cur = Lc[(size_t) j * stride + p];
      out[(size_t) j * stride + p] = cur;
    }
    return;
  }
  float hn = sn / ws, hrej = srej / ws, f = 1.0f;
  const bool capped = hn > k.maxHistory;
  if (capped) { f = k.maxHistory / hn; hrej = hrej * f; hn = k.maxHistory; }
  float t = 1.0f;
  if (Trusted) { t = trust[p]; hrej = hrej * t; hn = hn * t; }
TWK_CASCADE_UNROLL
  for (int j = 0; j < TWK_CASCADE_MAX_LAYERS; ++j)
  {
    if (j >= K) continue;
    float4 cur;
    if (j == 0) cur = first; else if (j == K - 1) cur = last; else cur = Lc[(size_t) j * stride + p];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
TWK_CASCADE_UNROLL
    for (int t = 0; t < 4; ++t)
    {
      if (!(w[t] > 0.0f)) continue;
      float4 h;
      if (j == 0) h = hFirst[t]; else if (j == K - 1) h = hLast[t]; else h = H[(size_t) j * stride + (size_t) (q00 + (long long) (t >> 1) * k.width + (t & 1))];
      sx = sx + w[t] * h.x; sy = sy + w[t] * h.y; sz = sz + w[t] * h.z;
    }
    float hx = sx / ws, hy = sy / ws, hz = sz / ws;
    if (capped) { hx = hx * f; hy = hy * f; hz = hz * f; }
    if (Trusted) { hx = hx * t; hy = hy * t; hz = hz * t; }
    out[(size_t) j * stride + p] = make_float4(hx + cur.x, hy + cur.y, hz + cur.z, (j == 0) ? hn + nc : ((j == K - 1) ? hrej + rc : 0.0f));
  }
}

} // namespace twk
