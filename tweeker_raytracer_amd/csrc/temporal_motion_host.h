// The host-only forms of the temporal merges, after their refusals: the definitions of temporal_device.h,
// temporal_rectify_device.h and temporal_cascade_device.h run pixel by pixel on host arrays, with or without a table of instance
// motion (temporal_motion_device.h). Written once here for twk_temporal_rectify_host, twk_temporal_cascade_host,
// twk_temporal_cascade_trusted_host, twk_temporal_moving_host and twk_temporal_cascade_moving_host (device_temporal.hip,
// device_temporal_cascade.hip), and for tests/temporal_motion_host.cpp, which compiles them with the sanitizers. No HIP call, no
// error state: k, r and c are the constants the entry points made of their checked parameters. Host arrays of floats need not
// have a float4's alignment and are copied.
#pragma once
#include "temporal_rectify_device.h"
#include "temporal_cascade_device.h"

#include <cstring>
#include <vector>

namespace twk {

// The frame and the history (historyColour nullptr: none, k.hasHistory 0) as float4 arrays
struct TemporalHostFrame
{
  std::vector<float4> cur, mc, g, hc, hm, hg;
  TemporalHostFrame(size_t n, const float* colour, const float* moments, const float* geometry, const float* historyColour, const float* historyMoments, const float* historyGeometry)
    : cur(n), mc(n), g(n), hc(historyColour ? n : 0), hm(historyColour ? n : 0), hg(historyColour ? n : 0)
  {
    memcpy(cur.data(), colour, n * sizeof(float4)); memcpy(mc.data(), moments, n * sizeof(float4)); memcpy(g.data(), geometry, n * sizeof(float4));
    if (historyColour) { memcpy(hc.data(), historyColour, n * sizeof(float4)); memcpy(hm.data(), historyMoments, n * sizeof(float4)); memcpy(hg.data(), historyGeometry, n * sizeof(float4)); }
  }
};

// temporalKernel / temporalMovingKernel on the host: colourOut, momentsOut (either may be nullptr) width x height x 4 floats
// Carried: the Carried build, plane (width x height float4) in place of the table
template<bool Moving, bool Carried = false>
inline void temporalPlainHost(const TemporalConstants& k, const TemporalHostFrame& f, const TwkInstanceMotion* motion, unsigned int numMotion, float* colourOut, float* momentsOut,
                              const float4* plane = nullptr)
{
  const size_t n = (size_t) k.width * k.height;
  for (size_t p = 0; p < n; ++p)
  {
    float4 c = f.cur[p], m = f.mc[p];
    TemporalSums s;
    temporalGather<Moving, Carried>(k, f.cur[p], f.mc[p], f.g[p], f.hc.data(), f.hm.data(), f.hg.data(), s, motion, numMotion, Carried ? plane[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    if (s.ws > 0.0f) temporalMerge(k, s, f.cur[p], f.mc[p], c, m);
    if (colourOut) memcpy(colourOut + 4 * p, &c, sizeof(float4));
    if (momentsOut) memcpy(momentsOut + 4 * p, &m, sizeof(float4));
  }
}

// The two launches of the rectified merge on the host; trustOut (may be nullptr) width x height floats
template<bool Moving, bool Carried = false>
inline void temporalRectifyHost(const TemporalConstants& k, const RectifyConstants& r, const TemporalHostFrame& f, const TwkInstanceMotion* motion, unsigned int numMotion,
                                float* colourOut, float* momentsOut, float* trustOut, const float4* plane = nullptr)
{
  const int width = k.width, height = k.height;
  const size_t n = (size_t) width * height;
  std::vector<float4> A(n), B(n);
  // launch 1
  for (size_t p = 0; p < n; ++p) rectifyReproject<Moving, Carried>(k, f.cur[p], f.mc[p], f.g[p], f.hc.data(), f.hm.data(), f.hg.data(), A[p], B[p], motion, numMotion,
                                                                    Carried ? plane[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  // launch 2: the staged words of the whole picture with a halo of `radius` zeros around it, as one tile
  const int R = r.radius, pitch = width + 2 * R;
  std::vector<float> d((size_t) pitch * (height + 2 * R), 0.0f);
  std::vector<unsigned int> key(d.size(), 0u);
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x)
    {
      const size_t p = (size_t) y * width + x, s = (size_t) (y + R) * pitch + (x + R);
      rectifyStage(f.mc[p], B[p], d[s], key[s]);
    }
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x)
    {
      const size_t p = (size_t) y * width + x;
      const float t = rectifyTrust<0>(r, d.data(), key.data(), pitch, (y + R) * pitch + (x + R), B[p].z, f.mc[p].z);
      float4 c = f.cur[p], m = f.mc[p];
      float trust;
      if (!rectifyMerge(t, f.cur[p], f.mc[p], A[p], B[p], c, m, trust)) { c = f.cur[p]; m = f.mc[p]; }
      if (colourOut) memcpy(colourOut + 4 * p, &c, sizeof(float4));
      if (momentsOut) memcpy(momentsOut + 4 * p, &m, sizeof(float4));
      if (trustOut) trustOut[p] = trust;
    }
}

// The plain (r nullptr) or the rectified merge, with a table (motion, numMotion > 0) or without
inline void temporalMergeHost(const TemporalConstants& k, const RectifyConstants* r, const TemporalHostFrame& f, const TwkInstanceMotion* motion, unsigned int numMotion,
                              float* colourOut, float* momentsOut, float* trustOut, const float* previousPositions = nullptr)
{
  if (previousPositions) // the Carried builds: the plane in place of the table
  {
    std::vector<float4> plane((size_t) k.width * k.height);
    memcpy(plane.data(), previousPositions, plane.size() * sizeof(float4));
    if (r) temporalRectifyHost<false, true>(k, *r, f, nullptr, 0u, colourOut, momentsOut, trustOut, plane.data());
    else   temporalPlainHost<false, true>(k, f, nullptr, 0u, colourOut, momentsOut, plane.data());
    return;
  }
  const bool moving = motion && numMotion > 0u;
  if (r) { if (moving) temporalRectifyHost<true>(k, *r, f, motion, numMotion, colourOut, momentsOut, trustOut); else temporalRectifyHost<false>(k, *r, f, nullptr, 0u, colourOut, momentsOut, trustOut); }
  else   { if (moving) temporalPlainHost<true>(k, f, motion, numMotion, colourOut, momentsOut); else temporalPlainHost<false>(k, f, nullptr, 0u, colourOut, momentsOut); }
}

// The cascade's merge on the host: layers [c.layers][width x height x 4] floats; historyLayers nullptr: none (k.hasHistory 0);
// trust nullptr: the plain build, else the trusted one
inline void temporalCascadeHostLayers(const TemporalConstants& k, const CascadeConstants& c, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                                      const float* historyGeometry, const float* trust, const TwkInstanceMotion* motion, unsigned int numMotion, float* layersOut,
                                      const float* previousPositions = nullptr)
{
  const size_t n = (size_t) k.width * k.height, all = n * (size_t) c.layers;
  std::vector<float4> plane(previousPositions ? n : 0);
  if (previousPositions) memcpy(plane.data(), previousPositions, n * sizeof(float4));
  std::vector<float4> layers(all), geometry(n), history(historyLayers ? all : 0), hGeometry(historyLayers ? n : 0), out(all);
  memcpy(layers.data(), currentLayers, all * sizeof(float4));
  memcpy(geometry.data(), currentGeometry, n * sizeof(float4));
  if (historyLayers)
  {
    memcpy(history.data(), historyLayers, all * sizeof(float4));
    memcpy(hGeometry.data(), historyGeometry, n * sizeof(float4));
  }
  const float4* H = historyLayers ? history.data() : nullptr;
  const float4* hG = historyLayers ? hGeometry.data() : nullptr;
  const bool moving = motion && numMotion > 0u;
  for (size_t p = 0; p < n; ++p)
  {
    if (previousPositions) // the Carried builds
    {
      if (trust) temporalCascadePixel<true, false, true>(k, c, layers.data(), geometry.data(), H, hG, n, p, out.data(), trust, nullptr, 0u, plane.data());
      else       temporalCascadePixel<false, false, true>(k, c, layers.data(), geometry.data(), H, hG, n, p, out.data(), nullptr, nullptr, 0u, plane.data());
      continue;
    }
    if (trust) { if (moving) temporalCascadePixel<true, true>(k, c, layers.data(), geometry.data(), H, hG, n, p, out.data(), trust, motion, numMotion);
                 else        temporalCascadePixel<true>(k, c, layers.data(), geometry.data(), H, hG, n, p, out.data(), trust); }
    else       { if (moving) temporalCascadePixel<false, true>(k, c, layers.data(), geometry.data(), H, hG, n, p, out.data(), nullptr, motion, numMotion);
                 else        temporalCascadePixel(k, c, layers.data(), geometry.data(), H, hG, n, p, out.data()); }
  }
  memcpy(layersOut, out.data(), all * sizeof(float4));
}

} // namespace twk
