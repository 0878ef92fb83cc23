// The rectified temporal merge behind the C ABI (temporal_rectify_device.h: the definition): the parameters and their refusals, the
// explicit form, the own-buffer and the assembled form (both through device_post.hip's temporalOwn, which they share with the plain
// merge), the readers of the trust plane and the host-only form. The trusted cascade merge is device_temporal_cascade.hip's.
#include "device_handle.h"

#include <cstring>
#include <vector>

// The two scratch streams of the rectified merge, at least `pixels` float4 each
int twk::ensureRectifyScratch(TwkDevice dev, size_t pixels)
{
  if (dev->d_rectify[0] && dev->d_rectify[1] && dev->rectifyPixels >= pixels) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  for (int s = 0; s < 2; ++s) freeDevice(dev->d_rectify[s]);
  dev->rectifyPixels = 0;
  for (int s = 0; s < 2; ++s) HIP_TRY(hipMalloc(&dev->d_rectify[s], pixels * sizeof(float4)));
  dev->rectifyPixels = pixels;
  return TWK_SUCCESS;
}

static bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes)
{
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
  return x < y + bBytes && y < x + aBytes;
}

// The refusals of the parameters every form shares (tp, rp NULL: the defaults), and the constants they give; width, height unset
static int rectifyParameters(const char* name, const TwkTemporal* tp, const TwkTemporalRectify* rp, TemporalConstants& k, RectifyConstants& r)
{
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  TwkTemporal temporal; temporal.maxHistory = TWK_TEMPORAL_MAX_HISTORY; temporal.positionTolerance = TWK_TEMPORAL_POSITION_TOLERANCE;
  if (tp) temporal = *tp;
  TwkTemporalRectify rectify; rectify.radius = TWK_TEMPORAL_RECTIFY_RADIUS; rectify.minTaps = TWK_TEMPORAL_RECTIFY_MIN_TAPS; rectify.gamma = TWK_TEMPORAL_RECTIFY_GAMMA;
  if (rp) rectify = *rp;
  if (temporal.maxHistory < 1) return refuse("maxHistory must be >= 1");
  if (!(temporal.positionTolerance >= 0.0f) || !finite1(temporal.positionTolerance)) return refuse("positionTolerance must be >= 0 and finite");
  static_assert(TWK_TEMPORAL_RECTIFY_MAX_RADIUS == TWK_RECTIFY_MAX_RADIUS, "the header's largest radius is the kernel's");
  if (rectify.radius < 1 || rectify.radius > TWK_RECTIFY_MAX_RADIUS) return refuse("radius must be in 1..4");
  if (rectify.minTaps < 2) return refuse("minTaps must be >= 2 (a variance needs two taps)");
  if (!(rectify.gamma >= 0.0f) || !finite1(rectify.gamma)) return refuse("gamma must be >= 0 and finite");
  memset(&k, 0, sizeof(k));
  k.maxHistory = (float) temporal.maxHistory; k.tol2 = temporal.positionTolerance * temporal.positionTolerance;
  r.radius = rectify.radius; r.minTaps = rectify.minTaps; r.gamma2 = rectify.gamma * rectify.gamma;
  return TWK_SUCCESS;
}

extern "C" {

int twk_temporal_rectify_defaults(TwkTemporalRectify* rp)
try
{
  if (!rp) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_temporal_rectify_defaults: NULL argument");
  rp->radius = TWK_TEMPORAL_RECTIFY_RADIUS; rp->minTaps = TWK_TEMPORAL_RECTIFY_MIN_TAPS; rp->gamma = TWK_TEMPORAL_RECTIFY_GAMMA;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_rectify_defaults")

int twk_temporal_accumulate_rectified(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalRectify* rp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                                      int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut)
try
{
  const char* name = "twk_temporal_accumulate_rectified";
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, (std::string(name) + ": " + text).c_str()); };
  int rc = activate(dev, name); if (rc) return rc;
  TemporalConstants k;
  RectifyConstants r;
  if ((rc = rectifyParameters(name, tp, rp, k, r))) return rc;
  if (!current)
  {
    if (history || colourOut || historyOut || momentsOut || trustOut || width || height)
      return refuse(TWK_ERROR_INVALID_VALUE, "a history, outputs or a size without a current frame (pass both frames, or neither for the handle's own buffers)");
    return temporalOwnFrame(dev, name, k, &r);
  }
  if (width < 1 || height < 1 || (size_t) width * (size_t) height >= ((size_t) 1 << 31)) return refuse(TWK_ERROR_INVALID_VALUE, "width and height must be >= 1");
  if (!current->colour || !current->moments || !current->geometry) return refuse(TWK_ERROR_INVALID_VALUE, "NULL buffer in the current frame");
  if (history && (!history->colour || !history->moments || !history->geometry)) return refuse(TWK_ERROR_INVALID_VALUE, "NULL buffer in the history frame");
  const void* colour = current->colour;
  const float4 *moments = static_cast<const float4*>(current->moments), *geometry = static_cast<const float4*>(current->geometry);
  const float4 *hColour = nullptr, *hMoments = nullptr, *hGeometry = nullptr;
  if (history) { hColour = static_cast<const float4*>(history->colour); hMoments = static_cast<const float4*>(history->moments); hGeometry = static_cast<const float4*>(history->geometry); }
  const size_t n = (size_t) width * height, wide = n * sizeof(float4), narrowBytes = n * pixelBytes(dev);
  const void* outs[4] = {colourOut, historyOut, momentsOut, trustOut}; const size_t outBytes[4] = {narrowBytes, wide, wide, n * sizeof(float)};
  const void* ins[6] = {colour, moments, geometry, hColour, hMoments, hGeometry}; const size_t inBytes[6] = {narrowBytes, wide, wide, wide, wide, wide};
  for (int o = 0; o < 4; ++o)
  {
    for (int i = 0; i < 6; ++i) if (overlaps(outs[o], outBytes[o], ins[i], inBytes[i])) return refuse(TWK_ERROR_INVALID_VALUE, "an output overlaps an input (the kernel gathers the history at other pixels)");
    for (int j = o + 1; j < 4; ++j) if (overlaps(outs[o], outBytes[o], outs[j], outBytes[j])) return refuse(TWK_ERROR_INVALID_VALUE, "two outputs overlap");
  }
  k.width = width; k.height = height;
  if (history)
  {
    k.hasHistory = 1;
    if (!temporalCamera(history->camera.P, k)) return refuse(TWK_ERROR_INVALID_VALUE, "the history's camera is degenerate: U, V, W are linearly dependent or not finite");
  }
  if ((rc = ensureRectifyScratch(dev, n))) return rc;
  launchTemporalRectify(colour, halfOutput(dev), moments, geometry, hColour, hMoments, hGeometry, dev->d_rectify[0], dev->d_rectify[1], colourOut, static_cast<float4*>(historyOut),
                        static_cast<float4*>(momentsOut), static_cast<float*>(trustOut), k, r, dev->stream);
  HIP_TRY(hipGetLastError());
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_accumulate_rectified")

int twk_temporal_accumulate_assembled_rectified(TwkDevice primary, const TwkTemporal* tp, const TwkTemporalRectify* rp)
try
{
  const char* name = "twk_temporal_accumulate_assembled_rectified";
  int rc = activate(primary, name); if (rc) return rc;
  TemporalConstants k;
  RectifyConstants r;
  if ((rc = rectifyParameters(name, tp, rp, k, r))) return rc;
  return temporalAssembledFrame(primary, name, k, &r);
}
TWK_CATCH("twk_temporal_accumulate_assembled_rectified")

int twk_get_temporal_trust_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  int rc = activate(dev, "twk_get_temporal_trust_device_pointer"); if (rc) return rc;
  if (!dptr) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_temporal_trust_device_pointer: NULL argument");
  if (!dev->temporalValid || !dev->temporalTrustValid || !dev->d_temporalTrust)
    return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_temporal_trust_device_pointer: the last merge on the handle's own buffers was no twk_temporal_accumulate_rectified, or its history has been dropped");
  *dptr = dev->d_temporalTrust;
  if (bytes) *bytes = (size_t) dev->temporalWidth * dev->temporalHeight * sizeof(float);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_temporal_trust_device_pointer")

int twk_read_temporal_trust(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_temporal_trust"); if (rc) return rc;
  if (!host) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_temporal_trust: NULL buffer");
  if (!dev->temporalValid || !dev->temporalTrustValid || !dev->d_temporalTrust)
    return twkSetError(TWK_ERROR_INVALID_STATE, "twk_read_temporal_trust: the last merge on the handle's own buffers was no twk_temporal_accumulate_rectified, or its history has been dropped");
  const size_t n = (size_t) dev->temporalWidth * dev->temporalHeight;
  if (numFloats != n) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_temporal_trust: buffer must hold width*height floats");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  HIP_TRY(hipMemcpy(host, dev->d_temporalTrust, n * sizeof(float), hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_read_temporal_trust")

int twk_temporal_rectify_host(const TwkTemporal* tp, const TwkTemporalRectify* rp, const float* colour, const float* moments, const float* geometry,
                              const float* historyColour, const float* historyMoments, const float* historyGeometry, const TwkCameraDefinition* historyCamera,
                              int width, int height, float* colourOut, float* momentsOut, float* trustOut)
try
{
  const char* name = "twk_temporal_rectify_host";
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!colour || !moments || !geometry) return refuse("NULL buffer in the current frame");
  const bool history = historyColour || historyMoments || historyGeometry;
  if (history && (!historyColour || !historyMoments || !historyGeometry || !historyCamera)) return refuse("a history without its colour, moments, geometry or camera");
  TemporalConstants k;
  RectifyConstants r;
  int rc = rectifyParameters(name, tp, rp, k, r); if (rc) return rc;
  if (width < 1 || height < 1 || (size_t) width * (size_t) height > ((size_t) 1 << 28)) return refuse("width and height must be >= 1, width*height at most 2^28");
  k.width = width; k.height = height;
  if (history)
  {
    k.hasHistory = 1;
    if (!temporalCamera(historyCamera->P, k)) return refuse("the history's camera is degenerate: U, V, W are linearly dependent or not finite");
  }
  const size_t n = (size_t) width * height;
  // (a host array of floats need not have a float4's alignment)
  std::vector<float4> cur(n), mc(n), g(n), hc(history ? n : 0), hm(history ? n : 0), hg(history ? n : 0), A(n), B(n);
  memcpy(cur.data(), colour, n * sizeof(float4)); memcpy(mc.data(), moments, n * sizeof(float4)); memcpy(g.data(), geometry, n * sizeof(float4));
  if (history) { memcpy(hc.data(), historyColour, n * sizeof(float4)); memcpy(hm.data(), historyMoments, n * sizeof(float4)); memcpy(hg.data(), historyGeometry, n * sizeof(float4)); }
  // launch 1
  for (size_t p = 0; p < n; ++p) rectifyReproject(k, cur[p], mc[p], g[p], hc.data(), hm.data(), hg.data(), A[p], B[p]);
  // launch 2: the staged words of the whole picture with a halo of `radius` zeros around it, as one tile
  const int R = r.radius, pitch = width + 2 * R;
  std::vector<float> d((size_t) pitch * (height + 2 * R), 0.0f);
  std::vector<unsigned int> key(d.size(), 0u);
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x)
    {
      const size_t p = (size_t) y * width + x, s = (size_t) (y + R) * pitch + (x + R);
      rectifyStage(mc[p], B[p], d[s], key[s]);
    }
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x)
    {
      const size_t p = (size_t) y * width + x;
      const float t = rectifyTrust<0>(r, d.data(), key.data(), pitch, (y + R) * pitch + (x + R), B[p].z, mc[p].z);
      float4 c = cur[p], m = mc[p];
      float trust;
      if (!rectifyMerge(t, cur[p], mc[p], A[p], B[p], c, m, trust)) { c = cur[p]; m = mc[p]; }
      if (colourOut) memcpy(colourOut + 4 * p, &c, sizeof(float4));
      if (momentsOut) memcpy(momentsOut + 4 * p, &m, sizeof(float4));
      if (trustOut) trustOut[p] = trust;
    }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_rectify_host")

} // extern "C"
