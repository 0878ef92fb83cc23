// What runs on finished pictures: compositor, tonemapper, the a-trous denoiser (≙ optixDenoiserInvoke, Optix7Gui
// Application.cpp:2478) and the noise estimate. The temporal merge is device_temporal.hip's. The internal denoised picture is a
// DevicePicture, the filter's streams a scratch array grown by growIdle (device_handle.h).
#include "device_handle.h"

#include <cmath>
#include <cstring>
#include <vector>

// =============================================================================================
extern "C" {

static int compositor(TwkDevice dev, const void* tiles, void* output, bool half, const char* where)
{
  int rc = activate(dev, where); if (rc) return rc;
  if (!tiles || !output) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(where) + ": NULL buffer");
  if (!dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, std::string(where) + ": twk_set_state first");
  launchCompositor(tiles, output, half, dev->state.resolution[0], dev->state.resolution[1],
                   dev->launchWidth, dev->count, dev->state.tileSize[0], calculateShift(dev->state.tileSize[0]), calculateShift(dev->state.tileSize[1]), dev->stream);
  HIP_TRY(hipGetLastError());
  return TWK_SUCCESS;
}

int twk_compositor(TwkDevice dev, const void* tiles, void* output)
try
{
  return compositor(dev, tiles, output, false, "twk_compositor");
}
TWK_CATCH("twk_compositor")

int twk_compositor_half(TwkDevice dev, const void* tiles, void* output)
try
{
  return compositor(dev, tiles, output, true, "twk_compositor_half");
}
TWK_CATCH("twk_compositor_half")

static int tonemap(TwkDevice dev, const TwkTonemapper* tm, const void* src, bool half, size_t numPixels, unsigned char* rgb8Host)
{
  if (numPixels == 0) return TWK_SUCCESS;
  DeviceArray<unsigned char> ldr;
  const int rc = ldr.allocate(numPixels * 3); if (rc) return rc;
  launchTonemap(src, half, ldr, numPixels, *tm, dev->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(rgb8Host, ldr, numPixels * 3, hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  return TWK_SUCCESS;
}

int twk_tonemap(TwkDevice dev, const TwkTonemapper* tm, const void* rgbaDevice, size_t numPixels, unsigned char* rgb8Host)
try
{
  int rc = activate(dev, "twk_tonemap"); if (rc) return rc;
  if (!tm || !rgb8Host) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_tonemap: NULL argument");
  if (!(tm->gamma > 0.0f) || !(tm->whitePoint > 0.0f)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_tonemap: gamma and whitePoint must be positive");
  if (rgbaDevice) return tonemap(dev, tm, rgbaDevice, false, numPixels, rgb8Host);
  // the handle's own buffer, in whatever format it holds
  const float4* src = ownOutput(dev);
  if (!src || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_tonemap: nothing has been rendered");
  if (numPixels != launchIndices(dev)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_tonemap: numPixels must be launchWidth*height for the handle's own buffer");
  return tonemap(dev, tm, src, halfOutput(dev), numPixels, rgb8Host);
}
TWK_CATCH("twk_tonemap")

int twk_tonemap_half(TwkDevice dev, const TwkTonemapper* tm, const void* rgbaHalfDevice, size_t numPixels, unsigned char* rgb8Host)
try
{
  int rc = activate(dev, "twk_tonemap_half"); if (rc) return rc;
  if (!tm || !rgbaHalfDevice || !rgb8Host) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_tonemap_half: NULL argument");
  if (!(tm->gamma > 0.0f) || !(tm->whitePoint > 0.0f)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_tonemap_half: gamma and whitePoint must be positive");
  return tonemap(dev, tm, rgbaHalfDevice, true, numPixels, rgb8Host);
}
TWK_CATCH("twk_tonemap_half")

// ---- denoiser ---------------------------------------------------------------------------------
int twk_denoiser_defaults(TwkDenoiser* dn)
try
{
  if (!dn) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoiser_defaults: NULL argument");
  dn->inputKind = TWK_DENOISER_RGB_ALBEDO_NORMAL;
  dn->iterations = 3;
  dn->sigmaColor = 8.0f; dn->sigmaNormal = 0.3f; dn->sigmaAlbedo = 0.1f;
  dn->demodulateAlbedo = 1;
  dn->blendFactor = 0.0f;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_denoiser_defaults")

// Every check of the parameters' values, for the device form and the host form alike, and the constants the passes take (k but
// for its width and height). `name` is the entry point, for the error texts; dv NULL: not the variance-guided mode; dg NULL: no
// geometry guide; minSamples 0: no sampled variance; `moments`: the caller gave a moments buffer
static int denoiseParameters(const char* name, const TwkDenoiser* dn, const TwkDenoiserVariance* dv, const TwkDenoiserGeometry* dg, int minSamples, bool moments, DenoiseConstants& k)
{
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, (std::string(name) + ": " + text).c_str()); };
  const int kind = dn->inputKind;
  if (kind != TWK_DENOISER_RGB && kind != TWK_DENOISER_RGB_ALBEDO && kind != TWK_DENOISER_RGB_ALBEDO_NORMAL) return refuse("unknown inputKind");
  if (minSamples != 0 && !dv) return refuse("minSamples without the parameters of the variance-guided mode");
  if (minSamples != 0 && minSamples < 2) return refuse("minSamples must be 0 (no sampled variance) or >= 2 (one sample has no variance)");
  if (minSamples == 0 && moments) return refuse("a moments buffer without minSamples");
  if (dg)
  {
    if (kind != TWK_DENOISER_RGB_ALBEDO_NORMAL) return refuse("the geometry guide needs inputKind TWK_DENOISER_RGB_ALBEDO_NORMAL (the plane's normal comes from the normal guide)");
    const float invPosition = 1.0f / (dg->sigmaPosition * dg->sigmaPosition);
    if (!(dg->sigmaPosition > 0.0f) || !std::isfinite(invPosition) || !(invPosition > 0.0f)) return refuse("sigmaPosition must be > 0 and 1 / sigmaPosition^2 a finite positive float");
  }
  if (dn->iterations < 0 || dn->iterations > 8) return refuse("iterations must be in [0, 8]");
  if ((!dv && !(dn->sigmaColor > 0.0f)) || (kind >= TWK_DENOISER_RGB_ALBEDO && !(dn->sigmaAlbedo > 0.0f)) || (kind >= TWK_DENOISER_RGB_ALBEDO_NORMAL && !(dn->sigmaNormal > 0.0f)))
    return refuse("the sigma of every guide in use must be positive");
  k.width = 0; k.height = 0;
  k.invColor  = dv ? 0.0f : 1.0f / (dn->sigmaColor * dn->sigmaColor);
  k.invNormal = (kind >= TWK_DENOISER_RGB_ALBEDO_NORMAL) ? 1.0f / (dn->sigmaNormal * dn->sigmaNormal) : 0.0f;
  k.invAlbedo = (kind >= TWK_DENOISER_RGB_ALBEDO) ? 1.0f / (dn->sigmaAlbedo * dn->sigmaAlbedo) : 0.0f;
  k.blendFactor = dn->blendFactor;
  k.demodulate = dn->demodulateAlbedo ? 1 : 0;
  k.fireflyThreshold = dv ? dv->fireflyThreshold : 0.0f;
  k.sigmaLuminance = dv ? dv->sigmaLuminance : 0.0f;
  // 1 / sigma^2 is what the passes multiply by: a sigma whose square underflows would make it inf, and 0 x inf the centre tap's NaN
  if (!std::isfinite(k.invColor) || !std::isfinite(k.invNormal) || !std::isfinite(k.invAlbedo)) return refuse("a sigma is too small: 1 / sigma^2 is not a finite float");
  if (!(dn->blendFactor >= 0.0f && dn->blendFactor <= 1.0f)) return refuse("blendFactor must be in [0, 1]");
  if (dn->demodulateAlbedo && kind == TWK_DENOISER_RGB) return refuse("demodulateAlbedo needs an albedo guide (inputKind TWK_DENOISER_RGB has none)");
  if (dv)
  {
    if (!(dv->fireflyThreshold >= 0.0f) || !std::isfinite(dv->fireflyThreshold)) return refuse("fireflyThreshold must be >= 0 (0 = no clamp) and finite");
    if (!(dv->sigmaLuminance > 0.0f) || !std::isfinite(dv->sigmaLuminance)) return refuse("sigmaLuminance must be > 0 and finite");
  }
  return TWK_SUCCESS;
}

// twk_denoise (dv NULL), twk_denoise_variance and twk_denoise_variance_sampled (minSamples > 0; `moments`: the caller's buffer
// beside an explicit beauty): `name` is the entry point, for its error texts. dg (twk_denoise_geometry): the geometry guide, with
// `geometry` the caller's buffer beside an explicit beauty and `camera` (12 floats P, U, V, W; NULL: the handle's camera 0) the one
// the geometry was traced from
static int denoise(const char* name, TwkDevice dev, const TwkDenoiser* dn, const TwkDenoiserVariance* dv, const void* beauty, const void* albedo, const void* normal, int width, int height, void* denoised,
                   int minSamples = 0, const void* moments = nullptr, const TwkDenoiserGeometry* dg = nullptr, const void* geometry = nullptr, const float* camera = nullptr)
{
  const bool sampled = (minSamples > 0);
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, (std::string(name) + ": " + text).c_str()); };
  const int kind = dn->inputKind;
  DenoiseConstants k;
  int rc = denoiseParameters(name, dn, dv, dg, minSamples, moments != nullptr, k); if (rc) return rc;
  rc = activate(dev, name); if (rc) return rc;

  const bool own = (beauty == nullptr);
  if (own)
  {
    if (albedo || normal || moments || geometry) return refuse(TWK_ERROR_INVALID_VALUE, "guides without a beauty buffer (pass every input, or none for the handle's own buffers)");
    if (!dev->stateSet) return refuse(TWK_ERROR_INVALID_STATE, "twk_set_state first");
    if (dev->state.distribution && 1 < dev->count) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffer is a packed tile buffer (distribution 1, more than one device), not a picture; denoise the composited frame");
    beauty = ownOutput(dev);
    if (!beauty) return refuse(TWK_ERROR_INVALID_STATE, "nothing has been rendered");
    width = dev->launchWidth; height = dev->state.resolution[1];
    const size_t n = launchIndices(dev);
    if (kind != TWK_DENOISER_RGB)
    {
      if (!ownAlbedo(dev, n) || !ownNormal(dev, n)) return refuse(TWK_ERROR_INVALID_STATE, "a guided inputKind on the handle's own buffers needs a render with twk_enable_aov(1)");
      albedo = dev->d_aovAlbedo;
      if (kind == TWK_DENOISER_RGB_ALBEDO_NORMAL) normal = dev->d_aovNormal;
    }
    if (sampled && !(moments = ownMoments(dev, n))) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffers have no luminance moments: render with twk_enable_moments(1)");
    if (dg)
    {
      if (!(geometry = ownGeometry(dev, n))) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffers have no geometry AOV: twk_enable_geometry(1) and twk_render_geometry");
      if (!dev->geometryValid) return refuse(TWK_ERROR_INVALID_STATE, "the geometry AOV is older than the camera, the state or the scene: twk_render_geometry first");
    }
  }
  else
  {
    if (width < 1 || height < 1) return refuse(TWK_ERROR_INVALID_VALUE, "width and height must be >= 1");
    if ((kind >= TWK_DENOISER_RGB_ALBEDO && !albedo) || (kind >= TWK_DENOISER_RGB_ALBEDO_NORMAL && !normal)) return refuse(TWK_ERROR_INVALID_VALUE, "NULL guide buffer for a guide the inputKind uses");
    if (kind < TWK_DENOISER_RGB_ALBEDO) albedo = nullptr;        // guides the kind does not use are not read
    if (kind < TWK_DENOISER_RGB_ALBEDO_NORMAL) normal = nullptr;
    if (sampled && !moments) return refuse(TWK_ERROR_INVALID_VALUE, "NULL moments buffer beside an explicit beauty buffer");
    if (dg && !geometry) return refuse(TWK_ERROR_INVALID_VALUE, "NULL geometry buffer beside an explicit beauty buffer");
  }
  const size_t numPixels = (size_t) width * height, bytes = numPixels * pixelBytes(dev);
  DenoiseGeometryConstants g = DenoiseGeometryConstants();
  if (dg)
  {
    if (!camera)
    {
      if (dev->cameras.empty()) return refuse(TWK_ERROR_INVALID_STATE, "no camera given and the handle has none: twk_init_cameras first");
      camera = dev->cameras[0].P;
    }
    if (!denoiseGeometryConstants(camera, dg->sigmaPosition, dg->instanceStop, g)) return refuse(TWK_ERROR_INVALID_VALUE, "the camera is degenerate: P is not finite, or U, V or W does not normalise");
    if (overlaps(denoised, bytes, geometry, numPixels * sizeof(float4))) return refuse(TWK_ERROR_INVALID_VALUE, "the denoised buffer overlaps an input");
  }
  if (denoised && (overlaps(denoised, beauty, bytes) || overlaps(denoised, albedo, bytes) || overlaps(denoised, normal, bytes) || (sampled && overlaps(denoised, bytes, moments, numPixels * sizeof(float4)))))
    return refuse(TWK_ERROR_INVALID_VALUE, "the denoised buffer overlaps an input");

  void* target = denoised;
  if (!target)
  {
    if ((rc = ensurePicture(dev, dev->denoised, width, height))) return rc;
    target = dev->denoised.pixels;
  }
  if (dn->iterations == 0 || dn->blendFactor == 1.0f)
  {
    HIP_TRY(hipMemcpyAsync(target, beauty, bytes, hipMemcpyDeviceToDevice, dev->stream)); // the input's bits
  }
  else
  {
    if ((rc = growIdle(dev, dev->d_denoiseStreams, numPixels * 4))) return rc;
    float4* colour[2] = {dev->d_denoiseStreams, dev->d_denoiseStreams + numPixels};
    float4* guideNormal = dev->d_denoiseStreams + 2 * numPixels;
    float4* guideAlbedo = dev->d_denoiseStreams + 3 * numPixels;
    k.width = width; k.height = height;
    // the variance-guided mode: prepare writes the pong stream and the moments pass the ping stream (clamped colour, variance in
    // .w), so that the levels ping-pong as without it and the mode needs no stream of its own
    launchDenoisePrepare(beauty, albedo, normal, halfOutput(dev), colour[dv ? 1 : 0], guideNormal, guideAlbedo, k, dev->stream);
    // the geometry guide: its stream is read where it lies (already f32). With four streams per tap the staged build of the level
    // wins up to step 16 (measured per step, profiles/r20_denoise_geometry.md), so the GEO builds have a border of their own.
    const int ldsMaxStep = dg ? dev->denoiseGeometryLdsMaxStep : dev->denoiseLdsMaxStep;
    const float4* guideGeometry = dg ? static_cast<const float4*>(geometry) : nullptr;
    if (dv) launchDenoiseMoments(kind, colour[1], guideNormal, guideAlbedo, colour[0], k, sampled ? static_cast<const float4*>(moments) : nullptr, (float) minSamples, dev->stream, guideGeometry, &g);
    for (int level = 0; level < dn->iterations; ++level)
      launchDenoiseLevel(kind, (1 << level) <= ldsMaxStep, dv != nullptr, colour[level & 1], guideNormal, guideAlbedo, colour[(level + 1) & 1], k, 1 << level, dev->stream, guideGeometry, &g);
    launchDenoiseFinish(beauty, halfOutput(dev), colour[dn->iterations & 1], normal ? guideNormal : nullptr, albedo ? guideAlbedo : nullptr, target, k, dev->stream);
    HIP_TRY(hipGetLastError());
  }
  if (!denoised) dev->denoised.valid = true;
  return TWK_SUCCESS;
}

int twk_denoise(TwkDevice dev, const TwkDenoiser* dn, const void* beauty, const void* albedo, const void* normal, int width, int height, void* denoised)
try
{
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise: NULL device handle");
  if (!dn) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise: NULL parameters");
  return denoise("twk_denoise", dev, dn, nullptr, beauty, albedo, normal, width, height, denoised);
}
TWK_CATCH("twk_denoise")

int twk_denoiser_variance_defaults(TwkDenoiserVariance* dv)
try
{
  if (!dv) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoiser_variance_defaults: NULL argument");
  dv->fireflyThreshold = 3.0f;
  dv->sigmaLuminance = 4.0f;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_denoiser_variance_defaults")

int twk_denoise_variance(TwkDevice dev, const TwkDenoiser* dn, const TwkDenoiserVariance* dv, const void* beauty, const void* albedo, const void* normal, int width, int height, void* denoised)
try
{
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise_variance: NULL device handle");
  if (!dn || !dv) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise_variance: NULL parameters");
  return denoise("twk_denoise_variance", dev, dn, dv, beauty, albedo, normal, width, height, denoised);
}
TWK_CATCH("twk_denoise_variance")

int twk_denoise_variance_sampled(TwkDevice dev, const TwkDenoiser* dn, const TwkDenoiserVariance* dv, int minSamples, const void* beauty, const void* albedo, const void* normal,
                                 const void* moments, int width, int height, void* denoised)
try
{
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise_variance_sampled: NULL device handle");
  if (!dn || !dv) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise_variance_sampled: NULL parameters");
  if (minSamples < 2) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise_variance_sampled: minSamples must be >= 2 (one sample has no variance)");
  return denoise("twk_denoise_variance_sampled", dev, dn, dv, beauty, albedo, normal, width, height, denoised, minSamples, moments);
}
TWK_CATCH("twk_denoise_variance_sampled")

int twk_denoiser_geometry_defaults(TwkDenoiserGeometry* dg)
try
{
  if (!dg) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoiser_geometry_defaults: NULL argument");
  dg->sigmaPosition = TWK_DENOISER_SIGMA_POSITION;
  dg->instanceStop = 0;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_denoiser_geometry_defaults")

int twk_denoise_geometry(TwkDevice dev, const TwkDenoiser* dn, const TwkDenoiserGeometry* dg, const TwkDenoiserVariance* dv, int minSamples, const void* beauty, const void* albedo,
                         const void* normal, const void* moments, const void* geometry, const float* camera, int width, int height, void* denoised)
try
{
  const char* name = "twk_denoise_geometry";
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise_geometry: NULL device handle");
  if (!dn || !dg) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_denoise_geometry: NULL parameters");
  return denoise(name, dev, dn, dv, beauty, albedo, normal, width, height, denoised, minSamples, moments, dg, geometry, camera);
}
TWK_CATCH("twk_denoise_geometry")

// The host form: the passes of denoise_kernels.hip as plain loops over the pixels, calling the same four bodies (denoise_device.h
// compiled for the host) with the global tap source on host pointers. RGBA32F, all three modes. The pixels of a pass are
// independent, so the order of the loops plays no part.
int twk_denoise_geometry_host(const TwkDenoiser* dn, const TwkDenoiserGeometry* dg, const TwkDenoiserVariance* dv, int minSamples, const float* beauty, const float* albedo,
                              const float* normal, const float* moments, const float* geometry, const float* camera, int width, int height, float* denoised)
try
{
  const char* name = "twk_denoise_geometry_host";
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, (std::string(name) + ": " + text).c_str()); };
  if (!dn || !dg) return refuse(TWK_ERROR_INVALID_VALUE, "NULL parameters");
  DenoiseConstants k;
  const int rc = denoiseParameters(name, dn, dv, dg, minSamples, moments != nullptr, k); if (rc) return rc;
  if (width < 1 || height < 1) return refuse(TWK_ERROR_INVALID_VALUE, "width and height must be >= 1");
  if (!beauty || !albedo || !normal || !geometry || !camera || !denoised || (minSamples != 0 && !moments)) return refuse(TWK_ERROR_INVALID_VALUE, "NULL buffer or camera");
  const size_t n = (size_t) width * height, bytes = n * sizeof(float4);
  if (overlaps(denoised, beauty, bytes) || overlaps(denoised, albedo, bytes) || overlaps(denoised, normal, bytes) || overlaps(denoised, geometry, bytes) || overlaps(denoised, moments, bytes))
    return refuse(TWK_ERROR_INVALID_VALUE, "the denoised buffer overlaps an input");
  DenoiseGeometryConstants g;
  if (!denoiseGeometryConstants(camera, dg->sigmaPosition, dg->instanceStop, g)) return refuse(TWK_ERROR_INVALID_VALUE, "the camera is degenerate: P is not finite, or U, V or W does not normalise");
  if (dn->iterations == 0 || dn->blendFactor == 1.0f) { memcpy(denoised, beauty, bytes); return TWK_SUCCESS; }
  constexpr int KIND = TWK_DENOISER_RGB_ALBEDO_NORMAL;
  k.width = width; k.height = height;
  const float4 *b = reinterpret_cast<const float4*>(beauty), *geo = reinterpret_cast<const float4*>(geometry), *sampled = reinterpret_cast<const float4*>(moments);
  std::vector<float4> streams[2] = {std::vector<float4>(n), std::vector<float4>(n)}, guideNormal(n), guideAlbedo(n);
  float4* colour[2] = {streams[0].data(), streams[1].data()};
  // every pixel of a pass: f(source of the pixel's taps at `step` in stream `in`, p)
  const auto pixels = [&](const float4* in, int step, auto f)
  {
    for (int y = 0; y < height; ++y) for (int x = 0; x < width; ++x)
    {
      const DenoiseGlobalTaps taps(in, guideNormal.data(), guideAlbedo.data(), geo, width, height, x, y, step);
      f(taps, taps.centre);
    }
  };
  for (size_t p = 0; p < n; ++p) denoisePreparePixel(k, p, b, reinterpret_cast<const float4*>(albedo), reinterpret_cast<const float4*>(normal), colour[dv ? 1 : 0], guideNormal.data(), guideAlbedo.data());
  if (dv)
    pixels(colour[1], 1, [&](const DenoiseGlobalTaps& taps, size_t p)
    {
      colour[0][p] = sampled ? denoiseMomentsPixel<KIND, true, true>(k, g, taps, colour[1][p], sampled + p, (float) minSamples)
                             : denoiseMomentsPixel<KIND, false, true>(k, g, taps, colour[1][p], nullptr, 0.0f);
    });
  for (int level = 0; level < dn->iterations; ++level)
  {
    float4* out = colour[(level + 1) & 1];
    pixels(colour[level & 1], 1 << level, [&](const DenoiseGlobalTaps& taps, size_t p) { out[p] = dv ? denoiseLevelPixel<KIND, true, true>(k, g, taps) : denoiseLevelPixel<KIND, false, true>(k, g, taps); });
  }
  for (size_t p = 0; p < n; ++p) denoiseFinishPixel(k, p, b, colour[dn->iterations & 1], guideNormal.data(), guideAlbedo.data(), reinterpret_cast<float4*>(denoised));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_denoise_geometry_host")

// twk_read_denoised and twk_read_denoised_raw: `raw`, the pixels as they are (`size` in bytes); else RGBA32F (`size` in floats)
static int readDenoised(TwkDevice dev, void* host, size_t size, bool raw, const char* where)
{
  int rc = activate(dev, where); if (rc) return rc;
  return readBack(dev, where, {currentPicture(dev, dev->denoised), "no twk_denoise into the internal buffer yet", dev->denoised.count(), raw ? pixelBytes(dev) : 0, true}, host, size,
                  raw ? pixelBytes(dev) : 4, raw ? "width*height pixels of the output format" : "width*height*4 floats of the denoised picture");
}

int twk_read_denoised(TwkDevice dev, float* rgbaHost, size_t numFloats)
try
{
  return readDenoised(dev, rgbaHost, numFloats, false, "twk_read_denoised");
}
TWK_CATCH("twk_read_denoised")

int twk_read_denoised_raw(TwkDevice dev, void* host, size_t bytes)
try
{
  return readDenoised(dev, host, bytes, true, "twk_read_denoised_raw");
}
TWK_CATCH("twk_read_denoised_raw")

int twk_get_denoised_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_denoised_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!(pointer = currentPicture(dev, dev->denoised))) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_denoised_device_pointer: no twk_denoise into the internal buffer yet");
    size = dev->denoised.count() * pixelBytes(dev);
    return (int) TWK_SUCCESS;
  });
}
TWK_CATCH("twk_get_denoised_device_pointer")

// ---- noise estimate (noise_device.h) -----------------------------------------------------------
int twk_noise_defaults(TwkNoise* np)
try
{
  if (!np) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_noise_defaults: NULL argument");
  np->minSamples = TWK_DENOISER_MIN_SAMPLES; np->darkFloor = TWK_NOISE_DARK_FLOOR;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_noise_defaults")

int twk_estimate_noise(TwkDevice dev, const TwkNoise* np, const void* moments, size_t numElements, void* errorMap)
try
{
  const char* name = "twk_estimate_noise";
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, (std::string(name) + ": " + text).c_str()); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  TwkNoise defaults; defaults.minSamples = TWK_DENOISER_MIN_SAMPLES; defaults.darkFloor = TWK_NOISE_DARK_FLOOR;
  if (!np) np = &defaults;
  if (np->minSamples < 2) return refuse(TWK_ERROR_INVALID_VALUE, "minSamples must be >= 2 (one sample has no variance)");
  if (!(np->darkFloor > 0.0f) || !finite1(np->darkFloor)) return refuse(TWK_ERROR_INVALID_VALUE, "darkFloor must be > 0 and finite");
  if (!moments && numElements != 0) return refuse(TWK_ERROR_INVALID_VALUE, "numElements without a moments buffer (pass both, or neither for the handle's own moments)");
  if (moments && (numElements == 0 || numElements > ((size_t) 1 << 31))) return refuse(TWK_ERROR_INVALID_VALUE, "numElements must be in [1, 2^31]");
  int rc = activate(dev, name); if (rc) return rc;
  if (!moments)
  {
    if (!dev->stateSet) return refuse(TWK_ERROR_INVALID_STATE, "twk_set_state first");
    numElements = launchIndices(dev);
    if (!(moments = ownMoments(dev, numElements))) return refuse(TWK_ERROR_INVALID_STATE, "the handle has no luminance moments: twk_enable_moments(1) and twk_set_state first");
  }
  if (overlaps(errorMap, numElements * sizeof(float), moments, numElements * sizeof(float4))) return refuse(TWK_ERROR_INVALID_VALUE, "the error map overlaps the moments");
  if ((rc = dev->d_noise.ensure(1))) return rc;
  NoiseConstants k;
  k.minSamples = (float) np->minSamples; k.darkFloor = np->darkFloor;
  HIP_TRY(hipMemsetAsync(dev->d_noise, 0, sizeof(TwkNoiseSummary), dev->stream));
  launchNoise(static_cast<const float4*>(moments), numElements, static_cast<float*>(errorMap), dev->d_noise, k, dev->numCUs, dev->stream);
  HIP_TRY(hipGetLastError());
  dev->noiseValid = true;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_estimate_noise")

int twk_read_noise(TwkDevice dev, TwkNoiseSummary* out)
try
{
  int rc = activate(dev, "twk_read_noise"); if (rc) return rc;
  if (!out) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_noise: NULL argument");
  if (!dev->d_noise || !dev->noiseValid) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_read_noise: no twk_estimate_noise on this handle yet");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  HIP_TRY(hipMemcpy(out, dev->d_noise, sizeof(TwkNoiseSummary), hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_read_noise")

int twk_noise_merge(TwkNoiseSummary* into, const TwkNoiseSummary* other)
try
{
  if (!into || !other) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_noise_merge: NULL argument");
  noiseMerge(*into, *other);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_noise_merge")

int twk_noise_mean(const TwkNoiseSummary* s, float* mean)
try
{
  if (!s || !mean) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_noise_mean: NULL argument");
  if (s->valid == 0) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_noise_mean: the summary has no valid element");
  *mean = noiseMean(*s);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_noise_mean")

int twk_noise_quantile(const TwkNoiseSummary* s, float q, float* error)
try
{
  if (!s || !error) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_noise_quantile: NULL argument");
  if (!(q > 0.0f && q <= 1.0f)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_noise_quantile: q must be in (0, 1]");
  if (s->valid == 0) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_noise_quantile: the summary has no valid element");
  *error = noiseBinUpperEdge(noiseQuantileBin(*s, q));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_noise_quantile")

} // extern "C"
