// Adaptive sampling behind the C ABI: the switch, the selection of the active list (adaptive_device.h, adaptive_kernels.hip) and
// the readers of the sample counts and the list. The pass that renders the list is device_pass.hip's (twk_launch_adaptive).
#include "device_handle.h"

#include <cmath>

static bool overlapping(const void* a, size_t aBytes, const void* b, size_t bBytes)
{
  const char* x = static_cast<const char*>(a); const char* y = static_cast<const char*>(b);
  return x && y && x < y + bBytes && y < x + aBytes;
}

// The parameter refusals of both selects; fills the constants the predicate takes
static int adaptiveConstants(const char* name, const TwkAdaptive* ap, AdaptiveConstants& k)
{
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!(ap->targetNoise > 0.0f) || !finite1(ap->targetNoise)) return refuse("targetNoise must be > 0 and finite");
  if (ap->minSamples < 2) return refuse("minSamples must be >= 2 (one sample has no variance)");
  if (!(ap->darkFloor > 0.0f) || !finite1(ap->darkFloor)) return refuse("darkFloor must be > 0 and finite");
  if (ap->maxSamples == 0u) return refuse("maxSamples must be >= 1");
  k.noise.minSamples = (float) ap->minSamples; k.noise.darkFloor = ap->darkFloor; k.targetNoise = ap->targetNoise; k.maxSamples = ap->maxSamples;
  return TWK_SUCCESS;
}

static void adaptiveDefaults(TwkAdaptive& a)
{
  a.targetNoise = TWK_ADAPTIVE_TARGET_NOISE; a.minSamples = TWK_DENOISER_MIN_SAMPLES; a.darkFloor = TWK_NOISE_DARK_FLOOR; a.maxSamples = TWK_ADAPTIVE_MAX_SAMPLES;
}

static int ensureAdaptiveScratch(TwkDevice dev, size_t numElements)
{
  if (dev->d_adaptiveScratch && dev->adaptiveScratchElements >= numElements) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  freeDevice(dev->d_adaptiveScratch); dev->adaptiveScratchElements = 0;
  HIP_TRY(hipMalloc(&dev->d_adaptiveScratch, adaptiveScratchBytes(numElements)));
  dev->adaptiveScratchElements = numElements;
  return TWK_SUCCESS;
}

extern "C" {

int twk_adaptive_defaults(TwkAdaptive* ap)
try
{
  if (!ap) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_adaptive_defaults: NULL argument");
  adaptiveDefaults(*ap);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_adaptive_defaults")

int twk_enable_adaptive(TwkDevice dev, int enable)
try
{
  int rc = activate(dev, "twk_enable_adaptive"); if (rc) return rc;
  if (enable && !dev->momentsEnabled) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_enable_adaptive: twk_enable_moments(1) first (the selection reads the samples' luminance moments)");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->adaptiveEnabled = (enable != 0);
  if (!dev->adaptiveEnabled)
  {
    freeDevice(dev->d_sampleCounts); freeDevice(dev->d_active); dev->adaptivePixels = 0;
    freeDevice(dev->d_adaptiveScratch); dev->adaptiveScratchElements = 0;
    dropAdaptive(dev);
    return TWK_SUCCESS;
  }
  if (!dev->stateSet) return TWK_SUCCESS; // allocated by the first use after twk_set_state
  if ((rc = ensureStreams(dev))) return rc;
  return ensureAdaptiveScratch(dev, (size_t) dev->launchWidth * dev->state.resolution[1]);
}
TWK_CATCH("twk_enable_adaptive")

int twk_adaptive_select(TwkDevice dev, const TwkAdaptive* ap, const void* moments, const void* counts, size_t numElements, void* activeOut, unsigned int* numActive)
try
{
  const char* name = "twk_adaptive_select";
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  if (!numActive) return refuse(TWK_ERROR_INVALID_VALUE, "NULL numActive");
  TwkAdaptive defaults; adaptiveDefaults(defaults);
  if (!ap) ap = &defaults;
  AdaptiveConstants k;
  int rc = adaptiveConstants(name, ap, k); if (rc) return rc;
  const bool own = !moments && !counts && !activeOut;
  if (!own && (!moments || !counts || !activeOut)) return refuse(TWK_ERROR_INVALID_VALUE, "moments, counts and activeOut go together: all three, or none for the handle's own buffers");
  if (own && numElements != 0) return refuse(TWK_ERROR_INVALID_VALUE, "numElements without buffers (pass all of them, or none and 0 for the handle's own)");
  if (!own && (numElements == 0 || numElements > ((size_t) 1 << 31))) return refuse(TWK_ERROR_INVALID_VALUE, "numElements must be in [1, 2^31]");
  if (!own)
  {
    const size_t words = numElements * sizeof(unsigned int);
    if (overlapping(activeOut, words, moments, numElements * sizeof(float4)) || overlapping(activeOut, words, counts, words))
      return refuse(TWK_ERROR_INVALID_VALUE, "activeOut overlaps an input");
  }
  if ((rc = activate(dev, name))) return rc;
  if (own)
  {
    if (!dev->stateSet || !dev->momentsEnabled || !dev->adaptiveEnabled) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffers need twk_enable_moments(1), twk_enable_adaptive(1) and twk_set_state");
    if ((rc = ensureStreams(dev))) return rc;
    numElements = (size_t) dev->launchWidth * dev->state.resolution[1];
    if (!dev->d_moments || (size_t) dev->momentsPixels < numElements || !dev->d_sampleCounts || (size_t) dev->adaptivePixels < numElements)
      return refuse(TWK_ERROR_INVALID_STATE, "the handle has no moments or sample counts");
    if ((rc = currentSampleCounts(dev))) return rc;
    moments = dev->d_moments; counts = dev->d_sampleCounts; activeOut = dev->d_active;
    dev->activeValid = false;
  }
  if ((rc = ensureAdaptiveScratch(dev, numElements))) return rc;
  const unsigned int* total = launchAdaptiveSelect(static_cast<const float4*>(moments), static_cast<const unsigned int*>(counts), numElements,
                                                   static_cast<unsigned int*>(activeOut), dev->d_adaptiveScratch, k, dev->numCUs, dev->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(dev->stream));
  unsigned int n = 0;
  HIP_TRY(hipMemcpy(&n, total, sizeof(n), hipMemcpyDeviceToHost));
  *numActive = n;
  if (own) { dev->numActive = n; dev->activeValid = true; }
  return checkDroppedPushes(dev, name);
}
TWK_CATCH("twk_adaptive_select")

int twk_adaptive_select_host(const TwkAdaptive* ap, const float* moments, const uint32_t* counts, size_t numElements, uint32_t* activeOut, size_t* numActive)
try
{
  const char* name = "twk_adaptive_select_host";
  if (!moments || !counts || !activeOut || !numActive) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  TwkAdaptive defaults; adaptiveDefaults(defaults);
  if (!ap) ap = &defaults;
  AdaptiveConstants k;
  int rc = adaptiveConstants(name, ap, k); if (rc) return rc;
  if (numElements > ((size_t) 1 << 31)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": numElements must be at most 2^31");
  size_t n = 0;
  for (size_t i = 0; i < numElements; ++i)
  {
    const float4 m = make_float4(moments[4 * i], moments[4 * i + 1], moments[4 * i + 2], moments[4 * i + 3]);
    if (adaptiveSelected(k, m, counts[i])) activeOut[n++] = (uint32_t) i;
  }
  *numActive = n;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_adaptive_select_host")

int twk_read_sample_counts(TwkDevice dev, uint32_t* host, size_t numElements)
try
{
  int rc = activate(dev, "twk_read_sample_counts"); if (rc) return rc;
  if (!host) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_sample_counts: NULL buffer");
  if (!dev->adaptiveEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_read_sample_counts: twk_enable_adaptive(1) and twk_set_state first");
  const size_t n = (size_t) dev->launchWidth * dev->state.resolution[1];
  if (numElements != n) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_sample_counts: buffer must hold launchWidth*height words");
  if ((rc = ensureStreams(dev))) return rc;
  if ((rc = currentSampleCounts(dev))) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  HIP_TRY(hipMemcpy(host, dev->d_sampleCounts, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_read_sample_counts")

int twk_get_sample_counts_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  int rc = activate(dev, "twk_get_sample_counts_device_pointer"); if (rc) return rc;
  if (!dptr) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_sample_counts_device_pointer: NULL argument");
  if (!dev->adaptiveEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_sample_counts_device_pointer: twk_enable_adaptive(1) and twk_set_state first");
  if ((rc = ensureStreams(dev))) return rc;
  if ((rc = currentSampleCounts(dev))) return rc;
  *dptr = dev->d_sampleCounts;
  if (bytes) *bytes = (size_t) dev->launchWidth * dev->state.resolution[1] * sizeof(uint32_t);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_sample_counts_device_pointer")

int twk_read_active(TwkDevice dev, uint32_t* host, size_t capacity, unsigned int* numActive)
try
{
  int rc = activate(dev, "twk_read_active"); if (rc) return rc;
  if (!numActive || (!host && capacity != 0)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_active: NULL argument");
  if (!dev->activeValid || !dev->d_active) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_read_active: no active list: twk_adaptive_select on the handle's own buffers first");
  *numActive = dev->numActive;
  if (!host) return TWK_SUCCESS; // the length alone
  if (capacity < dev->numActive) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_active: the list has " + std::to_string(dev->numActive) + " entries, the buffer holds fewer");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if (dev->numActive) HIP_TRY(hipMemcpy(host, dev->d_active, (size_t) dev->numActive * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_read_active")

} // extern "C"
