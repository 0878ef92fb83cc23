// Adaptive sampling behind the C ABI: the switch, the selection of the active list (adaptive_device.h, adaptive_kernels.hip), the plan
// of a planned pass (adaptive_plan_device.h, adaptive_plan_kernels.hip) and the readers of the sample counts, the list and the plan.
// The passes that render them are device_pass.hip's (twk_launch_adaptive, twk_launch_adaptive_planned).
#include "device_handle.h"

#include <algorithm>
#include <climits>
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

// The scan scratch, for a select of numElements elements (also the explicit form's). Its capacity counts elements.
static int ensureAdaptiveScratch(TwkDevice dev, size_t numElements)
{
  if (!dev->d_adaptiveScratch.holds(numElements)) dev->adaptiveScratchPlan = false;
  return growIdle(dev, dev->d_adaptiveScratch, numElements, adaptiveScratchBytes(numElements));
}

// ... for a plan: the same buffer at the plan's larger size, which holds a select of as many elements too
static int ensureAdaptivePlanScratch(TwkDevice dev, size_t numElements)
{
  if (dev->adaptiveScratchPlan && dev->d_adaptiveScratch.holds(numElements)) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  const size_t elements = std::max(numElements, dev->d_adaptiveScratch.capacity());
  dev->adaptiveScratchPlan = false;
  const int rc = dev->d_adaptiveScratch.allocate(elements, false, nullptr, std::max(adaptivePlanScratchBytes(elements), adaptiveScratchBytes(elements))); if (rc) return rc;
  dev->adaptiveScratchPlan = true;
  return TWK_SUCCESS;
}

// The plan's own list and offsets of the own-buffer form: numElements and numElements + 1 words
static int ensurePlanBuffers(TwkDevice dev, size_t numElements)
{
  if (dev->d_planActive.holds(numElements) && dev->d_planOffsets.holds(numElements + 1)) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->d_planActive.release(); dev->d_planOffsets.release(); dev->planValid = false;
  const int rc = dev->d_planActive.allocate(numElements);
  return rc ? rc : dev->d_planOffsets.allocate(numElements + 1);
}

static void adaptivePlanDefaults(TwkAdaptivePlan& p) { p.minBatch = TWK_DENOISER_MIN_SAMPLES; p.maxBatch = TWK_ADAPTIVE_PLAN_MAX_BATCH; }

// The plan's own constraint, refused by both plans
static int adaptivePlanConstants(const char* name, const TwkAdaptivePlan* pp, AdaptivePlanConstants& plan)
{
  if (pp->minBatch < 1u || pp->minBatch > pp->maxBatch || pp->maxBatch > TWK_ADAPTIVE_PLAN_MAX_BATCH)
    return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": 1 <= minBatch <= maxBatch <= 64 (got " + std::to_string(pp->minBatch) + ", " + std::to_string(pp->maxBatch) + ")");
  plan.minBatch = pp->minBatch; plan.maxBatch = pp->maxBatch;
  return TWK_SUCCESS;
}

static int tooManyPaths(const char* name, unsigned long long numActive, unsigned long long numPaths)
{
  return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": the plan of " + std::to_string(numActive) + " entries has " + std::to_string(numPaths) +
                     " paths, a wavefront pass holds at most " + std::to_string(INT_MAX) + " (lower maxBatch, or plan a part of the elements)");
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
    dev->d_sampleCounts.release(); dev->d_active.release();
    dev->d_adaptiveScratch.release(); dev->adaptiveScratchPlan = false;
    dev->d_planActive.release(); dev->d_planOffsets.release();
    dropAdaptive(dev);
    return TWK_SUCCESS;
  }
  if (!dev->stateSet) return TWK_SUCCESS; // allocated by the first use after twk_set_state
  if ((rc = ensureStreams(dev))) return rc;
  return ensureAdaptiveScratch(dev, launchIndices(dev));
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
    numElements = launchIndices(dev);
    if (!(moments = ownMoments(dev, numElements)) || !(counts = ownSampleCounts(dev, numElements))) return refuse(TWK_ERROR_INVALID_STATE, "the handle has no moments or sample counts");
    if ((rc = currentSampleCounts(dev))) return rc;
    activeOut = dev->d_active;
    dev->activeValid = false; dev->planValid = false; // a select supersedes the plan: the loop goes on with one or the other
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

int twk_adaptive_plan_defaults(TwkAdaptivePlan* plan)
try
{
  if (!plan) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_adaptive_plan_defaults: NULL argument");
  adaptivePlanDefaults(*plan);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_adaptive_plan_defaults")

int twk_adaptive_plan(TwkDevice dev, const TwkAdaptive* ap, const TwkAdaptivePlan* plan, const void* moments, const void* counts, size_t numElements,
                      void* activeOut, void* pathOffsetOut, unsigned int* numActive, unsigned long long* numPaths)
try
{
  const char* name = "twk_adaptive_plan";
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  if (!numActive || !numPaths) return refuse(TWK_ERROR_INVALID_VALUE, "NULL numActive or numPaths");
  TwkAdaptive defaults; adaptiveDefaults(defaults);
  if (!ap) ap = &defaults;
  TwkAdaptivePlan planDefaults; adaptivePlanDefaults(planDefaults);
  if (!plan) plan = &planDefaults;
  AdaptiveConstants k;
  AdaptivePlanConstants pk;
  int rc = adaptiveConstants(name, ap, k); if (rc) return rc;
  if ((rc = adaptivePlanConstants(name, plan, pk))) return rc;
  const bool own = !moments && !counts && !activeOut && !pathOffsetOut;
  if (!own && (!moments || !counts || !activeOut || !pathOffsetOut)) return refuse(TWK_ERROR_INVALID_VALUE, "moments, counts, activeOut and pathOffsetOut go together: all four, or none for the handle's own buffers");
  if (own && numElements != 0) return refuse(TWK_ERROR_INVALID_VALUE, "numElements without buffers (pass all of them, or none and 0 for the handle's own)");
  if (!own && (numElements == 0 || numElements > ((size_t) 1 << 31))) return refuse(TWK_ERROR_INVALID_VALUE, "numElements must be in [1, 2^31]");
  if (!own)
  {
    const size_t words = numElements * sizeof(unsigned int), offsetWords = words + sizeof(unsigned int), momentBytes = numElements * sizeof(float4);
    if (overlapping(activeOut, words, moments, momentBytes) || overlapping(activeOut, words, counts, words))
      return refuse(TWK_ERROR_INVALID_VALUE, "activeOut overlaps an input");
    if (overlapping(pathOffsetOut, offsetWords, moments, momentBytes) || overlapping(pathOffsetOut, offsetWords, counts, words))
      return refuse(TWK_ERROR_INVALID_VALUE, "pathOffsetOut overlaps an input");
    if (overlapping(activeOut, words, pathOffsetOut, offsetWords)) return refuse(TWK_ERROR_INVALID_VALUE, "activeOut overlaps pathOffsetOut");
  }
  if ((rc = activate(dev, name))) return rc;
  if (own)
  {
    if (!dev->stateSet || !dev->momentsEnabled || !dev->adaptiveEnabled) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffers need twk_enable_moments(1), twk_enable_adaptive(1) and twk_set_state");
    if ((rc = ensureStreams(dev))) return rc;
    numElements = launchIndices(dev);
    if (!(moments = ownMoments(dev, numElements)) || !(counts = ownSampleCounts(dev, numElements))) return refuse(TWK_ERROR_INVALID_STATE, "the handle has no moments or sample counts");
    if ((rc = currentSampleCounts(dev))) return rc;
    if ((rc = ensurePlanBuffers(dev, numElements))) return rc;
    activeOut = dev->d_planActive; pathOffsetOut = dev->d_planOffsets;
    dev->planValid = false;
  }
  if ((rc = ensureAdaptivePlanScratch(dev, numElements))) return rc;
  const unsigned long long* totals = launchAdaptivePlan(static_cast<const float4*>(moments), static_cast<const unsigned int*>(counts), numElements,
                                                        static_cast<unsigned int*>(activeOut), static_cast<unsigned int*>(pathOffsetOut), dev->d_adaptiveScratch, k, pk, dev->numCUs, dev->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(dev->stream));
  unsigned long long both[2] = {0ull, 0ull};
  HIP_TRY(hipMemcpy(both, totals, sizeof(both), hipMemcpyDeviceToHost));
  *numActive = (unsigned int) both[1]; *numPaths = both[0];
  if (both[0] > (unsigned long long) INT_MAX) return tooManyPaths(name, both[1], both[0]);
  if (own) { dev->planActive = (unsigned int) both[1]; dev->planPaths = (unsigned int) both[0]; dev->planValid = true; }
  return checkDroppedPushes(dev, name);
}
TWK_CATCH("twk_adaptive_plan")

int twk_adaptive_plan_host(const TwkAdaptive* ap, const TwkAdaptivePlan* plan, const float* moments, const uint32_t* counts, size_t numElements,
                           uint32_t* activeOut, uint32_t* pathOffsetOut, size_t* numActive, unsigned long long* numPaths)
try
{
  const char* name = "twk_adaptive_plan_host";
  if (!moments || !counts || !activeOut || !pathOffsetOut || !numActive || !numPaths) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  TwkAdaptive defaults; adaptiveDefaults(defaults);
  if (!ap) ap = &defaults;
  TwkAdaptivePlan planDefaults; adaptivePlanDefaults(planDefaults);
  if (!plan) plan = &planDefaults;
  AdaptiveConstants k;
  AdaptivePlanConstants pk;
  int rc = adaptiveConstants(name, ap, k); if (rc) return rc;
  if ((rc = adaptivePlanConstants(name, plan, pk))) return rc;
  if (numElements > ((size_t) 1 << 31)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": numElements must be at most 2^31");
  size_t n = 0;
  unsigned long long paths = 0ull;
  for (size_t i = 0; i < numElements; ++i)
  {
    const float4 m = make_float4(moments[4 * i], moments[4 * i + 1], moments[4 * i + 2], moments[4 * i + 3]);
    const unsigned int b = adaptiveBudget(k, pk, m, counts[i]);
    if (b == 0u) continue;
    activeOut[n] = (uint32_t) i; pathOffsetOut[n] = (uint32_t) paths;
    ++n; paths += b;
  }
  pathOffsetOut[n] = (uint32_t) paths;
  *numActive = n; *numPaths = paths;
  if (paths > (unsigned long long) INT_MAX) return tooManyPaths(name, n, paths);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_adaptive_plan_host")

int twk_read_plan(TwkDevice dev, uint32_t* active, uint32_t* pathOffset, size_t capacity, unsigned int* numActive, unsigned long long* numPaths)
try
{
  int rc = activate(dev, "twk_read_plan"); if (rc) return rc;
  if (!numActive || !numPaths || (!active != !pathOffset) || (!active && capacity != 0)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_plan: NULL argument (both buffers, or neither and capacity 0 for the lengths alone)");
  if (!dev->planValid || !dev->d_planActive || !dev->d_planOffsets) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_read_plan: no plan: twk_adaptive_plan on the handle's own buffers first (a rendered plan is gone)");
  *numActive = dev->planActive; *numPaths = dev->planPaths;
  if (!active) return TWK_SUCCESS; // the lengths alone
  if (capacity < dev->planActive) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_plan: the plan has " + std::to_string(dev->planActive) + " entries, the buffers hold fewer (active: capacity words, pathOffset: capacity + 1)");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if (dev->planActive) HIP_TRY(hipMemcpy(active, dev->d_planActive, (size_t) dev->planActive * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pathOffset, dev->d_planOffsets, ((size_t) dev->planActive + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_read_plan")

int twk_read_sample_counts(TwkDevice dev, uint32_t* host, size_t numElements)
try
{
  int rc = activate(dev, "twk_read_sample_counts"); if (rc) return rc;
  if (!host) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_sample_counts: NULL buffer");
  if (!dev->adaptiveEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_read_sample_counts: twk_enable_adaptive(1) and twk_set_state first");
  const size_t n = launchIndices(dev);
  if (numElements != n) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_sample_counts: buffer must hold launchWidth*height words");
  if ((rc = ensureStreams(dev))) return rc; // (allocated and made current only now that the call is known to read them)
  if ((rc = currentSampleCounts(dev))) return rc;
  return copyBack(dev, "twk_read_sample_counts", dev->d_sampleCounts, n, sizeof(uint32_t), host);
}
TWK_CATCH("twk_read_sample_counts")

int twk_get_sample_counts_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_sample_counts_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!dev->adaptiveEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_sample_counts_device_pointer: twk_enable_adaptive(1) and twk_set_state first");
    int rc = ensureStreams(dev); if (rc) return rc;
    rc = currentSampleCounts(dev);
    pointer = dev->d_sampleCounts; size = launchIndices(dev) * sizeof(uint32_t);
    return rc;
  });
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
