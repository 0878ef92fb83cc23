// The cascade's layers through the temporal merge behind the C ABI (temporal_cascade_device.h: the definition): the explicit form,
// the switch of the own-buffer form with its double-buffered merged layers and their readers, and the host-only form. The own-buffer
// merge itself is issued by twk_temporal_accumulate (device_temporal.hip) through temporalCascadeOwn(), before it swaps its history.
// The checks of TwkTemporal and the history's camera are device_temporal.hip's temporalParameters and temporalHistoryCamera.
#include "device_handle.h"
#include "temporal_motion_host.h"

#include <cstring>
#include <vector>

// Frees the merged layers of the own-buffer form: the next call has no history of layers. The switch stays as it is.
void twk::dropTemporalCascade(TwkDevice dev)
{
  for (int s = 0; s < 2; ++s) dev->d_temporalCascade[s].release();
  dev->temporalCascadeLayers = 0; dev->temporalCascadeKept = 0;
  dev->temporalCascadeHasHistory = false; dev->temporalCascadeValid = false;
}

// Why the own-buffer twk_temporal_accumulate cannot merge the handle's layers (the switch is on); nullptr: it can
const char* twk::temporalCascadeRefusal(TwkDevice dev)
{
  if (!dev->cascadeEnabled) return "twk_temporal_enable_cascade(1) is set but the handle has no cascade layers: twk_enable_cascade(1) first";
  return nullptr;
}

// The own-buffer form's merge of the frame's layers, on its stream: k, geometry and historyGeometry (nullptr: the temporal merge
// has no history) are those of the twk_temporal_accumulate or twk_temporal_accumulate_assembled that calls it, before it swaps its
// history. layers: [layers][k.width x k.height] float4, the assembled ones of a tiled primary; nullptr: the handle's own.
// trust: nullptr = the plain merge; else the trust plane of the rectified merge of the same frame, already written on the stream.
// motion, numMotion: the table that merge uses (a device pointer; nullptr or 0: none).
int twk::temporalCascadeOwn(TwkDevice dev, const TemporalConstants& k, const float4* layers, const float4* geometry, const float4* historyGeometry, const float* trust,
                            const TwkInstanceMotion* motion, unsigned int numMotion, const float4* carried)
{
  int rc = ensureStreams(dev); if (rc) return rc;
  const size_t n = (size_t) k.width * k.height;
  const int K = dev->cascadeK.layers;
  if (!layers)
  {
    if (dev->d_cascade.capacity() != n * (size_t) K) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_temporal_accumulate: the handle's cascade layers do not have the frame's shape");
    layers = dev->d_cascade;
  }
  if (dev->d_temporalCascade[0].capacity() != n * (size_t) K || dev->temporalCascadeLayers != K) // (exactly the frame's pixels of exactly K layers)
  {
    HIP_TRY(hipStreamSynchronize(dev->stream));
    dropTemporalCascade(dev);
    for (int s = 0; s < 2; ++s) if ((rc = dev->d_temporalCascade[s].allocate(n * (size_t) K))) return rc;
    dev->temporalCascadeLayers = K;
  }
  // layers are reprojected only with a history of their own and of the geometry: the first call after a drop copies the frame's through
  const bool history = dev->temporalCascadeHasHistory && k.hasHistory != 0 && historyGeometry != nullptr;
  const int keep = dev->temporalCascadeHasHistory ? 1 - dev->temporalCascadeKept : dev->temporalCascadeKept;
  TemporalConstants kc = k;
  kc.hasHistory = history ? 1 : 0;
  if (trust)
    launchTemporalCascadeTrusted(layers, geometry, history ? dev->d_temporalCascade[dev->temporalCascadeKept] : nullptr, history ? historyGeometry : nullptr, trust,
                                 dev->d_temporalCascade[keep], kc, dev->cascadeK, dev->stream, motion, numMotion, history ? carried : nullptr);
  else
    launchTemporalCascade(layers, geometry, history ? dev->d_temporalCascade[dev->temporalCascadeKept] : nullptr, history ? historyGeometry : nullptr,
                          dev->d_temporalCascade[keep], kc, dev->cascadeK, dev->stream, motion, numMotion, history ? carried : nullptr);
  HIP_TRY(hipGetLastError());
  dev->temporalCascadeKept = keep; dev->temporalCascadeHasHistory = true; dev->temporalCascadeValid = true;
  return TWK_SUCCESS;
}

// The refusals the explicit and the host-only form share, and the constants both take. history: a history was passed.
static int temporalCascadeParameters(const char* name, const TwkTemporal* tp, const TwkCascade* cp, bool history, const TwkCameraDefinition* historyCamera, int width, int height,
                                     TemporalConstants& k, CascadeConstants& c)
{
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  TwkCascade cascade; cascade.layers = TWK_CASCADE_LAYERS; cascade.start = TWK_CASCADE_START; cascade.base = TWK_CASCADE_BASE;
  if (cp) cascade = *cp;
  if (const char* why = cascadeConstants(cascade, c)) return refuse(why);
  const int rc = temporalParameters(name, tp, k); if (rc) return rc;
  if (width < 1 || height < 1) return refuse("width and height must be >= 1");
  if ((size_t) width * (size_t) height > ((size_t) 1 << 28)) return refuse("width*height must be at most 2^28");
  k.width = width; k.height = height;
  return history ? temporalHistoryCamera(name, *historyCamera, k) : TWK_SUCCESS;
}

// The explicit form, plain (trusted false) and trusted (trust: width x height floats). moving: twk_temporal_accumulate_cascade_moving,
// whose table (motion, numMotion; nullptr or 0: none) is checked here; the others pass none.
static int temporalCascadeExplicit(const char* name, bool trusted, TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                   const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, const void* trust, int width, int height,
                                   void* layersOut, const TwkInstanceMotion* motion = nullptr, int numMotion = 0, const void* previousPositions = nullptr)
{
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  if (!currentLayers || !currentGeometry || !layersOut) return refuse(TWK_ERROR_INVALID_VALUE, "NULL current layers, current geometry or output");
  if (historyLayers && (!historyGeometry || !historyCamera)) return refuse(TWK_ERROR_INVALID_VALUE, "history layers without the history's geometry or camera");
  if (trusted && !trust) return refuse(TWK_ERROR_INVALID_VALUE, "NULL trust");
  TemporalConstants k;
  CascadeConstants c;
  int rc = temporalCascadeParameters(name, tp, cp, historyLayers != nullptr, historyCamera, width, height, k, c); if (rc) return rc;
  const size_t n = (size_t) width * height, plane = n * sizeof(float4), layerBytes = plane * (size_t) c.layers;
  if (overlaps(layersOut, layerBytes, currentLayers, layerBytes) || overlaps(layersOut, layerBytes, currentGeometry, plane) ||
      (historyLayers && (overlaps(layersOut, layerBytes, historyLayers, layerBytes) || overlaps(layersOut, layerBytes, historyGeometry, plane))))
    return refuse(TWK_ERROR_INVALID_VALUE, "the output overlaps an input (the kernel gathers the history at other pixels)");
  if (trusted && overlaps(layersOut, layerBytes, trust, n * sizeof(float))) return refuse(TWK_ERROR_INVALID_VALUE, "the output overlaps the trust");
  if (numMotion < 0) return refuse(TWK_ERROR_INVALID_VALUE, "numMotion must be >= 0");
  if (!motion || !historyLayers) numMotion = 0; // (without a history nothing is reprojected)
  if (numMotion > 0 && ((uintptr_t) motion & 15u) != 0) return refuse(TWK_ERROR_INVALID_VALUE, "the motion table is not 16-byte aligned");
  if (numMotion > 0 && overlaps(layersOut, layerBytes, motion, (size_t) numMotion * sizeof(TwkInstanceMotion))) return refuse(TWK_ERROR_INVALID_VALUE, "the output overlaps the motion table");
  // the previous-position plane of a Carried build (twk_temporal_accumulate_cascade_carried); without a history nothing is reprojected
  const float4* carried = historyLayers ? static_cast<const float4*>(previousPositions) : nullptr;
  if (carried && ((uintptr_t) carried & 15u) != 0) return refuse(TWK_ERROR_INVALID_VALUE, "the previous positions are not 16-byte aligned");
  if (carried && overlaps(layersOut, layerBytes, carried, plane)) return refuse(TWK_ERROR_INVALID_VALUE, "the output overlaps the previous positions");
  if ((rc = activate(dev, name))) return rc;
  if (trusted)
    launchTemporalCascadeTrusted(static_cast<const float4*>(currentLayers), static_cast<const float4*>(currentGeometry), static_cast<const float4*>(historyLayers),
                                 historyLayers ? static_cast<const float4*>(historyGeometry) : nullptr, static_cast<const float*>(trust), static_cast<float4*>(layersOut), k, c, dev->stream,
                                 motion, (unsigned int) numMotion, carried);
  else
    launchTemporalCascade(static_cast<const float4*>(currentLayers), static_cast<const float4*>(currentGeometry), static_cast<const float4*>(historyLayers),
                          historyLayers ? static_cast<const float4*>(historyGeometry) : nullptr, static_cast<float4*>(layersOut), k, c, dev->stream, motion, (unsigned int) numMotion, carried);
  HIP_TRY(hipGetLastError());
  return TWK_SUCCESS;
}

// The host-only form, plain and trusted, with a table (twk_temporal_cascade_moving_host; a host array) or without
static int temporalCascadeHost(const char* name, bool trusted, const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry,
                               const float* historyLayers, const float* historyGeometry, const TwkCameraDefinition* historyCamera, const float* trust, int width, int height,
                               float* layersOut, const TwkInstanceMotion* motion = nullptr, int numMotion = 0, const float* previousPositions = nullptr)
{
  if (!currentLayers || !currentGeometry || !layersOut) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL current layers, current geometry or output");
  if (historyLayers && (!historyGeometry || !historyCamera)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": history layers without the history's geometry or camera");
  if (trusted && !trust) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL trust");
  if (numMotion < 0) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": numMotion must be >= 0");
  TemporalConstants k;
  CascadeConstants c;
  int rc = temporalCascadeParameters(name, tp, cp, historyLayers != nullptr, historyCamera, width, height, k, c); if (rc) return rc;
  temporalCascadeHostLayers(k, c, currentLayers, currentGeometry, historyLayers, historyGeometry, trusted ? trust : nullptr, motion, motion ? (unsigned int) numMotion : 0u, layersOut,
                            historyLayers ? previousPositions : nullptr);
  return TWK_SUCCESS;
}

extern "C" {

int twk_temporal_accumulate_cascade(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                    const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, int width, int height, void* layersOut)
try
{
  return temporalCascadeExplicit("twk_temporal_accumulate_cascade", false, dev, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, nullptr, width, height, layersOut);
}
TWK_CATCH("twk_temporal_accumulate_cascade")

int twk_temporal_accumulate_cascade_trusted(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                            const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, const void* trust,
                                            int width, int height, void* layersOut)
try
{
  return temporalCascadeExplicit("twk_temporal_accumulate_cascade_trusted", true, dev, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, trust, width, height, layersOut);
}
TWK_CATCH("twk_temporal_accumulate_cascade_trusted")

int twk_temporal_accumulate_cascade_moving(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                           const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, const void* trust,
                                           const TwkInstanceMotion* motion, int numMotion, int width, int height, void* layersOut)
try
{
  return temporalCascadeExplicit("twk_temporal_accumulate_cascade_moving", trust != nullptr, dev, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, trust,
                                 width, height, layersOut, motion, numMotion);
}
TWK_CATCH("twk_temporal_accumulate_cascade_moving")

int twk_temporal_accumulate_cascade_carried(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                            const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, const void* trust,
                                            const void* previousPositions, int width, int height, void* layersOut)
try
{
  return temporalCascadeExplicit("twk_temporal_accumulate_cascade_carried", trust != nullptr, dev, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, trust,
                                 width, height, layersOut, nullptr, 0, previousPositions);
}
TWK_CATCH("twk_temporal_accumulate_cascade_carried")

int twk_temporal_enable_cascade(TwkDevice dev, int enable)
try
{
  const char* name = "twk_temporal_enable_cascade";
  int rc = activate(dev, name); if (rc) return rc;
  if (enable && !dev->cascadeEnabled) return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": the handle has no cascade layers: twk_enable_cascade(1) first");
  if (!enable && dev->temporalCascade)
  {
    HIP_TRY(hipStreamSynchronize(dev->stream));
    dropTemporalCascade(dev);
  }
  dev->temporalCascade = (enable != 0);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_enable_cascade")

// The merged layers the last own-buffer merge kept, if there was one since the last drop
static float4* keptLayers(TwkDevice dev) { return dev->temporalCascadeValid ? dev->d_temporalCascade[dev->temporalCascadeKept].get() : nullptr; }
static const char* const noLayers = "no twk_temporal_accumulate with twk_temporal_enable_cascade(1) on the handle's own buffers since the last drop";

int twk_get_temporal_cascade_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_temporal_cascade_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!dev->temporalCascadeValid) return twkSetError(TWK_ERROR_INVALID_STATE, std::string("twk_get_temporal_cascade_device_pointer: ") + noLayers);
    pointer = keptLayers(dev); size = dev->d_temporalCascade[dev->temporalCascadeKept].capacity() * sizeof(float4);
    return (int) TWK_SUCCESS;
  });
}
TWK_CATCH("twk_get_temporal_cascade_device_pointer")

int twk_read_temporal_cascade(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_temporal_cascade"); if (rc) return rc;
  return readBack(dev, "twk_read_temporal_cascade", {keptLayers(dev), noLayers, dev->d_temporalCascade[dev->temporalCascadeKept].capacity(), sizeof(float4), true}, host, numFloats, 4,
                  "layers*launchWidth*height*4 floats");
}
TWK_CATCH("twk_read_temporal_cascade")

int twk_temporal_cascade_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                              const float* historyGeometry, const TwkCameraDefinition* historyCamera, int width, int height, float* layersOut)
try
{
  return temporalCascadeHost("twk_temporal_cascade_host", false, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, nullptr, width, height, layersOut);
}
TWK_CATCH("twk_temporal_cascade_host")

int twk_temporal_cascade_trusted_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                                      const float* historyGeometry, const TwkCameraDefinition* historyCamera, const float* trust, int width, int height, float* layersOut)
try
{
  return temporalCascadeHost("twk_temporal_cascade_trusted_host", true, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, trust, width, height, layersOut);
}
TWK_CATCH("twk_temporal_cascade_trusted_host")

int twk_temporal_cascade_moving_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                                     const float* historyGeometry, const TwkCameraDefinition* historyCamera, const float* trust, const TwkInstanceMotion* motion, int numMotion,
                                     int width, int height, float* layersOut)
try
{
  return temporalCascadeHost("twk_temporal_cascade_moving_host", trust != nullptr, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, trust, width, height,
                             layersOut, motion, numMotion);
}
TWK_CATCH("twk_temporal_cascade_moving_host")

int twk_temporal_cascade_carried_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                                      const float* historyGeometry, const TwkCameraDefinition* historyCamera, const float* trust, const float* previousPositions,
                                      int width, int height, float* layersOut)
try
{
  return temporalCascadeHost("twk_temporal_cascade_carried_host", trust != nullptr, tp, cp, currentLayers, currentGeometry, historyLayers, historyGeometry, historyCamera, trust, width, height,
                             layersOut, nullptr, 0, previousPositions);
}
TWK_CATCH("twk_temporal_cascade_carried_host")

} // extern "C"
