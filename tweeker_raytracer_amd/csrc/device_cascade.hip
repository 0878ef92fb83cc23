// The firefly cascade behind the C ABI (cascade_device.h: the definition): the switch and its layers, their readers, the resolve
// (cascade_kernels.hip) with its internal resolved picture, and the host-only forms of the fold and the resolve. The fold itself runs
// in the CASCADE builds of the accumulate kernels (shade_kernels.hip), which device_pass.hip launches with cascadeFold().
#include "device_handle.h"

#include <cstring>
#include <vector>

static void cascadeDefaults(TwkCascade& c) { c.layers = TWK_CASCADE_LAYERS; c.start = TWK_CASCADE_START; c.base = TWK_CASCADE_BASE; }

// The parameter refusals of every call that takes a TwkCascade (NULL: `fallback`); fills the table the kernels take
static int cascadeParameters(const char* name, const TwkCascade* cp, const TwkCascade& fallback, TwkCascade& c, CascadeConstants& k)
{
  c = cp ? *cp : fallback;
  if (const char* why = cascadeConstants(c, k)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + why);
  return TWK_SUCCESS;
}

static int resolveParameters(const char* name, const TwkCascadeResolve* rp, float& kappa)
{
  kappa = rp ? rp->kappa : TWK_CASCADE_KAPPA;
  if (!(kappa > 0.0f) || !cascadeFinite(kappa)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": kappa must be > 0 and finite");
  return TWK_SUCCESS;
}

static bool sameParameters(const TwkCascade& a, const TwkCascade& b) { return a.layers == b.layers && asUint(a.start) == asUint(b.start) && asUint(a.base) == asUint(b.base); }

// The floats4 of the handle's layers: every layer exactly the launch indices
static size_t cascadeElements(TwkDevice dev) { return launchIndices(dev) * (size_t) dev->cascadeK.layers; }

// What an accumulate launch folds into: the handle's layers and table, or layers == nullptr with the cascade off
CascadeOn twk::cascadeFold(TwkDevice dev)
{
  CascadeOn c;
  c.layers = (dev->cascadeEnabled && dev->d_cascade.capacity() == cascadeElements(dev)) ? dev->d_cascade.get() : nullptr;
  c.k = dev->cascadeK;
  return c;
}

extern "C" {

int twk_cascade_defaults(TwkCascade* cp)
try
{
  if (!cp) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_cascade_defaults: NULL argument");
  cascadeDefaults(*cp);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_cascade_defaults")

int twk_cascade_resolve_defaults(TwkCascadeResolve* rp)
try
{
  if (!rp) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_cascade_resolve_defaults: NULL argument");
  rp->kappa = TWK_CASCADE_KAPPA;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_cascade_resolve_defaults")

int twk_enable_cascade(TwkDevice dev, int enable, const TwkCascade* cp)
try
{
  const char* name = "twk_enable_cascade";
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL device handle");
  TwkCascade defaults, c; cascadeDefaults(defaults);
  CascadeConstants k;
  int rc;
  if (enable && (rc = cascadeParameters(name, cp, defaults, c, k))) return rc;
  if ((rc = activate(dev, name))) return rc; // recorded launches are rendered with the switch they were recorded under
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->resolved.valid = false;
  if (!enable || !dev->cascadeEnabled || !sameParameters(c, dev->cascadeParameters)) { dropAssembled(dev); dropTemporalCascade(dev); } // assembled and temporally merged layers are of the old parameters
  if (!enable)
  {
    dev->cascadeEnabled = false;
    dev->d_cascade.release(); dev->d_cascadeLambda.release(); dev->resolved.release();
    return TWK_SUCCESS;
  }
  if (dev->cascadeEnabled && sameParameters(c, dev->cascadeParameters)) return dev->stateSet ? ensureStreams(dev) : TWK_SUCCESS;
  // switched on, or new parameters: zeroed layers (a buffer of its own size when the number of layers changed)
  dev->d_cascade.release();
  dev->cascadeEnabled = true; dev->cascadeParameters = c; dev->cascadeK = k;
  return dev->stateSet ? ensureStreams(dev) : TWK_SUCCESS; // allocated, zeroed, here or by the first pass after twk_set_state
}
TWK_CATCH("twk_enable_cascade")

int twk_read_cascade(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_cascade"); if (rc) return rc;
  if (!host) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_cascade: NULL buffer");
  if (!dev->cascadeEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_read_cascade: twk_enable_cascade(1) and twk_set_state first");
  const size_t n = cascadeElements(dev);
  if (numFloats != n * 4) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_read_cascade: buffer must hold layers*launchWidth*height*4 floats");
  if ((rc = ensureStreams(dev))) return rc; // (the layers of a handle that has not rendered yet: allocated, zeroed, only now that the call is known to read them)
  return copyBack(dev, "twk_read_cascade", dev->d_cascade, n, sizeof(float4), host, true);
}
TWK_CATCH("twk_read_cascade")

int twk_get_cascade_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_cascade_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!dev->cascadeEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_cascade_device_pointer: twk_enable_cascade(1) and twk_set_state first");
    const int rc = ensureStreams(dev); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(dev->stream));
    pointer = dev->d_cascade; size = cascadeElements(dev) * sizeof(float4);
    return (int) TWK_SUCCESS;
  });
}
TWK_CATCH("twk_get_cascade_device_pointer")

int twk_cascade_resolve(TwkDevice dev, const TwkCascade* cp, const TwkCascadeResolve* rp, const void* layers, int width, int height, void* resolved)
try
{
  const char* name = "twk_cascade_resolve";
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  TwkCascade defaults, c; cascadeDefaults(defaults);
  const bool own = !layers;
  CascadeConstants k;
  float kappa;
  int rc;
  if ((rc = cascadeParameters(name, cp, own ? dev->cascadeParameters : defaults, c, k))) return rc;
  if ((rc = resolveParameters(name, rp, kappa))) return rc;
  if (own && (width != 0 || height != 0 || resolved)) return refuse(TWK_ERROR_INVALID_VALUE, "a size or a resolved buffer without layers (pass all of them, or none and 0 for the handle's own)");
  if (!own)
  {
    if (width < 1 || height < 1 || !resolved) return refuse(TWK_ERROR_INVALID_VALUE, "layers without a size or a resolved buffer");
    if ((size_t) width * (size_t) height > ((size_t) 1 << 28)) return refuse(TWK_ERROR_INVALID_VALUE, "width*height must be at most 2^28");
    const size_t pixels = (size_t) width * height, layerBytes = pixels * (size_t) k.layers * sizeof(float4), outBytes = pixels * pixelBytes(dev);
    const char* a = static_cast<const char*>(layers); const char* b = static_cast<const char*>(resolved);
    if (a < b + outBytes && b < a + layerBytes) return refuse(TWK_ERROR_INVALID_VALUE, "the resolved buffer overlaps the layers");
  }
  if ((rc = activate(dev, name))) return rc;
  if (own)
  {
    if (!dev->cascadeEnabled || !dev->stateSet) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own layers need twk_enable_cascade(1) and twk_set_state");
    if (dev->state.distribution && 1 < dev->count)
      return refuse(TWK_ERROR_INVALID_STATE, "the handle's buffer is a packed tile buffer (distribution 1, several devices): the 3x3 window would cross tile borders; assemble every layer with twk_compositor and pass them");
    if (!sameParameters(c, dev->cascadeParameters)) return refuse(TWK_ERROR_INVALID_VALUE, "cp differs from the parameters the handle's layers were enabled with");
    if ((rc = ensureStreams(dev))) return rc;
    width = dev->launchWidth; height = dev->state.resolution[1];
    if ((rc = ensurePicture(dev, dev->resolved, width, height))) return rc;
    layers = dev->d_cascade; resolved = dev->resolved.pixels;
  }
  if ((rc = growIdle(dev, dev->d_cascadeLambda, (size_t) width * height * (size_t) k.layers))) return rc;
  launchCascadeResolve(k, kappa, static_cast<const float4*>(layers), dev->d_cascadeLambda, width, height, resolved, halfOutput(dev), dev->stream);
  HIP_TRY(hipGetLastError());
  if (own) dev->resolved.valid = true;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_cascade_resolve")

int twk_get_resolved_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_resolved_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!(pointer = currentPicture(dev, dev->resolved)))
      return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_resolved_device_pointer: no twk_cascade_resolve on the handle's own layers since they last changed shape");
    size = dev->resolved.count() * pixelBytes(dev);
    return (int) TWK_SUCCESS;
  });
}
TWK_CATCH("twk_get_resolved_device_pointer")

int twk_read_resolved(TwkDevice dev, float* rgbaHost, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_resolved"); if (rc) return rc;
  return readBack(dev, "twk_read_resolved", {currentPicture(dev, dev->resolved), "no twk_cascade_resolve on the handle's own layers since they last changed shape", dev->resolved.count(), 0, true},
                  rgbaHost, numFloats, 4, "launchWidth*height*4 floats");
}
TWK_CATCH("twk_read_resolved")

int twk_cascade_fold_host(const TwkCascade* cp, const float* samples, size_t numSamples, size_t numElements, unsigned int firstIteration, int debugExceptions, float* layers)
try
{
  const char* name = "twk_cascade_fold_host";
  if (!samples || !layers) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  TwkCascade defaults, c; cascadeDefaults(defaults);
  CascadeConstants k;
  int rc = cascadeParameters(name, cp, defaults, c, k); if (rc) return rc;
  std::vector<float4> copy(numElements * (size_t) k.layers); // (a host array of floats need not have a float4's alignment)
  memcpy(copy.data(), layers, copy.size() * sizeof(float4));
  float4* layer = copy.data();
  for (size_t i = 0; i < numElements; ++i)
  {
    CascadeSums s;
    cascadeLoad(k, layer, numElements, i, s);
    bool touched = false;
    for (size_t n = 0; n < numSamples; ++n)
    {
      // the keep rule and the false colours of shade_device.h foldSample
      const float* r = samples + 4 * (n * numElements + i);
      if (r[3] == 0.0f) continue;
      float x = r[0], y = r[1], z = r[2];
      bool keep = !(x != x || y != y || z != z);
      if (debugExceptions)
      {
        if (!keep)                                                               { x = 1000000.0f; y = 0.0f; z = 0.0f; }
        else if (!cascadeFinite(x) || !cascadeFinite(y) || !cascadeFinite(z))   { x = 0.0f; y = 1000000.0f; z = 0.0f; }
        else if (x < 0.0f || y < 0.0f || z < 0.0f)                               { x = 0.0f; y = 0.0f; z = 1000000.0f; }
        keep = true;
      }
      if (!keep) continue;
      cascadeFoldSample(k, s, firstIteration + (unsigned int) n, x, y, z);
      touched = true;
    }
    if (touched) cascadeStore(k, layer, numElements, i, s);
  }
  memcpy(layers, copy.data(), copy.size() * sizeof(float4));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_cascade_fold_host")

int twk_cascade_resolve_host(const TwkCascade* cp, const TwkCascadeResolve* rp, const float* layers, int width, int height, float* resolved)
try
{
  const char* name = "twk_cascade_resolve_host";
  if (!layers || !resolved) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  TwkCascade defaults, c; cascadeDefaults(defaults);
  CascadeConstants k;
  float kappa;
  int rc = cascadeParameters(name, cp, defaults, c, k); if (rc) return rc;
  if ((rc = resolveParameters(name, rp, kappa))) return rc;
  if (width < 1 || height < 1) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": width and height must be >= 1");
  const size_t pixels = (size_t) width * height;
  std::vector<float4> copy(pixels * (size_t) k.layers); // (a host array of floats need not have a float4's alignment)
  memcpy(copy.data(), layers, copy.size() * sizeof(float4));
  const float4* layer = copy.data();
  std::vector<float> lambda(pixels * (size_t) k.layers);
  for (size_t i = 0; i < lambda.size(); ++i) lambda[i] = cascadeLambda(layer[i]);
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x)
    {
      const float4 v = cascadeResolvePixel(k, kappa, layer, lambda.data(), pixels, width, height, x, y);
      memcpy(resolved + 4 * ((size_t) y * width + x), &v, sizeof(v));
    }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_cascade_resolve_host")

} // extern "C"
