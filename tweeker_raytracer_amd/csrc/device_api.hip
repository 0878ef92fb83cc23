// The per-GPU renderer behind the C ABI of include/tweeker_hip.h (≙ rtigo3's Device family,
// reference apps/rtigo3/src/Device.cpp + DeviceSingleGPU.cpp + DeviceMultiGPULocalCopy.cpp).
// Host code here only moves data and enqueues kernels; nothing is ever computed on the CPU in place
// of a kernel. Without a HIP device every entry point that needs one fails.
// This file: the error state, the handle's life, the setters of state, camera, lights, materials and textures, the run-time
// switches, and the output, AOV, moments and geometry buffers with their readers (device_handle.h names the other files); and what
// every reader of every file ends in: readBack, copyBack, readPixels. twk_device_destroy frees no buffer by name: the handle's
// buffers are DeviceArray members (device_buffers.h).
#include "device_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

// ---------------------------------------------------------------------------------------------
static thread_local std::string g_lastError;

int twkSetError(int code, const std::string& message)
{
  g_lastError = message;
  return code;
}

// Exact f16 -> f32 (every half is a float): signed zeros, subnormals, +-inf and NaN payloads are kept
static float halfToFloat(const uint16_t h)
{
  const uint32_t sign = (uint32_t) (h & 0x8000u) << 16, exponent = (h >> 10) & 0x1fu, mantissa = h & 0x3ffu;
  uint32_t bits;
  if (exponent == 0x1fu)    bits = sign | 0x7f800000u | (mantissa << 13);
  else if (exponent != 0u)  bits = sign | ((exponent + 112u) << 23) | (mantissa << 13);
  else if (mantissa == 0u)  bits = sign;
  else                      bits = sign | asUint((float) mantissa * 5.9604644775390625e-8f); // mantissa * 2^-24, exact
  return asFloat(bits);
}

// Copies `numPixels` pixels of a device output / AOV buffer to host memory: `raw`, in the output format as they are; else as
// RGBA32F, widening RGBA16F exactly
int twk::readPixels(TwkDevice dev, const void* src, void* host, size_t numPixels, bool raw)
{
  if (raw || !halfOutput(dev))
  {
    HIP_TRY(hipMemcpy(host, src, numPixels * pixelBytes(dev), hipMemcpyDeviceToHost));
    return TWK_SUCCESS;
  }
  std::vector<uint16_t> halves(numPixels * 4);
  HIP_TRY(hipMemcpy(halves.data(), src, numPixels * 8, hipMemcpyDeviceToHost));
  float* rgbaHost = static_cast<float*>(host);
  for (size_t i = 0; i < halves.size(); ++i) rgbaHost[i] = halfToFloat(halves[i]);
  return TWK_SUCCESS;
}

// What every reader ends in, on an active handle: everything enqueued runs, then `count` elements go to the host (elementBytes 0:
// pixels of the output format, widened to RGBA32F); dropped: the buffer is a pass's result, so a lost traversal push is reported
int twk::copyBack(TwkDevice dev, const char* name, const void* source, size_t count, size_t elementBytes, void* host, bool dropped)
{
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if (elementBytes == 0) { const int rc = readPixels(dev, source, host, count, false); if (rc) return rc; }
  else HIP_TRY(hipMemcpy(host, source, count * elementBytes, hipMemcpyDeviceToHost));
  return dropped ? checkDroppedPushes(dev, name) : TWK_SUCCESS;
}

// One reader, on an active handle: `given` is the size the caller passed, in its own unit of `unit` per element (sizeText: what
// the buffer must hold)
int twk::readBack(TwkDevice dev, const char* name, const Readback& r, void* host, size_t given, size_t unit, const char* sizeText, bool dropped)
{
  if (!host) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL buffer");
  if (!r.source && r.ownShape) return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": " + r.refusal);
  if (given != r.count * unit) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": buffer must hold " + sizeText);
  if (!r.source) return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": " + r.refusal);
  return copyBack(dev, name, r.source, r.count, r.elementBytes, host, dropped);
}

// The on/off switches that only set one flag of the handle, once everything enqueued has run with the old value
int twk::setSwitch(TwkDevice dev, const char* where, bool TwkDevice_t::*flag, int enable)
{
  int rc = activate(dev, where); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->*flag = (enable != 0);
  return TWK_SUCCESS;
}

// MaterialGUI → MaterialDefinition, Device.cpp:1022-1050
static DevMaterial convertMaterial(const TwkMaterialGUI& g)
{
  DevMaterial m;
  memset(&m, 0, sizeof(m));
  m.textureAlbedo = g.useAlbedoTexture ? (TWK_TEXTURE_ALBEDO + 1) : 0;
  m.textureCutout = g.useCutoutTexture ? (TWK_TEXTURE_CUTOUT + 1) : 0;
  m.roughness[0] = g.roughness[0]; m.roughness[1] = g.roughness[1];
  m.indexBSDF = g.indexBSDF;
  m.albedo[0] = g.albedo[0]; m.albedo[1] = g.albedo[1]; m.albedo[2] = g.albedo[2];
  m.absorption[0] = m.absorption[1] = m.absorption[2] = 0.0f;
  if (0.0f < g.absorptionScale)
  {
    const float x = -logf(fmax(0.0001f, g.absorptionColor[0]));
    const float y = -logf(fmax(0.0001f, g.absorptionColor[1]));
    const float z = -logf(fmax(0.0001f, g.absorptionColor[2]));
    m.absorption[0] = x * g.absorptionScale; m.absorption[1] = y * g.absorptionScale; m.absorption[2] = z * g.absorptionScale;
  }
  m.ior   = g.ior;
  m.flags = g.thinwalled ? TWK_FLAG_THINWALLED : 0u;
  return m;
}

// Spherical environment CDFs + integral, Texture.cpp:1499-1645.
static float gaussianFilter(const float* rgba, unsigned int width, unsigned int height, unsigned int x, unsigned int y)
{
  const unsigned int left   = (0 < x)          ? x - 1 : width - 1;
  const unsigned int right  = (x < width - 1)  ? x + 1 : 0;
  const unsigned int bottom = (0 < y)          ? y - 1 : y;
  const unsigned int top    = (y < height - 1) ? y + 1 : y;
  auto sum3 = [&](unsigned int xx, unsigned int yy) { const float* q = rgba + ((size_t) width * yy + xx) * 4; return q[0] + q[1] + q[2]; };
  float intensity = sum3(x, y) * 0.619347f;
  float f = sum3(x, bottom);
  f += sum3(left, y);
  f += sum3(right, y);
  f += sum3(x, top);
  intensity += f * 0.0838195f;
  f  = sum3(left, bottom);
  f += sum3(right, bottom);
  f += sum3(left, top);
  f += sum3(right, top);
  intensity += f * 0.0113437f;
  return intensity / 3.0f;
}

static void calculateSphericalCDF(const float* rgba, unsigned int width, unsigned int height,
                                  std::vector<float>& cdfU, std::vector<float>& cdfV, float& integralOut)
{
  std::vector<float> funcU((size_t) width * height), funcV(height + 1);
  float sum = 0.0f;
  for (unsigned int y = 0; y < height; ++y)
  {
    const float sinTheta = float(sin(M_PI * (double(y) + 0.5) / double(height)));
    for (unsigned int x = 0; x < width; ++x)
    {
      const float value = gaussianFilter(rgba, width, height, x, y);
      funcU[(size_t) y * width + x] = value * sinTheta;
      const float* q = rgba + ((size_t) y * width + x) * 4;
      const float intensity = (q[0] + q[1] + q[2]) / 3.0f;
      sum += intensity * sinTheta;
    }
  }
  integralOut = sum * 2.0f * kPi * kPi / float(width * height);

  cdfU.assign((size_t) (width + 1) * height, 0.0f);
  cdfV.assign(height + 1, 0.0f);
  for (unsigned int y = 0; y < height; ++y)
  {
    const size_t row = (size_t) y * (width + 1);
    cdfU[row] = 0.0f;
    for (unsigned int x = 1; x <= width; ++x) cdfU[row + x] = cdfU[row + x - 1] + funcU[(size_t) y * width + x - 1];
    const float integral = cdfU[row + width];
    funcV[y] = integral;
    if (integral != 0.0f) { for (unsigned int x = 1; x <= width; ++x) cdfU[row + x] /= integral; }
    else                  { for (unsigned int x = 1; x <= width; ++x) cdfU[row + x] = float(x) / float(width); }
  }
  cdfV[0] = 0.0f;
  for (unsigned int y = 1; y <= height; ++y) cdfV[y] = cdfV[y - 1] + funcV[y - 1];
  const float integral = cdfV[height];
  if (integral != 0.0f) { for (unsigned int y = 1; y <= height; ++y) cdfV[y] /= integral; }
  else                  { for (unsigned int y = 1; y <= height; ++y) cdfV[y] = float(y) / float(height); }
}

// The A/B and tuning switches a handle reads from the environment once, when it is created
static void readEnvironmentSwitches(TwkDevice_t* dev)
{
  if (const char* e = getenv("TWK_PASS_LANES")) dev->lanesForced = std::max(0, std::min(TWK_MAX_LANES, atoi(e)));
  if (const char* e = getenv("TWK_LANE_TRACE_WAVES")) dev->laneTraceWaves = std::max(0, atoi(e));
  if (const char* e = getenv("TWK_TOP_CACHE")) dev->topCache = (atoi(e) != 0);
  if (const char* e = getenv("TWK_DIRECT_SMALL_LEAVES")) dev->directSmallLeaves = (atoi(e) != 0);
  if (const char* e = getenv("TWK_COSTED_CUTS")) dev->costedCuts = (atoi(e) != 0);
  if (const char* e = getenv("TWK_FUSED_PRIMARY")) dev->fusedPrimary = (atoi(e) != 0);
  if (const char* e = getenv("TWK_TILE_ENTRIES")) dev->tileEntries = (atoi(e) != 0);
  if (const char* e = getenv("TWK_WIDE_ROOT")) dev->wideRoot = (atoi(e) != 0);
  if (const char* e = getenv("TWK_PACKED_QUEUE")) dev->packedQueue = (atoi(e) != 0);
  if (const char* e = getenv("TWK_SLIM_STREAMS")) dev->slimStreams = (atoi(e) != 0);
  if (const char* e = getenv("TWK_TRIANGLE_PAIRS")) dev->trianglePairs = (atoi(e) != 0);
  if (const char* e = getenv("TWK_SHADE_SORT")) dev->shadeSort = std::max(0, std::min(2, atoi(e)));
  if (const char* e = getenv("TWK_DENOISE_LDS_MAX_STEP")) dev->denoiseLdsMaxStep = dev->denoiseGeometryLdsMaxStep = std::max(0, std::min(128, atoi(e))); // A/B; 128 = the largest step (iterations <= 8)
  if (const char* e = getenv("TWK_TRACE_WAVES_RUNTIME")) dev->traceWavesForced = atoi(e); // A/B: 6 or 7 blocks per CU of the persistent trace kernel
  if (const char* e = getenv("TWK_BUILD_QUALITY")) dev->builder.setQuality(atoi(e)); // A/B: 0 LBVH, 1 binned SAH (default)
  if (const char* e = getenv("TWK_STREAM_BUDGET_MB")) { const long long mb = atoll(e); dev->streamBudgetBytes = (mb > 0) ? (size_t) mb << 20 : 0; }
  if (const char* e = getenv("TWK_ASSEMBLE_STAGE")) dev->assembleStage = (atoi(e) != 0); // twk_assemble_devices stages every source (both paths on one GPU)
  if (const char* e = getenv("TWK_BATCH")) { const int b = atoi(e); dev->batchMax = (b < 1) ? 1 : ((b > 64) ? 64 : b); }
}

// The handle's own accumulations per launch index, freed: the internal output, both AOVs, the moments, the cascade's layers, the
// geometry AOV, the sample counts and the active and plan lists. The next ensureStreams allocates those that are enabled again, zeroed,
// at the new state's size, so that the padding of a packed tile buffer holds zeros whatever the handle rendered before. The path
// streams, spill stacks and scratch keep their capacity; a caller's external output buffer or shared frame is the caller's to clear.
static void dropAccumulations(TwkDevice dev)
{
  dev->d_outputInternal.release(); dev->d_firstHit.release(); dev->d_firstHitInstance.release();
  dev->d_aovAlbedo.release(); dev->d_aovNormal.release();
  dev->d_moments.release();
  dev->d_cascade.release(); dev->resolved.valid = false;
  dev->d_geometry.release();
  dev->d_sampleCounts.release(); dev->d_active.release();
  dev->d_planActive.release(); dev->d_planOffsets.release();
  dropAssembled(dev); // what the handle assembled as a primary has the old frame's shape
}

// =============================================================================================
extern "C" {

const char* twk_last_error(void) { return g_lastError.c_str(); }
int twk_abi_version(void) { return TWK_ABI_VERSION; }

int twk_device_count(int* count)
try
{
  if (!count) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_device_count: NULL argument");
  *count = 0;
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return twkSetError(TWK_ERROR_NO_DEVICE, std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e));
  *count = n;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_device_count")

int twk_device_create(TwkDevice* out, int ordinal, int index, int count, int miss)
try
{
  if (!out) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_device_create: NULL out pointer");
  *out = nullptr;
  if (count < 1 || index < 0 || index >= count) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_device_create: need 0 <= index < count");
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return twkSetError(TWK_ERROR_NO_DEVICE, std::string("twk_device_create: no HIP device available (") + ((e != hipSuccess) ? hipGetErrorString(e) : "device count 0") + "); this library has no CPU path");
  if (ordinal < 0 || ordinal >= n) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_device_create: device ordinal out of range");

  TwkDevice_t* dev = new TwkDevice_t();
  dev->ordinal = ordinal; dev->index = index; dev->count = count; dev->miss = miss;
  memset(&dev->params, 0, sizeof(dev->params));
  memset(&dev->state, 0, sizeof(dev->state));
  // Device.cpp:282-303 defaults
  dev->state.resolution[0] = dev->state.resolution[1] = 1;
  dev->state.tileSize[0] = dev->state.tileSize[1] = 8;
  dev->state.pathLengths[0] = 2; dev->state.pathLengths[1] = 5;
  dev->state.epsilonFactor = 500.0f;
  dev->state.clockFactor = 1000.0f;

  hipError_t err = hipSetDevice(ordinal);
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&dev->stream, hipStreamNonBlocking);
  hipDeviceProp_t prop;
  if (err == hipSuccess) err = hipGetDeviceProperties(&prop, ordinal);
  if (err != hipSuccess)
  {
    delete dev;
    return twkSetError(TWK_ERROR_NO_DEVICE, std::string("twk_device_create: ") + hipGetErrorString(err));
  }
  dev->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  readEnvironmentSwitches(dev);
  memset(&dev->buildInfo, 0, sizeof(dev->buildInfo));
  *out = dev;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_device_create")

int twk_device_destroy(TwkDevice dev)
try
{
  if (!dev) return TWK_SUCCESS;
  dev->pendingCount = 0; // recorded but never observed launches are dropped
  (void) hipSetDevice(dev->ordinal);
  if (dev->stream) (void) hipStreamSynchronize(dev->stream);
  for (TimedLaunch& t : dev->timed) { (void) hipEventDestroy(t.start); (void) hipEventDestroy(t.stop); }
  if (dev->assembleReady) (void) hipEventDestroy(dev->assembleReady);
  if (dev->assembleDone) (void) hipEventDestroy(dev->assembleDone);
  dev->builder.release();
  for (int k = 1; k < TWK_MAX_LANES; ++k)
  {
    if (dev->laneStream[k]) (void) hipStreamDestroy(dev->laneStream[k]);
    if (dev->laneDone[k]) (void) hipEventDestroy(dev->laneDone[k]);
  }
  if (dev->laneFork) (void) hipEventDestroy(dev->laneFork);
  if (dev->stream) (void) hipStreamDestroy(dev->stream);
  if (dev->h_dropped) (void) hipHostFree(dev->h_dropped);
  delete dev; // every device buffer is a DeviceArray member: freed here
  return TWK_SUCCESS;
}
TWK_CATCH("twk_device_destroy")

int twk_set_state(TwkDevice dev, const TwkDeviceState* s)
try
{
  int rc = activate(dev, "twk_set_state"); if (rc) return rc;
  if (!s) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_state: NULL state");
  if (s->resolution[0] < 1 || s->resolution[1] < 1) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_state: resolution must be >= 1");
  if (s->tileSize[0] < 1 || s->tileSize[1] < 1 || (s->tileSize[0] & (s->tileSize[0] - 1)) || (s->tileSize[1] & (s->tileSize[1] - 1)))
    return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_state: tileSize must be a power of two");
  if (s->pathLengths[1] < 0 || s->pathLengths[1] > TWK_MAX_DEPTH) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_state: pathLengths.y must be in [0, 64]");
  if (s->lensShader < 0 || s->lensShader > 2) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_state: lensShader must be 0..2");
  HIP_TRY(hipStreamSynchronize(dev->stream)); // Device.cpp:1194-1195
  if (dev->stateSet && (dev->state.resolution[0] != s->resolution[0] || dev->state.resolution[1] != s->resolution[1])) dropTemporal(dev);
  int launchWidth = s->resolution[0];
  if (s->distribution && 1 < dev->count)
  {
    // DeviceMultiGPULocalCopy.cpp:84-97
    const int width = (s->resolution[0] + dev->count - 1) / dev->count;
    const int mask  = s->tileSize[0] - 1;
    launchWidth = (width + mask) & ~mask;
  }
  // The frame's geometry: which pixel a launch index is. When it changes, every accumulation per launch index starts as a fresh
  // handle's does; a state that keeps it (path lengths, lens shader, epsilon, ...) allocates and clears nothing.
  const TwkDeviceState& was = dev->state;
  if (!dev->stateSet || was.resolution[0] != s->resolution[0] || was.resolution[1] != s->resolution[1] || was.tileSize[0] != s->tileSize[0] ||
      was.tileSize[1] != s->tileSize[1] || was.distribution != s->distribution || dev->launchWidth != launchWidth)
    dropAccumulations(dev);
  dev->state = *s; dev->launchWidth = launchWidth;
  dev->stateSet = true; staleGeometry(dev); dropAdaptive(dev);
  const size_t needBytes = (size_t) (dev->outputFrame ? s->resolution[0] : dev->launchWidth) * s->resolution[1] * pixelBytes(dev);
  if (dev->d_outputExternal && dev->outputExternalBytes < needBytes)
  {
    dev->d_outputExternal = nullptr; dev->outputExternalBytes = 0; dev->outputFrame = false; // too small for the new state: fall back to the internal buffer
  }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_set_state")

int twk_init_cameras(TwkDevice dev, const TwkCameraDefinition* c, int count)
try
{
  int rc = activate(dev, "twk_init_cameras"); if (rc) return rc;
  if (!c || count < 1) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_init_cameras: at least one camera is required");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->cameras.assign(c, c + count); staleGeometry(dev);
  if ((rc = dev->d_camera.ensure(sizeof(TwkCameraDefinition) / sizeof(float)))) return rc;
  HIP_TRY(hipMemcpyAsync(dev->d_camera, dev->cameras.data(), sizeof(TwkCameraDefinition), hipMemcpyHostToDevice, dev->stream)); // the lens shaders read cameraDefinitions[0]
  return TWK_SUCCESS;
}
TWK_CATCH("twk_init_cameras")

int twk_update_camera(TwkDevice dev, int idCamera, const TwkCameraDefinition* c)
try
{
  int rc = activate(dev, "twk_update_camera"); if (rc) return rc;
  if (!c || idCamera < 0 || idCamera >= (int) dev->cameras.size()) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_update_camera: bad camera id");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->cameras[idCamera] = *c;
  if (idCamera == 0) staleGeometry(dev);
  if (idCamera == 0) HIP_TRY(hipMemcpyAsync(dev->d_camera, dev->cameras.data(), sizeof(TwkCameraDefinition), hipMemcpyHostToDevice, dev->stream));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_update_camera")

int twk_init_lights(TwkDevice dev, const TwkLightDefinition* l, int count)
try
{
  int rc = activate(dev, "twk_init_lights"); if (rc) return rc;
  if (count < 0 || (count > 0 && !l)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_init_lights: bad arguments");
  if (dev->built && count <= dev->maxInstanceLight)
    return twkSetError(TWK_ERROR_INVALID_STATE, "twk_init_lights: the built scene has an instance with light index " + std::to_string(dev->maxInstanceLight) + "; " + std::to_string(count) + " lights would leave it dangling (twk_clear_scene first)");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->d_lights.release();
  dev->lights.assign(l, l + count); dropLightAnchors(dev);
  if (count > 0)
  {
    if ((rc = dev->d_lights.allocate((size_t) count))) return rc;
    HIP_TRY(hipMemcpyAsync(dev->d_lights, dev->lights.data(), sizeof(DevLight) * count, hipMemcpyHostToDevice, dev->stream));
  }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_init_lights")

int twk_update_light(TwkDevice dev, int idLight, const TwkLightDefinition* l)
try
{
  int rc = activate(dev, "twk_update_light"); if (rc) return rc;
  if (!l || idLight < 0 || idLight >= (int) dev->lights.size()) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_update_light: bad light id");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->lights[idLight] = *l;
  if ((size_t) idLight < dev->lightAnchors.size()) dev->lightAnchors[idLight].valid = false; // the next move anchors on this definition (light_motion.h)
  HIP_TRY(hipMemcpyAsync(dev->d_lights + idLight, &dev->lights[idLight], sizeof(DevLight), hipMemcpyHostToDevice, dev->stream));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_update_light")

int twk_get_light(TwkDevice dev, int idLight, TwkLightDefinition* out)
try
{
  const char* name = "twk_get_light";
  if (!dev || !out) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + (dev ? ": NULL definition" : ": NULL device handle"));
  if (idLight < 0 || idLight >= (int) dev->lights.size()) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": bad light id");
  *out = dev->lights[idLight];
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_light")

int twk_enable_emitter_motion(TwkDevice dev, int on)
try
{
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_enable_emitter_motion: NULL device handle");
  if (on != 0 && on != 1) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_enable_emitter_motion: the switch is " + std::to_string(on) + ", neither 0 nor 1");
  dev->emitterMotion = (on == 1); // read by the transform calls; the anchors stay: a light that has moved keeps deriving from where it started
  return TWK_SUCCESS;
}
TWK_CATCH("twk_enable_emitter_motion")

int twk_get_emitter_motion(TwkDevice dev, int* on)
try
{
  if (!dev || !on) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_emitter_motion: NULL argument");
  *on = dev->emitterMotion ? 1 : 0;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_emitter_motion")

int twk_light_moved_host(const TwkLightDefinition* anchor, const float anchorTransform[12], const float transform[12], TwkLightDefinition* out)
try
{
  const char* name = "twk_light_moved_host";
  if (!anchor || !anchorTransform || !transform || !out) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  TwkLightDefinition moved; // `out` may be `anchor`
  if (const char* why = lightMoved(*anchor, anchorTransform, transform, moved)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + why);
  *out = moved;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_light_moved_host")

int twk_init_materials(TwkDevice dev, const TwkMaterialGUI* m, int count)
try
{
  int rc = activate(dev, "twk_init_materials"); if (rc) return rc;
  if (!m || count < 1) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_init_materials: at least one material is required");
  if (dev->built && count <= dev->maxInstanceMaterial)
    return twkSetError(TWK_ERROR_INVALID_STATE, "twk_init_materials: the built scene has an instance with material index " + std::to_string(dev->maxInstanceMaterial) + "; " + std::to_string(count) + " materials would leave it dangling (twk_clear_scene first)");
  for (int i = 0; i < count; ++i)
  {
    if (m[i].indexBSDF < 0 || m[i].indexBSDF > 4) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_init_materials: indexBSDF out of range");
  }
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->materials.resize(count);
  for (int i = 0; i < count; ++i) dev->materials[i] = convertMaterial(m[i]);
  if ((rc = dev->d_materials.ensure((size_t) count))) return rc;
  HIP_TRY(hipMemcpyAsync(dev->d_materials, dev->materials.data(), sizeof(DevMaterial) * count, hipMemcpyHostToDevice, dev->stream));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_init_materials")

int twk_update_material(TwkDevice dev, int idMaterial, const TwkMaterialGUI* m)
try
{
  int rc = activate(dev, "twk_update_material"); if (rc) return rc;
  if (!m || idMaterial < 0 || idMaterial >= (int) dev->materials.size()) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_update_material: bad material id");
  if (m->indexBSDF < 0 || m->indexBSDF > 4) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_update_material: indexBSDF out of range");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->materials[idMaterial] = convertMaterial(*m);
  HIP_TRY(hipMemcpyAsync(dev->d_materials + idMaterial, &dev->materials[idMaterial], sizeof(DevMaterial), hipMemcpyHostToDevice, dev->stream));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_update_material")

int twk_init_texture(TwkDevice dev, int slot, const float* rgba, int width, int height)
try
{
  int rc = activate(dev, "twk_init_texture"); if (rc) return rc;
  if (slot < 0 || slot > 2 || !rgba || width < 1 || height < 1) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_init_texture: bad arguments");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  const size_t bytes = sizeof(float4) * (size_t) width * height;
  if ((rc = dev->d_texels[slot].allocate((size_t) width * height))) return rc;
  HIP_TRY(hipMemcpy(dev->d_texels[slot], rgba, bytes, hipMemcpyHostToDevice));
  DevTexture& t = dev->params.textures[slot];
  t.texels = dev->d_texels[slot]; t.width = width; t.height = height; t.clampV = (slot == TWK_TEXTURE_ENVIRONMENT) ? 1 : 0; t.pad = 0;
  if (slot == TWK_TEXTURE_ENVIRONMENT)
  {
    std::vector<float> cdfU, cdfV; float integral = 1.0f;
    calculateSphericalCDF(rgba, (unsigned int) width, (unsigned int) height, cdfU, cdfV, integral);
    dev->d_envCDF_U.release(); dev->d_envCDF_V.release();
    if ((rc = dev->d_envCDF_U.allocate(cdfU.size())) || (rc = dev->d_envCDF_V.allocate(cdfV.size()))) return rc;
    HIP_TRY(hipMemcpy(dev->d_envCDF_U, cdfU.data(), sizeof(float) * cdfU.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev->d_envCDF_V, cdfV.data(), sizeof(float) * cdfV.size(), hipMemcpyHostToDevice));
    dev->params.envWidth = (unsigned int) width; dev->params.envHeight = (unsigned int) height; dev->params.envIntegral = integral;
  }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_init_texture")

int twk_sync(TwkDevice dev)
try
{
  int rc = activate(dev, "twk_sync"); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  return checkDroppedPushes(dev, "twk_sync");
}
TWK_CATCH("twk_sync")

int twk_get_launch_width(TwkDevice dev, int* launchWidth)
try
{
  if (!dev || !launchWidth) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_launch_width: NULL argument");
  *launchWidth = dev->launchWidth;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_launch_width")

// twk_read_output and twk_read_output_raw: `raw`, the pixels as they are (`size` in bytes); else RGBA32F (`size` in floats)
static int readOutput(TwkDevice dev, void* host, size_t size, bool raw, const char* where)
{
  int rc = activate(dev, where); if (rc) return rc;
  return readBack(dev, where, {ownOutput(dev), "nothing has been rendered", outputPixels(dev), raw ? pixelBytes(dev) : 0, false}, host, size, raw ? pixelBytes(dev) : 4,
                  raw ? "launchWidth*height pixels (width*height with a shared frame) of the output format" : "launchWidth*height*4 floats (width*height*4 with a shared frame)", true);
}

int twk_read_output(TwkDevice dev, float* rgbaHost, size_t numFloats)
try
{
  return readOutput(dev, rgbaHost, numFloats, false, "twk_read_output");
}
TWK_CATCH("twk_read_output")

int twk_read_output_raw(TwkDevice dev, void* host, size_t bytes)
try
{
  return readOutput(dev, host, bytes, true, "twk_read_output_raw");
}
TWK_CATCH("twk_read_output_raw")

int twk_set_output_format(TwkDevice dev, int format)
try
{
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_output_format: NULL device handle");
  if (format != TWK_OUTPUT_FLOAT4 && format != TWK_OUTPUT_HALF4) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_output_format: format must be TWK_OUTPUT_FLOAT4 or TWK_OUTPUT_HALF4");
  int rc = activate(dev, "twk_set_output_format"); if (rc) return rc;
  if (format == dev->outputFormat) return TWK_SUCCESS;
  if (dev->d_outputExternal && dev->stateSet && dev->outputExternalBytes < outputPixels(dev) * pixelBytes(format))
    return twkSetError(TWK_ERROR_INVALID_STATE, "twk_set_output_format: the external output buffer is too small for the new format");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  // the internal output and AOV buffers are allocated again at the new pixel size, zeroed, by the next ensureStreams
  dev->d_outputInternal.release(); // (its group with it: ensureStreams)
  dev->d_aovAlbedo.release(); dev->d_aovNormal.release();
  dev->denoised.release(); // a denoised picture is in the format it was filtered in
  dropAssembled(dev); // and so is an assembled frame
  dev->outputFormat = format; dropAdaptive(dev);
  return dev->stateSet ? ensureStreams(dev) : TWK_SUCCESS;
}
TWK_CATCH("twk_set_output_format")

int twk_get_output_format(TwkDevice dev, int* format)
try
{
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_output_format: NULL device handle");
  if (!format) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_output_format: NULL argument");
  *format = dev->outputFormat;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_output_format")

int twk_set_shader_variant(TwkDevice dev, int variant)
try
{
  int rc = activate(dev, "twk_set_shader_variant"); if (rc) return rc;
  if (variant != TWK_SHADERS_RTIGO3 && variant != TWK_SHADERS_OPTIX7GUI) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_shader_variant: unknown variant");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->shaderVariant = variant;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_set_shader_variant")

int twk_enable_aov(TwkDevice dev, int enable)
try
{
  return setSwitch(dev, "twk_enable_aov", &TwkDevice_t::aovEnabled, enable);
}
TWK_CATCH("twk_enable_aov")

int twk_enable_moments(TwkDevice dev, int enable)
try
{
  int rc = activate(dev, "twk_enable_moments"); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->momentsEnabled = (enable != 0); dropAdaptive(dev);
  if (!dev->momentsEnabled) { dev->d_moments.release(); return TWK_SUCCESS; } // enabled again: a zeroed buffer
  return dev->stateSet ? ensureStreams(dev) : TWK_SUCCESS; // allocated, zeroed, here or by the first pass after twk_set_state
}
TWK_CATCH("twk_enable_moments")

int twk_read_moments(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_moments"); if (rc) return rc;
  const size_t n = launchIndices(dev);
  return readBack(dev, "twk_read_moments", {ownMoments(dev, n), "twk_enable_moments(1) and twk_set_state first", n, sizeof(float4), false}, host, numFloats, 4, "launchWidth*height*4 floats");
}
TWK_CATCH("twk_read_moments")

int twk_get_moments_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_moments_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!dev->momentsEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_moments_device_pointer: twk_enable_moments(1) and twk_set_state first");
    const int rc = ensureStreams(dev);
    pointer = dev->d_moments; size = launchIndices(dev) * sizeof(float4);
    return rc;
  });
}
TWK_CATCH("twk_get_moments_device_pointer")

int twk_set_sample_offset(TwkDevice dev, unsigned int offset)
try
{
  int rc = activate(dev, "twk_set_sample_offset"); if (rc) return rc; // recorded launches are rendered with the offset they were recorded under
  dev->sampleOffset = offset;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_set_sample_offset")

int twk_enable_geometry(TwkDevice dev, int enable)
try
{
  int rc = activate(dev, "twk_enable_geometry"); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->geometryEnabled = (enable != 0); staleGeometry(dev);
  if (!dev->geometryEnabled) { dev->d_geometry.release(); return TWK_SUCCESS; } // enabled again: a zeroed buffer
  return dev->stateSet ? ensureStreams(dev) : TWK_SUCCESS; // allocated, zeroed, here or by the first use after twk_set_state
}
TWK_CATCH("twk_enable_geometry")

int twk_read_geometry(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_geometry"); if (rc) return rc;
  const size_t n = launchIndices(dev);
  return readBack(dev, "twk_read_geometry", {ownGeometry(dev, n), "twk_enable_geometry(1) and twk_set_state first", n, sizeof(float4), false}, host, numFloats, 4, "launchWidth*height*4 floats", true);
}
TWK_CATCH("twk_read_geometry")

int twk_get_geometry_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_geometry_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!dev->geometryEnabled || !dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_geometry_device_pointer: twk_enable_geometry(1) and twk_set_state first");
    const int rc = ensureStreams(dev);
    pointer = dev->d_geometry; size = launchIndices(dev) * sizeof(float4);
    return rc;
  });
}
TWK_CATCH("twk_get_geometry_device_pointer")

int twk_set_time_view(TwkDevice dev, int enable)
try
{
  return setSwitch(dev, "twk_set_time_view", &TwkDevice_t::timeView, enable);
}
TWK_CATCH("twk_set_time_view")

int twk_set_next_event_estimation(TwkDevice dev, int enable)
try
{
  return setSwitch(dev, "twk_set_next_event_estimation", &TwkDevice_t::nextEventEstimation, enable);
}
TWK_CATCH("twk_set_next_event_estimation")

int twk_set_debug_exceptions(TwkDevice dev, int enable)
try
{
  return setSwitch(dev, "twk_set_debug_exceptions", &TwkDevice_t::debugExceptions, enable);
}
TWK_CATCH("twk_set_debug_exceptions")

// twk_read_aov and twk_read_aov_raw: `raw` and `size` as in readOutput
static int readAov(TwkDevice dev, int which, void* host, size_t size, bool raw, const char* where)
{
  int rc = activate(dev, where); if (rc) return rc;
  if (!host || (which != TWK_AOV_ALBEDO && which != TWK_AOV_NORMAL)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(where) + ": bad arguments");
  const size_t n = launchIndices(dev);
  return readBack(dev, where, {(which == TWK_AOV_ALBEDO) ? ownAlbedo(dev, n) : ownNormal(dev, n), "nothing has been rendered with twk_enable_aov(1)", n, raw ? pixelBytes(dev) : 0, false}, host, size,
                  raw ? pixelBytes(dev) : 4, raw ? "launchWidth*height pixels of the output format" : "launchWidth*height*4 floats");
}

int twk_read_aov(TwkDevice dev, int which, float* rgbaHost, size_t numFloats)
try
{
  return readAov(dev, which, rgbaHost, numFloats, false, "twk_read_aov");
}
TWK_CATCH("twk_read_aov")

int twk_read_aov_raw(TwkDevice dev, int which, void* host, size_t bytes)
try
{
  return readAov(dev, which, host, bytes, true, "twk_read_aov_raw");
}
TWK_CATCH("twk_read_aov_raw")

int twk_get_output_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_output_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_output_device_pointer: twk_set_state first");
    const int rc = ensureStreams(dev);
    pointer = ownOutput(dev); size = launchIndices(dev) * pixelBytes(dev);
    return rc;
  });
}
TWK_CATCH("twk_get_output_device_pointer")

// twk_set_output_device_pointer (the caller's packed launchWidth x H buffer) and twk_set_shared_frame (`frame`: a full W x H frame)
static int setExternalOutput(TwkDevice dev, void* dptr, size_t bytes, bool frame, const char* where)
{
  int rc = activate(dev, where); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dropAdaptive(dev);
  if (dptr == nullptr) { dev->d_outputExternal = nullptr; dev->outputExternalBytes = 0; dev->outputFrame = false; return TWK_SUCCESS; }
  if (!dev->stateSet) return twkSetError(TWK_ERROR_INVALID_STATE, std::string(where) + ": twk_set_state first");
  if (bytes < (size_t) (frame ? dev->state.resolution[0] : dev->launchWidth) * dev->state.resolution[1] * pixelBytes(dev))
    return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(where) + ": buffer smaller than " + (frame ? "width" : "launchWidth") + "*height pixels of the output format (16 bytes RGBA32F, 8 RGBA16F)");
  dev->d_outputExternal = static_cast<float4*>(dptr); dev->outputExternalBytes = bytes; dev->outputFrame = frame;
  return TWK_SUCCESS;
}

int twk_set_output_device_pointer(TwkDevice dev, void* dptr, size_t bytes)
try
{
  return setExternalOutput(dev, dptr, bytes, false, "twk_set_output_device_pointer");
}
TWK_CATCH("twk_set_output_device_pointer")

int twk_set_shared_frame(TwkDevice dev, void* frame, size_t bytes)
try
{
  return setExternalOutput(dev, frame, bytes, true, "twk_set_shared_frame");
}
TWK_CATCH("twk_set_shared_frame")

} // extern "C"
