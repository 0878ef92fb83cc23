// Assembling a tiled frame behind the C ABI (assemble_device.h: the definition): the assembled buffers a handle owns and what drops
// them, the table of a launch (assemble_kernels.hip), the explicit form for gathered blocks (twk_assemble), the in-process form over
// the handles' own buffers with its stream ordering, peer access and staging (twk_assemble_devices), the readers and the host-only form.
// twk_assemble_with_geometry and twk_assemble_devices_with_geometry are the same two forms with the geometry AOV of every tile share
// (twk_render_geometry_tile) as further entries of the same table: one launch, an assembled buffer of its own beside the six planes'.
// An assembled buffer is a DeviceArray of exactly the plane's bytes (ensureAssembled) with a valid flag beside it.
#include "device_handle.h"

#include <algorithm>
#include <cstring>
#include <vector>

static const char* const kPlaneNames[TWK_PLANE_COUNT] = {"TWK_PLANE_OUTPUT", "TWK_PLANE_ALBEDO", "TWK_PLANE_NORMAL", "TWK_PLANE_MOMENTS", "TWK_PLANE_SAMPLE_COUNTS", "TWK_PLANE_CASCADE"};
static const unsigned int kAllPlanes = (1u << TWK_PLANE_COUNT) - 1u;

// log2 of a plane's element size on this handle, and its number of layers
static unsigned int planeElementShift(TwkDevice dev, int plane)
{
  if (plane == TWK_PLANE_SAMPLE_COUNTS) return 2;
  if (plane == TWK_PLANE_MOMENTS || plane == TWK_PLANE_CASCADE) return 4;
  return halfOutput(dev) ? 3 : 4;
}
static size_t planeLayers(TwkDevice dev, int plane) { return (plane == TWK_PLANE_CASCADE) ? (size_t) dev->cascadeK.layers : 1; }
// Bytes of a plane as `columns` x height elements per layer: columns = launchWidth for a packed source, width for the assembled buffer
static size_t planeBytes(TwkDevice dev, int plane, int columns)
{
  return ((size_t) columns * (size_t) dev->state.resolution[1] * planeLayers(dev, plane)) << planeElementShift(dev, plane);
}

// The switch a plane needs; nullptr: it is on (the beauty needs none)
static const char* planeSwitchOff(TwkDevice dev, int plane)
{
  switch (plane)
  {
    case TWK_PLANE_ALBEDO: case TWK_PLANE_NORMAL: return dev->aovEnabled ? nullptr : "twk_enable_aov";
    case TWK_PLANE_MOMENTS:                       return dev->momentsEnabled ? nullptr : "twk_enable_moments";
    case TWK_PLANE_SAMPLE_COUNTS:                 return dev->adaptiveEnabled ? nullptr : "twk_enable_adaptive";
    case TWK_PLANE_CASCADE:                       return dev->cascadeEnabled ? nullptr : "twk_enable_cascade";
    default:                                      return nullptr;
  }
}

// Frees the assembled buffers and the staging block: the getters refuse until the next assemble. Everything enqueued has run.
void twk::dropAssembled(TwkDevice dev)
{
  for (int p = 0; p < TWK_PLANE_COUNT; ++p) { dev->d_assembled[p].release(); dev->assembledValid[p] = false; }
  dev->d_assembledGeometry.release(); dev->assembledGeometryValid = false;
  dev->d_assembleStage.release();
}

// An assembled buffer of exactly `bytes`: one of another size, or none, is freed once everything enqueued has run and allocated
// again, not valid
static int ensureAssembled(TwkDevice primary, DeviceArray<void>& buffer, bool& valid, size_t bytes)
{
  if (buffer && buffer.capacity() == bytes) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(primary->stream));
  valid = false;
  return buffer.allocate(bytes);
}

// Bytes of the geometry AOV as `columns` x height float4
static size_t geometryBytes(TwkDevice dev, int columns) { return (size_t) columns * (size_t) dev->state.resolution[1] * sizeof(float4); }

static AssembleShape assembleShape(TwkDevice dev)
{
  AssembleShape s;
  s.width = dev->state.resolution[0]; s.height = dev->state.resolution[1]; s.launchWidth = dev->launchWidth; s.deviceCount = dev->count;
  s.tileSizeX = dev->state.tileSize[0]; s.tileShiftX = calculateShift(dev->state.tileSize[0]); s.tileShiftY = calculateShift(dev->state.tileSize[1]);
  return s;
}

// What both forms refuse of primary alone, without a HIP call. withGeometry: the geometry AOV is assembled too, an empty mask is legal
static int refusePrimary(const char* name, TwkDevice primary, unsigned int planeMask, bool withGeometry)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if ((planeMask == 0 && !withGeometry) || (planeMask & ~kAllPlanes)) return refuse(TWK_ERROR_INVALID_VALUE, withGeometry ? "the plane mask names an unknown plane" : "the plane mask is empty or names an unknown plane");
  if (!primary->stateSet) return refuse(TWK_ERROR_INVALID_STATE, "twk_set_state first");
  if (!primary->state.distribution && 1 < primary->count) return refuse(TWK_ERROR_INVALID_STATE, "distribution 0 with several devices: every handle holds the whole frame, there are no tiles to assemble");
  if ((size_t) primary->state.resolution[1] > (size_t) 65535 * 4) return refuse(TWK_ERROR_INVALID_VALUE, "the height exceeds what one launch covers");
  for (int p = 0; p < TWK_PLANE_COUNT; ++p)
    if ((planeMask >> p) & 1u)
      if (const char* off = planeSwitchOff(primary, p)) return refuse(TWK_ERROR_INVALID_STATE, std::string(kPlaneNames[p]) + " needs " + off + "(1) on the primary handle");
  if (withGeometry && !primary->geometryEnabled) return refuse(TWK_ERROR_INVALID_STATE, "the geometry AOV needs twk_enable_geometry(1) on the primary handle");
  return TWK_SUCCESS;
}

// Allocates primary's assembled buffers of the requested planes, builds the table and launches; sources[d]: device index d's
// packed buffers, addressable from primary's device. geometry: nullptr, or device index d's packed geometry AOV, which goes out as
// further entries of the same table. primary is active.
static int assembleLaunch(TwkDevice primary, unsigned int planeMask, const std::vector<TwkAssemblySource>& sources, const std::vector<const void*>* geometry = nullptr)
{
  int rc;
  for (int p = 0; p < TWK_PLANE_COUNT; ++p)
    if (((planeMask >> p) & 1u) && (rc = ensureAssembled(primary, primary->d_assembled[p], primary->assembledValid[p], planeBytes(primary, p, primary->state.resolution[0])))) return rc;
  if (geometry && (rc = ensureAssembled(primary, primary->d_assembledGeometry, primary->assembledGeometryValid, geometryBytes(primary, primary->state.resolution[0])))) return rc;
  const AssembleShape s = assembleShape(primary);
  AssembleTable table;
  memset(&table, 0, sizeof(table));
  int used = 0;
  const size_t sourceLayer = (size_t) s.launchWidth * s.height, assembledLayer = (size_t) s.width * s.height;
  for (int p = 0; p < TWK_PLANE_COUNT; ++p)
  {
    if (!((planeMask >> p) & 1u)) continue;
    const unsigned int shift = planeElementShift(primary, p);
    for (size_t layer = 0; layer < planeLayers(primary, p); ++layer)
      for (int d = 0; d < s.deviceCount; ++d)
      {
        AssembleEntry& e = table.entry[used];
        e.source       = static_cast<const char*>(sources[(size_t) d].plane[p]) + ((layer * sourceLayer) << shift);
        e.destination  = static_cast<char*>(primary->d_assembled[p].get()) + ((layer * assembledLayer) << shift);
        e.device       = (unsigned int) d;
        e.elementShift = shift;
        e.groupShift   = assembleGroupShift(s, shift, e.source, e.destination);
        if (++used == TWK_ASSEMBLE_MAX_ENTRIES) // (more than 13 planes and layers x 9 devices: the table is launched in pieces)
        {
          launchAssemble(s, table, used, primary->stream);
          HIP_TRY(hipGetLastError());
          used = 0;
        }
      }
  }
  if (geometry)
    for (int d = 0; d < s.deviceCount; ++d)
    {
      AssembleEntry& e = table.entry[used];
      e.source       = (*geometry)[(size_t) d];
      e.destination  = primary->d_assembledGeometry;
      e.device       = (unsigned int) d;
      e.elementShift = 4;
      e.groupShift   = assembleGroupShift(s, 4, e.source, e.destination);
      if (++used == TWK_ASSEMBLE_MAX_ENTRIES)
      {
        launchAssemble(s, table, used, primary->stream);
        HIP_TRY(hipGetLastError());
        used = 0;
      }
    }
  if (used)
  {
    launchAssemble(s, table, used, primary->stream);
    HIP_TRY(hipGetLastError());
  }
  for (int p = 0; p < TWK_PLANE_COUNT; ++p) if ((planeMask >> p) & 1u) primary->assembledValid[p] = true;
  if (geometry) primary->assembledGeometryValid = true;
  return TWK_SUCCESS;
}

// The packed buffer of a plane on a handle whose streams are allocated
static const void* ownPlane(TwkDevice dev, int plane)
{
  switch (plane)
  {
    case TWK_PLANE_OUTPUT:        return ownOutput(dev);
    case TWK_PLANE_ALBEDO:        return dev->d_aovAlbedo;
    case TWK_PLANE_NORMAL:        return dev->d_aovNormal;
    case TWK_PLANE_MOMENTS:       return dev->d_moments;
    case TWK_PLANE_SAMPLE_COUNTS: return dev->d_sampleCounts;
    default:                      return dev->d_cascade;
  }
}

static bool sameCascade(const TwkCascade& a, const TwkCascade& b) { return a.layers == b.layers && asUint(a.start) == asUint(b.start) && asUint(a.base) == asUint(b.base); }

// twk_assemble (geometrySources unused, withGeometry false) and twk_assemble_with_geometry
static int assembleExplicit(const char* name, TwkDevice primary, unsigned int planeMask, const TwkAssemblySource* sources, const void* const* geometrySources, int deviceCount, bool withGeometry)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!primary) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  int rc = refusePrimary(name, primary, planeMask, withGeometry); if (rc) return rc;
  if (!sources && planeMask) return refuse(TWK_ERROR_INVALID_VALUE, "NULL sources");
  if (withGeometry && !geometrySources) return refuse(TWK_ERROR_INVALID_VALUE, "NULL geometry sources");
  if (deviceCount != primary->count) return refuse(TWK_ERROR_INVALID_VALUE, "deviceCount must be the primary handle's device count");
  for (int d = 0; d < deviceCount; ++d)
  {
    for (int p = 0; p < TWK_PLANE_COUNT; ++p)
      if (((planeMask >> p) & 1u) && !sources[d].plane[p]) return refuse(TWK_ERROR_INVALID_VALUE, std::string("NULL source of ") + kPlaneNames[p] + " for device " + std::to_string(d));
    if (withGeometry && !geometrySources[d]) return refuse(TWK_ERROR_INVALID_VALUE, "NULL geometry source for device " + std::to_string(d));
  }
  if ((rc = activate(primary, name))) return rc;
  std::vector<TwkAssemblySource> planes((size_t) deviceCount);
  if (planeMask) planes.assign(sources, sources + deviceCount);
  else memset(planes.data(), 0, planes.size() * sizeof(TwkAssemblySource));
  if (!withGeometry) return assembleLaunch(primary, planeMask, planes);
  const std::vector<const void*> geometry(geometrySources, geometrySources + deviceCount);
  return assembleLaunch(primary, planeMask, planes, &geometry);
}

// twk_assemble_devices (withGeometry false) and twk_assemble_devices_with_geometry
static int assembleDevices(const char* name, TwkDevice primary, unsigned int planeMask, const TwkDevice* devices, int count, bool withGeometry)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!primary) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  if (!devices || count < 1) return refuse(TWK_ERROR_INVALID_VALUE, "NULL devices");
  for (int i = 0; i < count; ++i) if (!devices[i]) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle among the devices");
  int rc = refusePrimary(name, primary, planeMask, withGeometry); if (rc) return rc;
  if (count != primary->count) return refuse(TWK_ERROR_INVALID_VALUE, "count must be the primary handle's device count");
  if (withGeometry && geometryDeformed(primary))
    return refuse(TWK_ERROR_INVALID_STATE, "a geometry is deformed (twk_update_geometry_vertices since the history's frame): the previous-position plane is not built on tiled frames; twk_temporal_reset first");
  std::vector<TwkDevice> byIndex((size_t) count, nullptr);
  for (int i = 0; i < count; ++i)
  {
    TwkDevice dev = devices[i];
    if (!dev->stateSet) return refuse(TWK_ERROR_INVALID_STATE, "twk_set_state first, on every handle");
    const TwkDeviceState& a = dev->state; const TwkDeviceState& b = primary->state;
    if (a.resolution[0] != b.resolution[0] || a.resolution[1] != b.resolution[1] || a.tileSize[0] != b.tileSize[0] || a.tileSize[1] != b.tileSize[1] ||
        a.distribution != b.distribution || dev->count != primary->count || dev->launchWidth != primary->launchWidth)
      return refuse(TWK_ERROR_INVALID_VALUE, "the handles disagree in resolution, tile size, distribution or device count");
    if (dev->outputFormat != primary->outputFormat) return refuse(TWK_ERROR_INVALID_VALUE, "the handles disagree in output format");
    if (((planeMask >> TWK_PLANE_CASCADE) & 1u) && dev->cascadeEnabled && !sameCascade(dev->cascadeParameters, primary->cascadeParameters))
      return refuse(TWK_ERROR_INVALID_VALUE, "the handles disagree in cascade parameters");
    if (dev->index < 0 || dev->index >= count || byIndex[(size_t) dev->index]) return refuse(TWK_ERROR_INVALID_VALUE, "the handles' indices must be each of 0..count-1 exactly once");
    byIndex[(size_t) dev->index] = dev;
    for (int p = 0; p < TWK_PLANE_COUNT; ++p)
      if ((planeMask >> p) & 1u)
        if (const char* off = planeSwitchOff(dev, p)) return refuse(TWK_ERROR_INVALID_STATE, std::string(kPlaneNames[p]) + " needs " + off + "(1) on every handle");
    if ((planeMask & TWK_PLANE_BIT(TWK_PLANE_OUTPUT)) && dev->d_outputExternal && dev->outputFrame)
      return refuse(TWK_ERROR_INVALID_STATE, "a handle renders into a shared frame (twk_set_shared_frame): its beauty is not a packed tile buffer");
    if (!withGeometry) continue;
    if (!dev->geometryEnabled) return refuse(TWK_ERROR_INVALID_STATE, "the geometry AOV needs twk_enable_geometry(1) on every handle");
    if (!dev->geometryValid || !dev->d_geometry)
      return refuse(TWK_ERROR_INVALID_STATE, "the geometry AOV of the handle with index " + std::to_string(dev->index) + " is older than its camera, state or scene: twk_render_geometry_tile first");
    if (dev->cameras.empty() || primary->cameras.empty() || memcmp(&dev->cameras[0], &primary->cameras[0], sizeof(TwkCameraDefinition)) != 0)
      return refuse(TWK_ERROR_INVALID_VALUE, "camera 0 of the handle with index " + std::to_string(dev->index) + " is not the primary handle's: the tile shares would be of different views");
    // twk_update_instance_transform is made on every handle by the caller: a share of a scene whose object is elsewhere is refused
    // (handles of the same instances only: what else they may differ in is as it was)
    if (dev->instances.size() == primary->instances.size())
      for (size_t i = 0; i < dev->instances.size(); ++i)
        if (memcmp(dev->instances[i].transform, primary->instances[i].transform, sizeof(float) * 12) != 0)
          return refuse(TWK_ERROR_INVALID_STATE, "instance " + std::to_string(i) + " of the handle with index " + std::to_string(dev->index) +
                                                 " is not where the primary handle has it: twk_update_instance_transform on every handle");
  }

  // every source: recorded launches rendered, buffers allocated, counts current, then an event on its stream
  for (TwkDevice dev : byIndex)
  {
    if ((rc = activate(dev, name))) return rc;
    if ((rc = ensureStreams(dev))) return rc;
    if ((planeMask & TWK_PLANE_BIT(TWK_PLANE_SAMPLE_COUNTS)) && (rc = currentSampleCounts(dev))) return rc;
    if (dev == primary) continue;
    if (!dev->assembleReady) HIP_TRY(hipEventCreateWithFlags(&dev->assembleReady, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(dev->assembleReady, dev->stream));
  }
  if ((rc = activate(primary, name))) return rc;
  for (TwkDevice dev : byIndex) if (dev != primary) HIP_TRY(hipStreamWaitEvent(primary->stream, dev->assembleReady, 0));

  // direct where primary's device can read the source, else (or when forced) through the staging block
  std::vector<char> staged((size_t) count, 0);
  size_t stageBytes = 0;
  const auto segment = [](size_t bytes) { return (bytes + 255) & ~(size_t) 255; };
  for (int d = 0; d < count; ++d)
  {
    TwkDevice dev = byIndex[(size_t) d];
    bool stage = primary->assembleStage;
    if (!stage && dev->ordinal != primary->ordinal)
    {
      int can = 0;
      HIP_TRY(hipDeviceCanAccessPeer(&can, primary->ordinal, dev->ordinal));
      if (can)
      {
        const hipError_t e = hipDeviceEnablePeerAccess(dev->ordinal, 0);
        if (e == hipErrorPeerAccessAlreadyEnabled) (void) hipGetLastError();
        else HIP_TRY(e);
      }
      else stage = true;
    }
    staged[(size_t) d] = stage ? 1 : 0;
    if (stage) for (int p = 0; p < TWK_PLANE_COUNT; ++p) if ((planeMask >> p) & 1u) stageBytes += segment(planeBytes(primary, p, primary->launchWidth));
    if (stage && withGeometry) stageBytes += segment(geometryBytes(primary, primary->launchWidth));
  }
  if (stageBytes > primary->d_assembleStage.capacity())
  {
    HIP_TRY(hipStreamSynchronize(primary->stream));
    if ((rc = primary->d_assembleStage.allocate(stageBytes))) return rc;
  }
  std::vector<TwkAssemblySource> sources((size_t) count);
  std::vector<const void*> geometry((size_t) count, nullptr);
  size_t offset = 0;
  for (int d = 0; d < count; ++d)
  {
    TwkDevice dev = byIndex[(size_t) d];
    for (int p = 0; p < TWK_PLANE_COUNT; ++p)
    {
      sources[(size_t) d].plane[p] = nullptr;
      if (!((planeMask >> p) & 1u)) continue;
      const void* own = ownPlane(dev, p);
      if (!own) return refuse(TWK_ERROR_INVALID_STATE, std::string(kPlaneNames[p]) + " has no buffer on device " + std::to_string(d));
      if (!staged[(size_t) d]) { sources[(size_t) d].plane[p] = own; continue; }
      const size_t bytes = planeBytes(primary, p, primary->launchWidth);
      char* to = static_cast<char*>(primary->d_assembleStage.get()) + offset;
      if (dev->ordinal == primary->ordinal) HIP_TRY(hipMemcpyAsync(to, own, bytes, hipMemcpyDeviceToDevice, primary->stream));
      else                                  HIP_TRY(hipMemcpyPeerAsync(to, primary->ordinal, own, dev->ordinal, bytes, primary->stream));
      sources[(size_t) d].plane[p] = to;
      offset += segment(bytes);
    }
    if (!withGeometry) continue;
    geometry[(size_t) d] = dev->d_geometry;
    if (!staged[(size_t) d]) continue;
    const size_t bytes = geometryBytes(primary, primary->launchWidth);
    char* to = static_cast<char*>(primary->d_assembleStage.get()) + offset;
    if (dev->ordinal == primary->ordinal) HIP_TRY(hipMemcpyAsync(to, dev->d_geometry, bytes, hipMemcpyDeviceToDevice, primary->stream));
    else                                  HIP_TRY(hipMemcpyPeerAsync(to, primary->ordinal, dev->d_geometry, dev->ordinal, bytes, primary->stream));
    geometry[(size_t) d] = to;
    offset += segment(bytes);
  }
  if ((rc = assembleLaunch(primary, planeMask, sources, withGeometry ? &geometry : nullptr))) return rc;

  // the sources render on only once their buffers have been read
  bool others = false;
  for (TwkDevice dev : byIndex) others = others || dev != primary;
  if (others)
  {
    if (!primary->assembleDone) HIP_TRY(hipEventCreateWithFlags(&primary->assembleDone, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(primary->assembleDone, primary->stream));
    for (TwkDevice dev : byIndex) if (dev != primary) HIP_TRY(hipStreamWaitEvent(dev->stream, primary->assembleDone, 0));
  }
  return TWK_SUCCESS;
}

extern "C" {

int twk_assemble(TwkDevice primary, unsigned int planeMask, const TwkAssemblySource* sources, int deviceCount)
try
{
  return assembleExplicit("twk_assemble", primary, planeMask, sources, nullptr, deviceCount, false);
}
TWK_CATCH("twk_assemble")

int twk_assemble_devices(TwkDevice primary, unsigned int planeMask, const TwkDevice* devices, int count)
try
{
  return assembleDevices("twk_assemble_devices", primary, planeMask, devices, count, false);
}
TWK_CATCH("twk_assemble_devices")

int twk_assemble_with_geometry(TwkDevice primary, unsigned int planeMask, const TwkAssemblySource* sources, const void* const* geometrySources, int deviceCount)
try
{
  return assembleExplicit("twk_assemble_with_geometry", primary, planeMask, sources, geometrySources, deviceCount, true);
}
TWK_CATCH("twk_assemble_with_geometry")

int twk_assemble_devices_with_geometry(TwkDevice primary, unsigned int planeMask, const TwkDevice* devices, int count)
try
{
  return assembleDevices("twk_assemble_devices_with_geometry", primary, planeMask, devices, count, true);
}
TWK_CATCH("twk_assemble_devices_with_geometry")

int twk_get_assembled_device_pointer(TwkDevice primary, int plane, void** dptr, size_t* bytes)
try
{
  const char* name = "twk_get_assembled_device_pointer";
  if (!primary) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL device handle");
  if (!dptr || plane < 0 || plane >= TWK_PLANE_COUNT) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument or unknown plane");
  if (!primary->assembledValid[plane] || !primary->d_assembled[plane])
    return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": " + kPlaneNames[plane] + " has not been assembled since the handle's frame last changed shape");
  *dptr = primary->d_assembled[plane];
  if (bytes) *bytes = primary->d_assembled[plane].capacity();
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_assembled_device_pointer")

int twk_read_assembled(TwkDevice primary, int plane, void* host, size_t bytes)
try
{
  const char* name = "twk_read_assembled";
  if (!primary) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL device handle");
  if (!host || plane < 0 || plane >= TWK_PLANE_COUNT) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL buffer or unknown plane");
  if (!primary->assembledValid[plane] || !primary->d_assembled[plane])
    return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": " + kPlaneNames[plane] + " has not been assembled since the handle's frame last changed shape");
  if (bytes != primary->d_assembled[plane].capacity()) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": buffer must hold the assembled plane, " + std::to_string(primary->d_assembled[plane].capacity()) + " bytes");
  int rc = activate(primary, name); if (rc) return rc;
  return copyBack(primary, name, primary->d_assembled[plane], bytes, 1, host);
}
TWK_CATCH("twk_read_assembled")

int twk_get_assembled_geometry_device_pointer(TwkDevice primary, void** dptr, size_t* bytes)
try
{
  const char* name = "twk_get_assembled_geometry_device_pointer";
  if (!primary) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL device handle");
  if (!dptr) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  if (!primary->assembledGeometryValid || !primary->d_assembledGeometry)
    return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": the geometry AOV has not been assembled since the handle's frame last changed shape or its camera, state or scene changed");
  *dptr = primary->d_assembledGeometry;
  if (bytes) *bytes = primary->d_assembledGeometry.capacity();
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_assembled_geometry_device_pointer")

int twk_read_assembled_geometry(TwkDevice primary, float* host, size_t numFloats)
try
{
  const char* name = "twk_read_assembled_geometry";
  if (!primary) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL device handle");
  if (!host) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL buffer");
  if (!primary->assembledGeometryValid || !primary->d_assembledGeometry)
    return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": the geometry AOV has not been assembled since the handle's frame last changed shape or its camera, state or scene changed");
  if (numFloats * sizeof(float) != primary->d_assembledGeometry.capacity()) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": buffer must hold width*height*4 floats");
  int rc = activate(primary, name); if (rc) return rc;
  return copyBack(primary, name, primary->d_assembledGeometry, primary->d_assembledGeometry.capacity(), 1, host);
}
TWK_CATCH("twk_read_assembled_geometry")

int twk_assemble_host(const void* const* sources, int deviceCount, int width, int height, const int tileSize[2], int elementBytes, int layers, void* destination)
try
{
  const char* name = "twk_assemble_host";
  if (!sources || !tileSize || !destination) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  if (deviceCount < 1 || width < 1 || height < 1 || layers < 1) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": deviceCount, width, height and layers must be >= 1");
  if (tileSize[0] < 1 || tileSize[1] < 1 || (tileSize[0] & (tileSize[0] - 1)) || (tileSize[1] & (tileSize[1] - 1)))
    return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": tile size must be a power of two");
  if (elementBytes != 4 && elementBytes != 8 && elementBytes != 16) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": elementBytes must be 4, 8 or 16");
  for (int d = 0; d < deviceCount; ++d) if (!sources[d]) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL source");
  AssembleShape s;
  s.width = width; s.height = height; s.deviceCount = deviceCount; s.tileSizeX = tileSize[0];
  s.tileShiftX = calculateShift(tileSize[0]); s.tileShiftY = calculateShift(tileSize[1]);
  s.launchWidth = assembleLaunchWidth(width, tileSize[0], deviceCount);
  const unsigned int shift = (elementBytes == 4) ? 2u : ((elementBytes == 8) ? 3u : 4u);
  const size_t sourceLayer = (size_t) s.launchWidth * height, assembledLayer = (size_t) width * height;
  for (int d = 0; d < deviceCount; ++d)
    for (int layer = 0; layer < layers; ++layer)
    {
      // one entry of the kernel's table, moved group by group as assembleKernel's lanes do
      const char* source = static_cast<const char*>(sources[d]) + (((size_t) layer * sourceLayer) << shift);
      char* to = static_cast<char*>(destination) + (((size_t) layer * assembledLayer) << shift);
      const unsigned int groupShift = assembleGroupShift(s, shift, source, to);
      const size_t groupBytes = (size_t) 1 << (shift + groupShift);
      for (unsigned int y = 0; y < (unsigned int) height; ++y)
        for (unsigned int group = 0; group < ((unsigned int) s.launchWidth >> groupShift); ++group)
        {
          const unsigned int xLaunch = group << groupShift;
          const unsigned int x = assembleColumn(s, (unsigned int) d, xLaunch, y);
          if (x >= (unsigned int) width) continue;
          memcpy(to + (((size_t) y * width + x) << shift), source + (((size_t) y * s.launchWidth + xLaunch) << shift), groupBytes);
        }
    }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_assemble_host")

} // extern "C"
