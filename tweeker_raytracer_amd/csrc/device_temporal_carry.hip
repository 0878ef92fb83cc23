// Per-vertex motion behind the C ABI (temporal_carry_device.h: the definition): the previous positions a vertex update keeps,
// twk_render_geometry_motion with the previous-position plane, its readers and its host form.
#include "device_handle.h"
#include "temporal_carry_device.h"

#include <cstring>
#include <vector>

// No geometry is deformed any more and the plane describes a history that was. release: the device arrays go too (everything
// enqueued has run: the callers of dropTemporal wait first); else they stay for the next plane.
void twk::dropPreviousPositions(TwkDevice dev, bool release)
{
  dev->previousPositions.clear(); dev->previousOnDevice.clear(); dev->previousPlaneValid = false; dev->previousPositionsUploaded = false;
  if (release) { dev->carryMotionUploaded.clear(); dev->carryUploaded.clear(); }
  if (release) { dev->d_previousPositions.release(); dev->d_previousPlane.release(); dev->d_carryMotion.release(); dev->d_carry.release(); }
}

// Before the vertices of geometry idGeometry are replaced: with a history, and unless an earlier update since the history's frame has
// kept them already (several updates between two merges keep the oldest), its positions are kept. Without a history nothing is.
void twk::keepPreviousPositions(TwkDevice dev, int idGeometry)
{
  if (!dev->temporalHasHistory) return;
  dev->previousPositions.resize(dev->geometries.size());
  std::vector<float4>& kept = dev->previousPositions[idGeometry];
  if (!kept.empty()) return;
  const std::vector<TwkTriangleAttributes>& attributes = dev->geometries[idGeometry].attributes;
  kept.resize(attributes.size());
  dev->previousPositionsUploaded = false;
  for (size_t v = 0; v < attributes.size(); ++v) kept[v] = make_float4(attributes[v].vertex[0], attributes[v].vertex[1], attributes[v].vertex[2], 0.0f);
}

static const char* const noPlane = "no twk_render_geometry_motion since the last change of camera, state, scene or history";

extern "C" {

int twk_render_geometry_motion(TwkDevice dev)
try
{
  const char* name = "twk_render_geometry_motion";
  const auto refuse = [name](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": " + text); };
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL device handle");
  int rc = activate(dev, name); if (rc) return rc;
  // twk_render_geometry's refusals, with its texts
  if (!dev->built) return refuse("twk_build has not been called");
  if (!dev->stateSet || dev->cameras.empty()) return refuse("twk_set_state and twk_init_cameras first");
  if (!dev->geometryEnabled) return refuse("twk_enable_geometry(1) first");
  if (dev->state.lensShader != 0) return refuse("pinhole lens shader only (reprojection inverts the pinhole mapping)");
  if (dev->state.distribution && 1 < dev->count) return refuse("the handle's buffers are packed tile buffers (distribution 1, more than one device), not pictures");
  for (const DevMaterial& m : dev->materials) if (m.textureCutout) return refuse("geometric query only, not for scenes with cutout opacity");
  if ((rc = ensureStreams(dev))) return rc;
  refreshParams(dev);
  const size_t numPixels = launchIndices(dev);
  if (!ownGeometry(dev, numPixels)) return refuse("no geometry buffer");

  // the two records per instance and the packed previous positions, as the history and the scene stand now
  const size_t count = dev->instances.size();
  const bool snapshot = dev->temporalHasHistory && dev->temporalTransforms.size() == 12 * count;
  // (the positions themselves are packed further below, and only when the device does not hold them: the bases need their counts alone)
  std::vector<size_t> positionBase(dev->geometries.size(), 0);
  size_t numPositions = 0;
  for (size_t k = 0; k < dev->previousPositions.size() && k < dev->geometries.size(); ++k)
  {
    positionBase[k] = numPositions;
    numPositions += dev->previousPositions[k].size();
  }
  if (numPositions >= ((size_t) 1 << 32)) return refuse("more than 2^32 - 1 previous positions");
  std::vector<TwkInstanceMotion> motion(count);
  std::vector<TwkInstanceCarry> carry(count);
  for (size_t i = 0; i < count; ++i)
  {
    const InstanceHost& inst = dev->instances[i];
    const float* current = inst.transform;
    const float* previous = snapshot ? &dev->temporalTransforms[12 * i] : current;
    memset(&motion[i], 0, sizeof(TwkInstanceMotion)); memset(&carry[i], 0, sizeof(TwkInstanceCarry));
    if (memcmp(previous, current, 12 * sizeof(float)) == 0) motion[i].previousFromCurrent[0] = motion[i].previousFromCurrent[5] = motion[i].previousFromCurrent[10] = 1.0f;
    else if (!instanceMotion(previous, current, motion[i]))
      return refuse("instance " + std::to_string(i) + " has moved and its transform, now or in the history's frame, is singular or not finite");
    memcpy(carry[i].previousObjectToWorld, previous, 12 * sizeof(float));
    const bool deformed = (size_t) inst.geometry < dev->previousPositions.size() && !dev->previousPositions[inst.geometry].empty();
    carry[i].deformed = deformed ? 1u : 0u;
    carry[i].positionBase = deformed ? (unsigned int) positionBase[inst.geometry] : 0u;
    carry[i].indexBase = dev->geometries[inst.geometry].indexBase;
  }
  if ((rc = growIdle(dev, dev->d_previousPlane, numPixels))) return rc;
  // the uploads, and the wait for them, only when a table or the previous positions differ from what the device holds: a viewer that
  // calls this every frame uploads after an update and is asynchronous otherwise
  const bool sameTables = dev->d_carryMotion.holds(count) && dev->d_carry.holds(count) && dev->carryMotionUploaded.size() == count && dev->carryUploaded.size() == count &&
                          memcmp(dev->carryMotionUploaded.data(), motion.data(), count * sizeof(TwkInstanceMotion)) == 0 &&
                          memcmp(dev->carryUploaded.data(), carry.data(), count * sizeof(TwkInstanceCarry)) == 0;
  const bool samePositions = dev->previousPositionsUploaded && dev->d_previousPositions.holds(std::max<size_t>(1, numPositions));
  if (!sameTables || !samePositions)
  {
    std::vector<float4> positions; // packed in geometry order, as the bases say
    // a geometry whose previous positions a device-pointer source kept (vertex_source_device.h) holds them on the device: it is
    // packed by a device-to-device copy at its base, and the host vectors of the others are uploaded one by one
    bool onDevice = false;
    for (size_t k = 0; k < dev->previousOnDevice.size() && k < dev->previousPositions.size(); ++k) onDevice = onDevice || (dev->previousOnDevice[k] && !dev->previousPositions[k].empty());
    if (!samePositions && !onDevice)
    {
      positions.reserve(numPositions);
      for (size_t k = 0; k < dev->previousPositions.size() && k < dev->geometries.size(); ++k) positions.insert(positions.end(), dev->previousPositions[k].begin(), dev->previousPositions[k].end());
    }
    dev->carryMotionUploaded.clear(); dev->carryUploaded.clear(); dev->previousPositionsUploaded = false; // until the uploads below have succeeded
    if ((rc = growIdle(dev, dev->d_carryMotion, count)) || (rc = growIdle(dev, dev->d_carry, count)) ||
        (rc = growIdle(dev, dev->d_previousPositions, std::max<size_t>(1, numPositions)))) return rc;
    HIP_TRY(hipMemcpyAsync(dev->d_carryMotion, motion.data(), count * sizeof(TwkInstanceMotion), hipMemcpyHostToDevice, dev->stream));
    HIP_TRY(hipMemcpyAsync(dev->d_carry, carry.data(), count * sizeof(TwkInstanceCarry), hipMemcpyHostToDevice, dev->stream));
    if (!positions.empty()) HIP_TRY(hipMemcpyAsync(dev->d_previousPositions, positions.data(), positions.size() * sizeof(float4), hipMemcpyHostToDevice, dev->stream));
    if (!samePositions && onDevice)
      for (size_t k = 0; k < dev->previousPositions.size() && k < dev->geometries.size(); ++k)
      {
        const std::vector<float4>& kept = dev->previousPositions[k];
        if (kept.empty()) continue;
        const bool device = k < dev->previousOnDevice.size() && dev->previousOnDevice[k] != 0;
        if (device && !(dev->geometries[k].device && dev->geometries[k].device->d_kept.holds(kept.size()))) return refuse("geometry " + std::to_string(k) + ": its kept previous positions are gone");
        HIP_TRY(hipMemcpyAsync(dev->d_previousPositions + positionBase[k], device ? (const void*) dev->geometries[k].device->d_kept.get() : (const void*) kept.data(), kept.size() * sizeof(float4),
                               device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, dev->stream));
      }
    HIP_TRY(hipStreamSynchronize(dev->stream)); // (the tables are pageable host memory that goes out of use here)
    dev->carryMotionUploaded = motion; dev->carryUploaded = carry; dev->previousPositionsUploaded = true;
  }

  int grid = (int) ((numPixels + TWK_TRACE_BLOCK - 1) / TWK_TRACE_BLOCK);
  if (grid > dev->numCUs * TWK_TRACE_WAVES) grid = dev->numCUs * TWK_TRACE_WAVES; // within the per-lane spill stacks, like twk_render_geometry
  launchGeometryMotion(dev->params, dev->d_geometry, dev->d_previousPlane, dev->d_carryMotion, (unsigned int) count, dev->d_carry, (unsigned int) count, dev->d_previousPositions, grid, dev->stream);
  HIP_TRY(hipGetLastError());
  dev->geometryValid = true; dev->previousPlaneValid = true;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_render_geometry_motion")

int twk_get_previous_position_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_previous_position_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!dev->previousPlaneValid || !dev->d_previousPlane.holds(launchIndices(dev))) return twkSetError(TWK_ERROR_INVALID_STATE, std::string("twk_get_previous_position_device_pointer: ") + noPlane);
    pointer = dev->d_previousPlane.get(); size = launchIndices(dev) * sizeof(float4);
    return (int) TWK_SUCCESS;
  });
}
TWK_CATCH("twk_get_previous_position_device_pointer")

int twk_read_previous_positions(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_previous_positions"); if (rc) return rc;
  const size_t n = launchIndices(dev);
  const float4* plane = (dev->previousPlaneValid && dev->d_previousPlane.holds(n)) ? dev->d_previousPlane.get() : nullptr;
  return readBack(dev, "twk_read_previous_positions", {plane, noPlane, n, sizeof(float4), false}, host, numFloats, 4, "width*height*4 floats");
}
TWK_CATCH("twk_read_previous_positions")

int twk_get_geometry_deformed(TwkDevice dev, int idGeometry, int* deformed)
try
{
  const char* name = "twk_get_geometry_deformed";
  if (!dev || !deformed) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  if (idGeometry < 0 || idGeometry >= (int) dev->geometries.size()) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": bad geometry id");
  *deformed = ((size_t) idGeometry < dev->previousPositions.size() && !dev->previousPositions[idGeometry].empty()) ? 1 : 0;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_geometry_deformed")

int twk_previous_positions_host(const float* hits, const int* instance, const int* primitive, const float* geometry, size_t numPixels, const unsigned int* indices, size_t numIndices,
                                const float* previousPositions, size_t numPositions, const TwkInstanceMotion* motion, int numMotion, const TwkInstanceCarry* carry, int numCarry, float* plane)
try
{
  const char* name = "twk_previous_positions_host";
  const auto refuse = [name](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!hits || !instance || !primitive || !geometry || !plane) return refuse("NULL argument");
  if (numPixels < 1 || numPixels > ((size_t) 1 << 28)) return refuse("numPixels must be in 1..2^28");
  if (numMotion < 0 || numCarry < 0 || (numMotion > 0 && !motion) || (numCarry > 0 && !carry)) return refuse("a negative count, or a count without its records");
  if ((numIndices > 0 && !indices) || (numPositions > 0 && !previousPositions)) return refuse("a count without its array");
  // every read of a deformed hit lies inside the arrays given
  for (size_t p = 0; p < numPixels; ++p)
  {
    if (instance[p] < 0 || instance[p] >= numCarry || carry[instance[p]].deformed == 0u) continue;
    const TwkInstanceCarry& c = carry[instance[p]];
    if (primitive[p] < 0 || (size_t) c.indexBase + 3 * (size_t) primitive[p] + 3 > numIndices) return refuse("pixel " + std::to_string(p) + ": the primitive's indices lie beyond numIndices");
    for (int j = 0; j < 3; ++j)
      if ((size_t) c.positionBase + indices[(size_t) c.indexBase + 3 * (size_t) primitive[p] + j] >= numPositions) return refuse("pixel " + std::to_string(p) + ": a vertex lies beyond numPositions");
  }
  previousPositionsHost(hits, instance, primitive, geometry, numPixels, indices, previousPositions, numPositions, motion, (unsigned int) numMotion, carry, (unsigned int) numCarry, plane);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_previous_positions_host")

} // extern "C"
