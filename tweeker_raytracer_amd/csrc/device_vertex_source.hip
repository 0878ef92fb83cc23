// A device-pointer source for a geometry's vertices behind the C ABI (vertex_source_device.h: the definition): the refusals, the
// read-only check launch, the ingest into the geometry's slice of d_attributes, the host mirror that goes stale and is refreshed for
// its readers, the host form of the frames and the read-back of a geometry's current records. The two entry points are in
// device_scene.hip, beside the host calls: after ingestVertexSource they run updateSelective and buildScene as they are.
#include "device_handle.h"
#include "vertex_source_device.h"

#include <cstring>
#include <vector>

// The mirror of geometry idGeometry as the device holds it: one device-to-host copy of its slice when a device-pointer source has
// written it since the mirror was last whole, nothing otherwise. Every reader of GeometryHost::attributes calls it first.
int twk::refreshMirror(TwkDevice dev, int idGeometry)
{
  GeometryHost& g = dev->geometries[idGeometry];
  if (!mirrorStale(g)) return TWK_SUCCESS;
  if (!dev->d_attributes.holds(12 * ((size_t) g.attributeBase + g.attributes.size())))
    return twkSetError(TWK_ERROR_INVALID_STATE, "geometry " + std::to_string(idGeometry) + ": its vertices came from a device-pointer source and the attribute array is gone");
  HIP_TRY(hipMemcpyAsync(g.attributes.data(), dev->d_attributes + 12 * (size_t) g.attributeBase, sizeof(TwkTriangleAttributes) * g.attributes.size(), hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  g.device->mirrorStale = false;
  return TWK_SUCCESS;
}

// Whether [pointer, pointer + bytes) is device or managed memory this handle's device can read; never dereferenced. A pointer the
// runtime does not know leaves a sticky error behind, which is cleared.
static bool deviceReadable(TwkDevice dev, const void* pointer, size_t bytes, std::string& why)
{
  hipPointerAttribute_t attributes;
  memset(&attributes, 0, sizeof(attributes));
  const hipError_t e = hipPointerGetAttributes(&attributes, pointer);
  (void) hipGetLastError();
  if (e != hipSuccess || (attributes.type != hipMemoryTypeDevice && attributes.type != hipMemoryTypeManaged)) { why = "not device or managed memory (a host pointer is the host call's)"; return false; }
  if (attributes.type == hipMemoryTypeDevice && attributes.device != dev->ordinal)
  {
    int can = 0;
    const hipError_t peer = hipDeviceCanAccessPeer(&can, dev->ordinal, attributes.device);
    (void) hipGetLastError();
    if (peer != hipSuccess || !can) { why = "memory of device " + std::to_string(attributes.device) + ", which the handle's device " + std::to_string(dev->ordinal) + " cannot read"; return false; }
  }
  // the bytes the launches read lie inside the allocation, where the runtime can say what that is
  hipDeviceptr_t base = nullptr; size_t size = 0;
  const hipError_t range = hipMemGetAddressRange(&base, &size, const_cast<void*>(pointer));
  (void) hipGetLastError();
  if (range == hipSuccess && base != nullptr && (uintptr_t) pointer + bytes > (uintptr_t) base + size)
  { why = "the allocation ends " + std::to_string((uintptr_t) pointer + bytes - ((uintptr_t) base + size)) + " bytes before the last vertex"; return false; }
  return true;
}

// The adjacency table of the frames, built from the geometry's indices and uploaded at the first call that needs it
static int ensureAdjacency(TwkDevice dev, GeometryHost& g)
{
  GeometryDevice& d = *g.device;
  if (d.d_adjacencyOffsets.holds(g.attributes.size() + 1) && d.d_adjacencyTriangles != nullptr) return TWK_SUCCESS;
  std::vector<unsigned int> offsets, triangles;
  vertexAdjacency(g.indices.data(), g.indices.size(), g.attributes.size(), offsets, triangles);
  int rc;
  if ((rc = d.d_adjacencyOffsets.allocate(offsets.size())) || (rc = d.d_adjacencyTriangles.allocate(std::max<size_t>(1, triangles.size())))) { d.d_adjacencyOffsets.release(); return rc; }
  HIP_TRY(hipMemcpyAsync(d.d_adjacencyOffsets, offsets.data(), sizeof(unsigned int) * offsets.size(), hipMemcpyHostToDevice, dev->stream));
  if (!triangles.empty()) HIP_TRY(hipMemcpyAsync(d.d_adjacencyTriangles, triangles.data(), sizeof(unsigned int) * triangles.size(), hipMemcpyHostToDevice, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream)); // the two vectors go away
  return TWK_SUCCESS;
}

// A geometry's device-pointer source, refused with the texts of twk_update_geometry_vertices_device behind `where` (the call's name,
// and its entry in twk_refit_scene): the vertex update's refusals, then the source's own. Reads nothing of the source. view: what the
// launches are given.
int twk::checkVertexSource(TwkDevice dev, const std::string& where, int idGeometry, const TwkVertexSource* source, size_t numVertices, VertexSourceView& view)
{
  const auto refuse = [&where](int code, const std::string& text) { return twkSetError(code, where + text); };
  if (idGeometry < 0 || idGeometry >= (int) dev->geometries.size()) return refuse(TWK_ERROR_INVALID_VALUE, "bad geometry id");
  GeometryHost& g = dev->geometries[idGeometry];
  const size_t n = g.attributes.size();
  if (numVertices != n)
    return refuse(TWK_ERROR_INVALID_VALUE, "the geometry has " + std::to_string(n) + " vertices, not " + std::to_string(numVertices) + " (the indices stay: no topology change)");
  if ((source->attributes != nullptr) == (source->positions != nullptr)) return refuse(TWK_ERROR_INVALID_VALUE, "the source sets exactly one of attributes and positions");
  if (source->reserved[0] || source->reserved[1] || source->reserved[2]) return refuse(TWK_ERROR_INVALID_VALUE, "a reserved word of the source is not 0");
  const bool records = source->attributes != nullptr;
  if (source->recomputeFrames > 1u || (records && source->recomputeFrames)) return refuse(TWK_ERROR_INVALID_VALUE, "recomputeFrames is 0 or 1, and 1 with positions only");
  if (records && source->positionStride != 0) return refuse(TWK_ERROR_INVALID_VALUE, "positionStride goes with positions (records are 48 bytes apart)");
  const size_t stride = records ? sizeof(TwkTriangleAttributes) : (source->positionStride ? source->positionStride : 12);
  if (stride < 12 || (stride % 4) != 0) return refuse(TWK_ERROR_INVALID_VALUE, "positionStride " + std::to_string(stride) + " is below 12 or no multiple of 4");
  const void* pointer = records ? source->attributes : source->positions;
  if ((uintptr_t) pointer % (records ? 16 : 4) != 0) return refuse(TWK_ERROR_INVALID_VALUE, records ? "attributes are not 16-byte aligned" : "positions are not 4-byte aligned");
  const size_t bytes = (n - 1) * stride + (records ? sizeof(TwkTriangleAttributes) : 12);
  std::string why;
  if (!deviceReadable(dev, pointer, bytes, why)) return refuse(TWK_ERROR_INVALID_VALUE, std::string(records ? "attributes: " : "positions: ") + why);
  if (!dev->d_attributes.holds(12 * ((size_t) g.attributeBase + n))) return refuse(TWK_ERROR_INVALID_STATE, "the built scene holds no attribute array");
  if (overlaps(pointer, bytes, dev->d_attributes.get(), sizeof(float) * dev->d_attributes.capacity())) return refuse(TWK_ERROR_INVALID_VALUE, "the source overlaps the handle's own attribute array");
  for (size_t i = 0; i < dev->instances.size(); ++i)
    if (dev->instances[i].geometry == idGeometry && dev->instances[i].light >= 0)
      return refuse(TWK_ERROR_INVALID_VALUE, "instance " + std::to_string(i) + " of the geometry carries a light (idLight >= 0): its light definition holds the emitter's shape and would disagree; deforming emitters is not supported");
  view.pointer = pointer; view.stride = stride; view.records = records; view.recompute = source->recomputeFrames != 0;
  return TWK_SUCCESS;
}

// ... and, once the source has passed its check launch, the ingest into the geometry's slice on the handle's stream
int twk::storeVertexSource(TwkDevice dev, int idGeometry, const VertexSourceView& view)
{
  int rc;
  GeometryHost& g = dev->geometries[idGeometry];
  const size_t n = g.attributes.size();
  float* slice = dev->d_attributes + 12 * (size_t) g.attributeBase;
  if (!g.device) g.device.reset(new GeometryDevice());
  if (!view.records && view.recompute && (rc = ensureAdjacency(dev, g))) return rc;
  // keepPreviousPositions' rule, with the content on the device: the vector gets its size (what says "deformed"), the kernel the array
  const bool keep = dev->temporalHasHistory && ((size_t) idGeometry >= dev->previousPositions.size() || dev->previousPositions[idGeometry].empty());
  if (keep && (rc = g.device->d_kept.ensure(n))) return rc;
  // nothing was changed up to here: a refused call changes nothing
  if (keep)
  {
    dev->previousPositions.resize(dev->geometries.size()); dev->previousOnDevice.resize(dev->geometries.size(), 0);
    dev->previousPositions[idGeometry].assign(n, make_float4(0.0f, 0.0f, 0.0f, 0.0f)); dev->previousOnDevice[idGeometry] = 1;
    dev->previousPositionsUploaded = false;
  }
  float4* kept = keep ? g.device->d_kept.get() : nullptr;
  if (view.records) launchIngestAttributes(static_cast<const float4*>(view.pointer), reinterpret_cast<float4*>(slice), kept, (unsigned int) n, dev->stream);
  else launchIngestPositions(view.pointer, view.stride, view.recompute, dev->d_indices + g.indexBase, g.device->d_adjacencyOffsets, g.device->d_adjacencyTriangles,
                             reinterpret_cast<float4*>(slice), kept, (unsigned int) n, dev->stream);
  g.device->mirrorStale = true; // before the launch is known to have been taken: a slice half written is not the mirror's either
  dev->updateInfoValid = false;
  HIP_TRY(hipGetLastError());
  return TWK_SUCCESS;
}

// The front half of twk_update_geometry_vertices_device and of twk_refit_geometry_vertices_device: replaceVertices' refusals under
// the caller's name, the source's own, the check launch — nothing was changed up to there — then the ingest on the handle's stream.
int twk::ingestVertexSource(TwkDevice dev, const char* name, bool refit, int idGeometry, const TwkVertexSource* source, size_t numVertices)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  if (!source) return refuse(TWK_ERROR_INVALID_VALUE, "NULL source");
  int rc = activate(dev, name); if (rc) return rc;
  if (!dev->built) return refuse(TWK_ERROR_INVALID_STATE, "twk_build has not been called");
  if (refit && !dev->kept.valid)
    return refuse(TWK_ERROR_INVALID_STATE, "the scene was not built in TWK_UPDATE_SELECTIVE (twk_set_update_mode before twk_build): nothing a refit needs was kept");
  VertexSourceView view;
  if ((rc = checkVertexSource(dev, std::string(name) + ": ", idGeometry, source, numVertices, view))) return rc;

  // the check launch: read-only, and read before anything is written. The host call can look before it writes; this one cannot.
  if ((rc = dev->d_sourceCheck.ensure(1))) return rc;
  unsigned int lowest = 0xffffffffu;
  HIP_TRY(hipMemsetAsync(dev->d_sourceCheck, 0xff, sizeof(unsigned int), dev->stream));
  launchVertexSourceCheck(view.pointer, view.stride, (unsigned int) numVertices, dev->d_sourceCheck, dev->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&lowest, dev->d_sourceCheck, sizeof(unsigned int), hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if (lowest != 0xffffffffu) return refuse(TWK_ERROR_INVALID_VALUE, "vertex " + std::to_string(lowest) + ": the position is not finite");
  return storeVertexSource(dev, idGeometry, view);
}

extern "C" {

int twk_vertex_frames_host(const float* positions, size_t numVertices, const unsigned int* indices, size_t numIndices, const TwkTriangleAttributes* before, TwkTriangleAttributes* after)
try
{
  const auto refuse = [](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_vertex_frames_host: " + text); };
  if (!positions || !indices || !before || !after) return refuse("NULL argument");
  if (numVertices < 1 || numVertices >= ((size_t) 1 << 32)) return refuse("numVertices must be in 1..2^32 - 1");
  if (numIndices < 3 || (numIndices % 3) != 0) return refuse("numIndices is " + std::to_string(numIndices) + ", not a non-empty multiple of three");
  for (size_t i = 0; i < numIndices; ++i) if (indices[i] >= numVertices) return refuse("index " + std::to_string(i) + " is beyond the vertices");
  std::vector<float> out(12 * numVertices); // `after` may be `before`
  vertexFramesHost(positions, numVertices, indices, numIndices, reinterpret_cast<const float*>(before), out.data());
  memcpy(after, out.data(), sizeof(float) * out.size());
  return TWK_SUCCESS;
}
TWK_CATCH("twk_vertex_frames_host")

int twk_read_geometry_vertices(TwkDevice dev, int idGeometry, TwkTriangleAttributes* out, size_t capacity)
try
{
  const char* name = "twk_read_geometry_vertices";
  const auto refuse = [name](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!dev) return refuse("NULL device handle");
  if (!out) return refuse("NULL array");
  int rc = activate(dev, name); if (rc) return rc;
  if (idGeometry < 0 || idGeometry >= (int) dev->geometries.size()) return refuse("bad geometry id");
  const GeometryHost& g = dev->geometries[idGeometry];
  if (capacity < g.attributes.size()) return refuse("the geometry has " + std::to_string(g.attributes.size()) + " vertices, the array room for " + std::to_string(capacity));
  if ((rc = refreshMirror(dev, idGeometry))) return rc;
  memcpy(out, g.attributes.data(), sizeof(TwkTriangleAttributes) * g.attributes.size());
  return TWK_SUCCESS;
}
TWK_CATCH("twk_read_geometry_vertices")

} // extern "C"
