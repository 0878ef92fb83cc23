// Scene assembly and the acceleration-structure build behind the C ABI (≙ Device::createGeometry / createInstance / createTLAS,
// reference apps/rtigo3/src/Device.cpp:1339-1500).
#include "device_handle.h"
#include "temporal_motion_device.h" // instanceTransformUsable
#include "bvh_refit.h"              // the host form of a tree's refit
#include "vertex_source_device.h"   // the finite check of twk_refit_scene's device sources

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

// Inverse of a row-major 3x4 affine matrix in double, rounded once (OptiX derives the same matrix for
// optixGetInstanceInverseTransformFromHandle, closesthit.cu:49-52).
static void invertAffine(const float m[12], float inv[12])
{
  const double a00 = m[0], a01 = m[1], a02 = m[2],  t0 = m[3];
  const double a10 = m[4], a11 = m[5], a12 = m[6],  t1 = m[7];
  const double a20 = m[8], a21 = m[9], a22 = m[10], t2 = m[11];
  const double c00 = a11 * a22 - a12 * a21;
  const double c01 = a12 * a20 - a10 * a22;
  const double c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double r = 1.0 / det;
  const double i00 = c00 * r, i01 = (a02 * a21 - a01 * a22) * r, i02 = (a01 * a12 - a02 * a11) * r;
  const double i10 = c01 * r, i11 = (a00 * a22 - a02 * a20) * r, i12 = (a02 * a10 - a00 * a12) * r;
  const double i20 = c02 * r, i21 = (a01 * a20 - a00 * a21) * r, i22 = (a00 * a11 - a01 * a10) * r;
  inv[0] = (float) i00; inv[1] = (float) i01; inv[2]  = (float) i02; inv[3]  = (float) -(i00 * t0 + i01 * t1 + i02 * t2);
  inv[4] = (float) i10; inv[5] = (float) i11; inv[6]  = (float) i12; inv[7]  = (float) -(i10 * t0 + i11 * t1 + i12 * t2);
  inv[8] = (float) i20; inv[9] = (float) i21; inv[10] = (float) i22; inv[11] = (float) -(i20 * t0 + i21 * t1 + i22 * t2);
}

// =============================================================================================
extern "C" {

int twk_clear_scene(TwkDevice dev)
try
{
  int rc = activate(dev, "twk_clear_scene"); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->geometries.clear(); dev->instances.clear(); dev->built = false; dropAdaptive(dev);
  staleGeometry(dev); dropTemporal(dev); dropLightAnchors(dev);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_clear_scene")

int twk_add_geometry(TwkDevice dev, const TwkTriangleAttributes* attributes, size_t numAttributes,
                     const unsigned int* indices, size_t numIndices, int* idGeometry)
try
{
  int rc = activate(dev, "twk_add_geometry"); if (rc) return rc;
  if (!attributes || !indices || numAttributes == 0 || numIndices == 0 || (numIndices % 3) != 0)
    return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_add_geometry: need attributes and a non-empty multiple of three indices");
  // a leaf reference holds a 28-bit triangle slot (device_types.h BvhNode): refuse here what twk_build could not address
  if (numIndices / 3 >= ((size_t) 1 << 28) || numAttributes >= ((size_t) 1 << 32))
    return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_add_geometry: more than 2^28 - 1 triangles (or 2^32 - 1 vertices) in one geometry");
  for (size_t i = 0; i < numIndices; ++i)
    if (indices[i] >= numAttributes) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_add_geometry: index out of range");
  GeometryHost g;
  g.attributes.assign(attributes, attributes + numAttributes);
  g.indices.assign(indices, indices + numIndices);
  g.numTriangles = (int) (numIndices / 3);
  dev->geometries.push_back(std::move(g));
  dev->built = false;
  if (idGeometry) *idGeometry = (int) dev->geometries.size() - 1;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_add_geometry")

int twk_add_instance(TwkDevice dev, int idGeometry, const float transform[12], int idMaterial, int idLight, int* idInstance)
try
{
  int rc = activate(dev, "twk_add_instance"); if (rc) return rc;
  if (!transform || idGeometry < 0 || idGeometry >= (int) dev->geometries.size()) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_add_instance: bad geometry id");
  if (idMaterial < 0) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_add_instance: an instance needs a material (Device.cpp:1429)");
  InstanceHost inst;
  inst.geometry = idGeometry; inst.material = idMaterial; inst.light = idLight;
  memcpy(inst.transform, transform, sizeof(float) * 12);
  dev->instances.push_back(inst);
  dev->built = false;
  if (idInstance) *idInstance = (int) dev->instances.size() - 1;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_add_instance")

int twk_set_flatten_policy(TwkDevice dev, int maxTriangles, int maxReferences)
try
{
  int rc = activate(dev, "twk_set_flatten_policy"); if (rc) return rc;
  if (maxTriangles < 0 || maxReferences < 0) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_flatten_policy: limits must be >= 0");
  dev->flattenMaxTriangles = maxTriangles; dev->flattenMaxReferences = maxReferences;
  dev->built = false;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_set_flatten_policy")

int twk_set_build_quality(TwkDevice dev, int quality)
try
{
  int rc = activate(dev, "twk_set_build_quality"); if (rc) return rc;
  if (quality != TWK_BUILD_LBVH && quality != TWK_BUILD_SAH) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_build_quality: unknown quality");
  dev->builder.setQuality(quality);
  dev->built = false;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_set_build_quality")

int twk_get_build_info(TwkDevice dev, TwkBuildInfo* info)
try
{
  if (!dev || !info) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_build_info: NULL argument");
  if (!dev->built) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_build_info: twk_build has not been called");
  refreshParams(dev); // the traversal kernel variant depends on the materials as they are now
  dev->buildInfo.traceBlocksPerCU = (uint64_t) traceBuild(dev, false).blocksPerCU;
  *info = dev->buildInfo;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_build_info")

int twk_get_stream_layout(TwkDevice dev, int* layout)
try
{
  if (!dev || !layout) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_stream_layout: NULL argument");
  if (!dev->built) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_stream_layout: twk_build has not been called");
  refreshParams(dev); // cutout opacity is a property of the materials as they are now
  *layout = (slimSlotBits(dev) != 0) ? TWK_STREAMS_SLIM : TWK_STREAMS_FULL;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_stream_layout")

// The device record of instance i of a scene laid out as `layout` says, with the transform the instance has now
static void instanceRecord(TwkDevice dev, const SceneLayout& layout, int i, DevInstance& r)
{
  const InstanceHost& inst = dev->instances[i];
  const GeometryHost& g = dev->geometries[inst.geometry];
  memset(&r, 0, sizeof(r));
  memcpy(r.objectToWorld, inst.transform, sizeof(float) * 12);
  invertAffine(inst.transform, r.worldToObject);
  r.blasRoot = layout.flattened[i] ? layout.flatNodeBase[i] : g.nodeBase; r.material = inst.material; r.light = inst.light;
  r.triangleFirst = layout.flattened[i] ? layout.flatTriangleBase[i] : g.triangleBase; r.triangleCount = g.numTriangles;
  r.attributeBase = g.attributeBase; r.indexBase = g.indexBase; r.geometry = inst.geometry;
}

// World box of an entered instance: its geometry's object-space root box through the transform
static void enteredWorldBox(const float rootBounds[6], const float m[12], float4& boxLo, float4& boxHi)
{
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int corner = 0; corner < 8; ++corner)
  {
    const float x = rootBounds[(corner & 1) ? 3 : 0], y = rootBounds[(corner & 2) ? 4 : 1], z = rootBounds[(corner & 4) ? 5 : 2];
    const float w[3] = { m[0] * x + m[1] * y + m[2] * z + m[3], m[4] * x + m[5] * y + m[6] * z + m[7], m[8] * x + m[9] * y + m[10] * z + m[11] };
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], w[k]); hi[k] = fmaxf(hi[k], w[k]); }
  }
  for (int k = 0; k < 3; ++k)
  {
    // world box of an object-space box: pad for the rounding of the transform in both directions
    const float e = 1.0e-5f * fmaxf(1.0f, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
    lo[k] -= e; hi[k] += e;
  }
  boxLo = make_float4(lo[0], lo[1], lo[2], 0.0f);
  boxHi = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

// The stages of a scene's build. buildScene runs each over the whole scene, updateSelective over what its plan names, both on one
// SceneState: buildScene's own, which a selective-mode build moves into the handle, and from then on the handle's. So an updated
// handle equals a fresh build byte for byte. Their refusals name twk_build, whose they are, whoever runs the stage.
using SceneState = TwkDevice_t::KeptBuild;

// The builder knows the node-cost array during a build or an update only
struct NodeCostScope { BvhBuilder& b; ~NodeCostScope() { b.setNodeCost(nullptr); } };

// Every instance's material and light exist; the largest indices go into the handle, which reads them of a built scene only
static int checkInstanceTables(TwkDevice dev)
{
  dev->maxInstanceMaterial = -1; dev->maxInstanceLight = -1;
  for (const InstanceHost& inst : dev->instances)
  {
    if (inst.material >= (int) dev->materials.size()) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_build: instance material index beyond twk_init_materials");
    if (inst.light >= (int) dev->lights.size()) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_build: instance light index beyond twk_init_lights");
    dev->maxInstanceMaterial = std::max(dev->maxInstanceMaterial, inst.material);
    dev->maxInstanceLight = std::max(dev->maxInstanceLight, inst.light);
  }
  return TWK_SUCCESS;
}

// What update_plan.h lays a scene out from and plans an update with
static void layoutInputs(TwkDevice dev, std::vector<int>& instanceGeometry, std::vector<int>& geometryTriangles)
{
  instanceGeometry.resize(dev->instances.size()); geometryTriangles.resize(dev->geometries.size());
  for (size_t i = 0; i < dev->instances.size(); ++i) instanceGeometry[i] = dev->instances[i].geometry;
  for (size_t k = 0; k < dev->geometries.size(); ++k) geometryTriangles[k] = dev->geometries[k].numTriangles;
}

// The terms of the tree built last; a real build: no refit since, and sahBuilt is what it measured
static TwkDevice_t::TreeTerms lastTerms(const BvhBuilder& b) { return {b.lastSahInner(), b.lastSahLeaf(), b.lastHeight(), b.lastSahInner() + b.lastSahLeaf(), 0}; }

// The world-space tree of flattened instance i at the bases the layout gives it, over `soup` (scratch for its triangles); its terms and
// world box go into the state. Reads d_instances[i]. Zeroes nothing: its node ranges and pair flags are zero before the call.
static int buildFlattenedTree(TwkDevice dev, SceneState& state, int i, int4* soup)
{
  const InstanceHost& inst = dev->instances[i];
  const GeometryHost& g = dev->geometries[inst.geometry];
  const int nodeBase = state.layout.flatNodeBase[i], triangleBase = state.layout.flatTriangleBase[i];
  float bounds[6];
  dev->builder.soupDescriptors(dev->stream, soup, 0, g.numTriangles, i, (int) g.attributeBase, (int) g.indexBase);
  HIP_TRY(hipGetLastError());
  HIP_TRY(dev->builder.buildTriangles(dev->stream, dev->d_attributes, dev->d_indices, g.numTriangles,
                                      dev->d_nodes + nodeBase, dev->d_wideNodes + 2 * (size_t) nodeBase, nodeBase,
                                      dev->d_triangles, dev->d_shadeTriangles, triangleBase, bounds, soup, dev->d_instances,
                                      state.pairs ? state.primFirst[inst.geometry].data() : nullptr, (int) state.primFirst[inst.geometry].size(), dev->d_pairFlags));
  state.instanceTerms[i] = lastTerms(dev->builder);
  state.boxLo[i] = make_float4(bounds[0], bounds[1], bounds[2], 0.0f);
  state.boxHi[i] = make_float4(bounds[3], bounds[4], bounds[5], 0.0f);
  return TWK_SUCCESS;
}

// The top level over the state's boxes and payloads: its emission reads the binary nodes and the costs of the spliced roots
static int buildTopLevel(TwkDevice dev, SceneState& state)
{
  const SceneLayout& layout = state.layout;
  if (layout.single) { dev->tlasRoot = layout.flatNodeBase[0]; state.topHeight = 0; return TWK_SUCCESS; } // the one world-space tree IS the scene
  HIP_TRY(dev->builder.buildInstances(dev->stream, state.boxLo.data(), state.boxHi.data(), state.leafPayload.data(), (int) dev->instances.size(), dev->d_nodes + layout.tlasBase,
                                      dev->d_wideNodes + 2 * (size_t) layout.tlasBase, layout.tlasBase));
  dev->tlasRoot = layout.tlasBase; state.topHeight = dev->builder.lastHeight();
  return TWK_SUCCESS;
}

// Deepest stack a single-ray traversal can need (trace_device.h traverse(): at most one push per inner node on the path,
// plus the sentinel of an instance entry): the top level, then either a spliced world-space tree or an entered
// geometry's tree. The persistent kernel hands rays that outgrow its LDS stack to that traversal, whose stack holds
// TWK_TRACE_STACK_LDS + TWK_TRACE_STACK_SPILL entries; a scene beyond that would lose subtrees silently, so it is refused.
static int checkDepth(TwkDevice dev, const SceneState& state, int* traversalDepth)
{
  const SceneLayout& layout = state.layout;
  int maxEnteredHeight = 0, maxFlatHeight = 0; // binary-tree heights: what a traversal stack may have to hold
  for (size_t k = 0; k < dev->geometries.size(); ++k) if (layout.needsBlas[k]) maxEnteredHeight = std::max(maxEnteredHeight, state.geometryTerms[k].height);
  for (size_t i = 0; i < dev->instances.size(); ++i) if (layout.flattened[i]) maxFlatHeight = std::max(maxFlatHeight, state.instanceTerms[i].height);
  *traversalDepth = state.topHeight + std::max(maxFlatHeight, (layout.numEntered > 0) ? 1 + maxEnteredHeight : 0);
  int depthLimit = TWK_TRACE_STACK_LDS + TWK_TRACE_STACK_SPILL - 2;
  if (const char* e = getenv("TWK_MAX_TRAVERSAL_DEPTH")) depthLimit = std::min(depthLimit, atoi(e)); // test hook: a lower limit only
  if (*traversalDepth <= depthLimit) return TWK_SUCCESS;
  return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_build: the acceleration structure is " + std::to_string(*traversalDepth) + " levels deep (top " + std::to_string(state.topHeight) +
                     ", flattened trees " + std::to_string(maxFlatHeight) + ", entered geometries " + std::to_string(maxEnteredHeight) + "); the traversal stacks hold " +
                     std::to_string(TWK_TRACE_STACK_LDS + TWK_TRACE_STACK_SPILL) + " entries" + (dev->builder.quality() == TWK_BUILD_SAH ? " (try twk_set_build_quality(TWK_BUILD_LBVH))" : ""));
}

// The root as two wide nodes where that pays (bvh_build.hip wideRootKernel), in the two slots behind the scene's last node, which must
// be zero: it opens entries of other trees' full-precision wide nodes. scratch: one word for the kernel's answer.
static int openWideRoot(TwkDevice dev, size_t numNodes, DeviceArray<int>& scratch)
{
  int rc;
  dev->wideRoot1 = dev->tlasRoot; dev->wideRoot2 = TWK_BVH_SENTINEL; dev->wideNodesTotal = numNodes;
  if (!dev->wideRoot) return TWK_SUCCESS;
  if ((rc = scratch.ensure(1))) return rc;
  launchWideRoot(dev->d_wideNodes, dev->tlasRoot, (int) numNodes, scratch, dev->stream);
  int has = 0;
  HIP_TRY(hipMemcpyAsync(&has, scratch, sizeof(int), hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if (has) { dev->wideRoot1 = (int) numNodes; dev->wideRoot2 = (int) numNodes + 1; dev->wideNodesTotal = numNodes + 2; }
  return TWK_SUCCESS;
}

// The top-of-tree caches of the persistent kernel, from the quantised wide nodes as they stand, and the wait that ends the device work
static int fillTopCaches(TwkDevice dev)
{
  int rc;
  if ((rc = dev->d_topNodes.ensure(4 * TWK_TOP_NODES)) || (rc = dev->d_topNodes7.ensure(4 * TWK_TOP_NODES7))) return rc;
  launchTopCache(dev->d_wideQ, dev->wideRoot1, dev->wideRoot2, dev->d_topNodes, TWK_TOP_NODES, dev->stream);
  launchTopCache(dev->d_wideQ, dev->wideRoot1, dev->wideRoot2, dev->d_topNodes7, TWK_TOP_NODES7, dev->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(dev->stream));
  return TWK_SUCCESS;
}

// The SAH terms of the scene: the sum of those of its trees — the entered geometries ascending, then the flattened instances
// ascending. A tree over one build primitive has no inner node and no terms: it adds nothing. (The builder leaves the terms of the
// tree built before it standing, and the sum used to take those again: a one-quad wall built after a sphere counted as another
// sphere. tests/test_gpu_bvh_audit.py holds the sum against the trees read back.)
static void sahTotals(TwkDevice dev, const SceneState& state, TwkBuildInfo& info)
{
  info.sahInnerCost = 0.0; info.sahLeafCost = 0.0;
  const auto tree = [&](const TwkDevice_t::TreeTerms& own, size_t geometry)
  {
    const size_t primitives = state.pairs ? state.primFirst[geometry].size() : (size_t) dev->geometries[geometry].numTriangles;
    if (primitives > 1) { info.sahInnerCost += own.sahInner; info.sahLeafCost += own.sahLeaf; }
  };
  for (size_t k = 0; k < dev->geometries.size(); ++k) if (state.layout.needsBlas[k]) tree(state.geometryTerms[k], k);
  for (size_t i = 0; i < dev->instances.size(); ++i) if (state.layout.flattened[i]) tree(state.instanceTerms[i], (size_t) dev->instances[i].geometry);
}

// The end of a build and of an update: the build info is the handle's, the scene is built
static void finishBuild(TwkDevice dev, const SceneState& state, TwkBuildInfo info, int traversalDepth, std::chrono::steady_clock::time_point start)
{
  sahTotals(dev, state, info);
  info.maxTraversalDepth = (uint64_t) traversalDepth;
  info.buildMilliseconds = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - start).count();
  dev->buildInfo = info;
  dev->twoLevel = (state.layout.numEntered > 0);
  dev->built = true; ++dev->buildSerial; // everything keyed on the serial (tile entry points, refreshParams) is stale
  staleGeometry(dev); // the geometry AOV describes the scene that was
}

// Internal, no entry point: the build of the acceleration structure from the handle's geometries and instances as they are, on an
// active handle — the body of twk_build and of a full-mode twk_update_instance_transform[s] (its refusals name twk_build, whose they are). Drops
// the adaptive state and leaves the geometry AOV stale; the temporal history is the caller's business.
// keep: the build keeps its by-products for selective updates — twk_build passes the handle's update mode, an update of a scene that
// was built without them passes false whatever the mode has been set to since (the mode takes effect at the next twk_build).
static int buildScene(TwkDevice dev, bool keep)
{
  int rc;
  if (dev->geometries.empty() || dev->instances.empty()) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_build: the scene has no geometry or no instance");
  dropAdaptive(dev);
  dev->built = false; // until this build has succeeded: a failure below leaves no half-built scene to launch on
  dev->refitInfoValid = false; // twk_get_refit_info describes a refit of the scene as built
  const auto buildStart = std::chrono::steady_clock::now();
  TwkBuildInfo info;
  memset(&info, 0, sizeof(info));
  info.quality = dev->builder.quality();
  if ((rc = checkInstanceTables(dev))) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  // the mirrors a device-pointer source left stale, while the attribute array they are read from still stands (vertex_source_device.h)
  for (size_t k = 0; k < dev->geometries.size(); ++k) if ((rc = refreshMirror(dev, (int) k))) return rc;

  // Which instances are flattened (include/tweeker_hip.h twk_set_flatten_policy): those of tiny geometries and those
  // whose geometry is referenced so rarely that instancing saves no memory worth the per-ray instance entry (ray
  // transform, per-instance Woop constants, exit step). A flattened instance gets world-space triangle slots and an
  // LBVH of its own whose root is spliced into the top level as an inner node: traversal walks from the top level
  // straight into it with the untransformed ray.
  // The decision and the ranges it gives every tree are update_plan.h's (sceneLayout), which the selective update plans with too.
  const int numInstances = (int) dev->instances.size();
  if (const char* e = getenv("TWK_MAX_LEAF")) dev->builder.setMaxLeaf(atoi(e)); // tuning knob, default 2 triangles per leaf
  std::vector<int> instanceGeometry, geometryTriangles;
  layoutInputs(dev, instanceGeometry, geometryTriangles);
  SceneState state; // what this build produces; a selective-mode build keeps it in the handle
  sceneLayout(instanceGeometry.data(), numInstances, geometryTriangles.data(), (int) dev->geometries.size(), dev->flattenMaxTriangles, dev->flattenMaxReferences,
              dev->builder.maxLeaf(), dev->directSmallLeaves, state.layout);
  const SceneLayout& layout = state.layout;
  const size_t numTris = layout.numTriangles, numNodes = layout.numNodes;

  // shared attribute / index arrays and the node / triangle budgets: one bottom level per geometry that is still
  // entered through an instance, one world-space tree per flattened instance, the top level
  size_t numAttr = 0, numIdx = 0;
  for (size_t k = 0; k < dev->geometries.size(); ++k)
  {
    GeometryHost& g = dev->geometries[k];
    g.attributeBase = (unsigned int) numAttr; g.indexBase = (unsigned int) numIdx;
    g.triangleBase = layout.geometryTriangleBase[k]; g.nodeBase = layout.geometryNodeBase[k];
    numAttr += g.attributes.size(); numIdx += g.indices.size();
  }
  if (numTris >= ((size_t) 1 << 28) || numAttr >= ((size_t) 1 << 31) || numIdx >= ((size_t) 1 << 31))
    return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_build: " + std::to_string(numTris) + " triangle slots; a leaf reference holds 28 bits of slot index");

  // What a selective-mode build keeps past its end is released by anything else: a full-mode build, a failure
  struct KeptScope { TwkDevice dev; bool keep = false; ~KeptScope() { if (!keep) { dev->d_wideNodes.release(); dev->d_nodeCost.release(); dev->d_pairFlags.release(); dev->d_updateSoup.release(); dev->d_updateRanges.release(); dev->d_updateResult.release(); dev->kept.clear(); } } } keptScope{dev};
  dev->kept.clear(); dev->d_nodeCost.release(); dev->d_pairFlags.release();
  // the old scene's arrays are freed before the first of the new one's is asked for
  dev->d_attributes.release(); dev->d_indices.release(); dev->d_nodes.release(); dev->d_wideNodes.release(); dev->d_wideQ.release(); dev->d_triangles.release(); dev->d_shadeTriangles.release(); dev->d_instances.release();
  if ((rc = dev->d_attributes.allocate(sizeof(TwkTriangleAttributes) / sizeof(float) * numAttr)) || (rc = dev->d_indices.allocate(numIdx)) || (rc = dev->d_nodes.allocate(numNodes)) ||
      (rc = dev->d_wideNodes.allocate(2 * (numNodes + 2))) || // + the two nodes of an 8-wide root (wideRootKernel)
      (rc = dev->d_wideQ.allocate(4 * (numNodes + 2))) || (rc = dev->d_triangles.allocate(3 * numTris)) || (rc = dev->d_shadeTriangles.allocate(TWK_SHADE_RECORD * numTris)) ||
      (rc = dev->d_instances.allocate((size_t) numInstances))) return rc;
  // unused nodes stay zero: a tree over pairs has fewer nodes than its triangles reserve
  HIP_TRY(hipMemsetAsync(dev->d_nodes, 0, sizeof(BvhNode) * numNodes, dev->stream));
  HIP_TRY(hipMemsetAsync(dev->d_wideNodes, 0, sizeof(BvhNode) * 2 * (numNodes + 2), dev->stream));
  for (const GeometryHost& g : dev->geometries)
  {
    HIP_TRY(hipMemcpyAsync(dev->d_attributes + 12 * (size_t) g.attributeBase, g.attributes.data(), sizeof(TwkTriangleAttributes) * g.attributes.size(), hipMemcpyHostToDevice, dev->stream));
    HIP_TRY(hipMemcpyAsync(dev->d_indices + g.indexBase, g.indices.data(), sizeof(unsigned int) * g.indices.size(), hipMemcpyHostToDevice, dev->stream));
  }

  // Triangle pairs (device_types.h): the two halves of a quad are one primitive of every tree's build. pairFlags: per slot, whether
  // a pair begins there — what the references of pair leaves are found by once the trees stand.
  state.pairs = dev->trianglePairs && dev->builder.maxLeaf() >= 2;
  state.primFirst.resize(dev->geometries.size());
  std::vector<size_t> geometryPairs(dev->geometries.size(), 0);
  if (state.pairs)
    for (size_t k = 0; k < dev->geometries.size(); ++k)
      geometryPairs[k] = trianglePairs(dev->geometries[k].indices.data(), dev->geometries[k].numTriangles, state.primFirst[k]);
  dev->d_trianglePairs.release();
  if (state.pairs)
  {
    if ((rc = dev->d_pairFlags.allocate(numTris))) return rc;
    HIP_TRY(hipMemsetAsync(dev->d_pairFlags, 0, sizeof(int) * numTris, dev->stream));
  }
  // d_nodeCost: expected wide-node visits below each node, what the wide nodes' cuts are chosen by (bvh_build.hip refitKernel)
  if (dev->costedCuts && (rc = dev->d_nodeCost.allocate(numNodes))) return rc;
  NodeCostScope nodeCostScope{dev->builder};
  dev->builder.setNodeCost(dev->d_nodeCost);
  dev->builder.clearLastSah();
  state.geometryTerms.resize(dev->geometries.size()); state.instanceTerms.resize((size_t) numInstances);
  // bottom level: one LBVH per entered geometry, shared by all of its instances (Device.cpp:1339 caches the GAS per Triangles id)
  for (size_t k = 0; k < dev->geometries.size(); ++k)
  {
    GeometryHost& g = dev->geometries[k];
    if (!layout.needsBlas[k]) continue;
    HIP_TRY(dev->builder.buildTriangles(dev->stream, dev->d_attributes + 12 * (size_t) g.attributeBase, dev->d_indices + g.indexBase, g.numTriangles,
                                        dev->d_nodes + g.nodeBase, dev->d_wideNodes + 2 * (size_t) g.nodeBase, g.nodeBase, dev->d_triangles, dev->d_shadeTriangles, g.triangleBase, g.rootBounds,
                                        nullptr, nullptr, state.pairs ? state.primFirst[k].data() : nullptr, (int) state.primFirst[k].size(), dev->d_pairFlags));
    state.geometryTerms[k] = lastTerms(dev->builder);
    info.pairLeaves += geometryPairs[k]; info.trees += 1;
  }

  // instance records (shading reads them for every hit, flattened or not); every flattened tree's build reads its own
  std::vector<DevInstance> records(numInstances);
  for (int i = 0; i < numInstances; ++i) instanceRecord(dev, layout, i, records[i]);
  HIP_TRY(hipMemcpyAsync(dev->d_instances, records.data(), sizeof(DevInstance) * numInstances, hipMemcpyHostToDevice, dev->stream));

  // world-space trees of the flattened instances + the world boxes and top-level payloads of all instances
  state.boxLo.resize((size_t) numInstances); state.boxHi.resize((size_t) numInstances); state.leafPayload.resize((size_t) numInstances);
  DeviceArray<int4> soup; DeviceArray<int> rootResult; // this build's own scratch, where an update uses the handle's
  if (layout.maxFlatTriangles > 0 && (rc = soup.allocate((size_t) layout.maxFlatTriangles))) return rc;
  for (int i = 0; i < numInstances; ++i)
  {
    const InstanceHost& inst = dev->instances[i];
    const GeometryHost& g = dev->geometries[inst.geometry];
    if (!layout.flattened[i])
    {
      enteredWorldBox(g.rootBounds, inst.transform, state.boxLo[i], state.boxHi[i]);
      state.leafPayload[i] = i;
      continue;
    }
    if ((rc = buildFlattenedTree(dev, state, i, soup))) return rc;
    info.pairLeaves += geometryPairs[inst.geometry]; info.trees += 1;
    state.leafPayload[i] = ~layout.flatNodeBase[i]; // child reference ~payload = the instance's root node: an inner reference
    // A flattened instance of no more triangles than a leaf holds (a wall, the area light: two triangles) IS a leaf of the
    // top level: its slots are referenced directly instead of through a one-node tree of two single-triangle leaves —
    // one node visit and one leaf step less for every ray that crosses its box (C2: six of the eight instances).
    if (layout.directLeaf[i])
    {
      state.leafPayload[i] = layout.flatTriangleBase[i] | ((g.numTriangles - 1) << 28) | TWK_LEAF_WORLD;
      info.directLeafInstances += 1;
    }
  }
  int traversalDepth = 0;
  if ((rc = buildTopLevel(dev, state)) || (rc = checkDepth(dev, state, &traversalDepth)) || (rc = openWideRoot(dev, numNodes, rootResult))) return rc;
  // the whole-array tail. The persistent trace kernel reads the quantised copy of the wide nodes; the full-precision ones were scratch
  launchQuantizeWide(dev->d_wideNodes, dev->d_wideQ, (int) dev->wideNodesTotal, dev->stream);
  // pair leaves get their records and their references in the structures the persistent kernel reads: a flattened scene only
  // (device_types.h "triangle pairs": a two-level scene's references have no free bit)
  if (state.pairs && layout.numEntered == 0 && info.pairLeaves > 0)
  {
    if ((rc = dev->d_trianglePairs.allocate(4 * (numTris / 2 + 1)))) return rc;
    launchPairLeaves(dev->d_wideQ, (int) dev->wideNodesTotal, dev->d_pairFlags, (int) numTris, dev->d_triangles, dev->d_trianglePairs, dev->stream);
  }
  state.pairRewrite = (dev->d_trianglePairs.capacity() != 0);
  if ((rc = fillTopCaches(dev))) return rc;
  if (!keep) dev->d_wideNodes.release();

  info.pairTriangles = 2 * info.pairLeaves;
  info.triangleSlots = numTris; info.nodes = numNodes; info.instances = (uint64_t) numInstances; info.flattenedInstances = (uint64_t) (numInstances - layout.numEntered);
  dev->totalNodes = numNodes; dev->totalTriangles = numTris;
  finishBuild(dev, state, info, traversalDepth, buildStart);
  // selective mode: the by-products stay (include/tweeker_hip.h "Selective instance updates"), and the state with them
  if (keep) { state.valid = true; dev->kept = std::move(state); keptScope.keep = true; }
  return TWK_SUCCESS;
}

int twk_build(TwkDevice dev)
try
{
  int rc = activate(dev, "twk_build"); if (rc) return rc;
  dropLightAnchors(dev); // a built scene starts where its instances and lights are: the next move of an emitter anchors anew
  if ((rc = buildScene(dev, dev->updateMode == TWK_UPDATE_SELECTIVE))) return rc;
  dropTemporal(dev); // the temporal history describes the scene that was
  return TWK_SUCCESS;
}
TWK_CATCH("twk_build")

} // extern "C"

// Device memory a selective-mode handle keeps beyond a full-mode one's
static uint64_t keptBytes(TwkDevice dev)
{
  return (uint64_t) (sizeof(BvhNode) * dev->d_wideNodes.capacity() + sizeof(float) * dev->d_nodeCost.capacity() + sizeof(int) * dev->d_pairFlags.capacity() +
                     sizeof(int4) * dev->d_updateSoup.capacity() + sizeof(int2) * dev->d_updateRanges.capacity() + sizeof(int) * dev->d_updateResult.capacity());
}

// What an update did (twk_get_update_info). keptBytes: a full update is a full-mode build, which keeps nothing past its end
static void recordUpdate(TwkDevice dev, bool selective, int moved, int trees, bool topLevel, size_t nodes, size_t slots, size_t records)
{
  TwkUpdateInfo& u = dev->updateInfo;
  memset(&u, 0, sizeof(u));
  u.selective = selective ? 1 : 0; u.instancesMoved = moved; u.treesRebuilt = trees; u.topLevelRebuilt = topLevel ? 1 : 0;
  u.nodesRequantised = (uint64_t) nodes; u.slotsRewritten = (uint64_t) slots; u.instanceRecordsUploaded = (uint64_t) records;
  u.keptBytes = keptBytes(dev); u.milliseconds = dev->buildInfo.buildMilliseconds;
  dev->updateInfoValid = true;
}

// A tree of geometry `geometry` over `nodes` nodes has been refit, with the SAH terms `now`: its terms (the height stays: a refit
// changes no tree's height) and the call's record. A tree over one build primitive has no terms (sahTotals).
static void countRefit(TwkDevice dev, const SceneState& state, int geometry, TwkDevice_t::TreeTerms& terms, const double now[2], int nodes, TwkRefitInfo& info)
{
  const size_t primitives = state.pairs ? state.primFirst[(size_t) geometry].size() : (size_t) dev->geometries[(size_t) geometry].numTriangles;
  terms.refits += 1;
  if (primitives > 1)
  {
    terms.sahInner = now[0]; terms.sahLeaf = now[1];
    info.sahBuilt += terms.sahBuilt; info.sahNow += now[0] + now[1];
  }
  info.treesRefit += 1; info.nodesRefit += (uint64_t) nodes; info.refitsSinceBuild = std::max(info.refitsSinceBuild, terms.refits);
}

// An update of a handle that kept nothing: the scene built again in full mode, and the record of it
static int updateFull(TwkDevice dev, int moved, size_t records)
{
  int rc;
  if ((rc = buildScene(dev, false))) return rc;
  recordUpdate(dev, false, moved, dev->buildInfo.trees, !(dev->instances.size() == 1 && dev->buildInfo.flattenedInstances == 1), dev->wideNodesTotal, dev->totalTriangles, records);
  return TWK_SUCCESS;
}

// What a selective update works from: the update plan of the call's moved instances and updated geometries (update_plan.h) and, for
// a refit, the trees of its one batch (refit_scene_plan.h). Why the batch cannot be planned, or nullptr. Changes nothing:
// twk_refit_scene asks before it stores anything, updateSelective when it runs.
struct UpdatePlans { std::vector<int> instanceGeometry, geometryTriangles; UpdatePlan plan; RefitScenePlan refit; };
static const char* planUpdate(TwkDevice dev, const int* moved, int numMoved, const int* updated, int numUpdated, bool refit, UpdatePlans& p)
{
  layoutInputs(dev, p.instanceGeometry, p.geometryTriangles);
  updatePlanWith(dev->kept.layout, p.instanceGeometry.data(), p.geometryTriangles.data(), moved, numMoved, updated, numUpdated, p.plan);
  if (!refit) return nullptr;
  return refitScenePlan(dev->kept.layout, p.instanceGeometry.data(), p.geometryTriangles.data(), p.plan, moved, numMoved, updated, numUpdated, p.refit);
}

// The refit stage of a selective update: every tree of the plan in place, all in one batch (bvh_refit.hip launchRefitSceneTrees), in
// stream order behind the rebuilds of the direct leaves. Then, per tree in the plan's order — geometries ascending, then instances
// ascending — its box to where the top level reads it (a bottom-level tree's to the geometry's rootBounds, so that the boxes of its
// entered instances follow; a world-space tree's to the instance's box), its new SAH terms, and the call into `info`.
static int refitTrees(TwkDevice dev, SceneState& state, const RefitScenePlan& plan, TwkRefitInfo& info)
{
  int rc;
  const size_t numTrees = plan.tree.size();
  if (numTrees == 0) return TWK_SUCCESS;
  if ((rc = dev->d_refitScratch.ensure(refitSceneScratchWords(plan)))) return rc;
  std::vector<RefitSceneKind> kinds(numTrees);
  for (size_t k = 0; k < numTrees; ++k)
  {
    const GeometryHost& g = dev->geometries[plan.geometry[k]];
    kinds[k] = {plan.kind[k], plan.kind[k] == REFIT_SCENE_GEOMETRY ? -1 : plan.tree[k], (int) g.attributeBase, (int) g.indexBase};
  }
  std::vector<float> bounds(6 * numTrees);
  std::vector<double> now(2 * numTrees);
  HIP_TRY(launchRefitSceneTrees(dev->stream, dev->d_attributes, dev->d_indices, dev->d_instances, dev->d_nodes, dev->d_wideNodes, dev->d_nodeCost, dev->d_triangles,
                                dev->d_shadeTriangles, state.pairs ? dev->d_pairFlags.get() : nullptr, plan, kinds.data(), dev->d_refitScratch, bounds.data(), now.data()));
  for (size_t k = 0; k < numTrees; ++k)
  {
    const int geometry = plan.geometry[k], i = plan.tree[k];
    const float* b = &bounds[6 * k];
    if (plan.kind[k] == REFIT_SCENE_GEOMETRY) memcpy(dev->geometries[geometry].rootBounds, b, sizeof(float) * 6);
    else { state.boxLo[i] = make_float4(b[0], b[1], b[2], 0.0f); state.boxHi[i] = make_float4(b[3], b[4], b[5], 0.0f); }
    countRefit(dev, state, geometry, plan.kind[k] == REFIT_SCENE_GEOMETRY ? state.geometryTerms[geometry] : state.instanceTerms[i], &now[2 * k], plan.nodes[k], info);
  }
  return TWK_SUCCESS;
}

// Internal, no entry point: the update of a handle built in selective mode (include/tweeker_hip.h "Selective instance updates") after
// the transforms of the instances `moved` (distinct) have been replaced. It runs buildScene's stages (above) for what the plan names,
// on arrays that hold what buildScene's held at that point — so the result is a fresh build's, byte for byte. A failure leaves the
// handle unbuilt (twk_build recovers it).
// updated: geometries (distinct) whose attributes have been replaced, numUpdated of them: their slices of d_attributes are uploaded,
// the bottom-level tree of an entered one is rebuilt at the node and slot range it has, and the trees and boxes of their instances
// follow (update_plan.h updatePlanWith).
// refit (the twk_refit_* calls): only a direct-leaf instance, which has no tree of its own, takes the rebuild's path; every other
// tree the plan names is refit in place (refitTrees, above) instead of zeroed and rebuilt. The stages around the trees are the same;
// the handle is then a legal scene for the new vertices and transforms, not a fresh build's.
static int updateSelective(TwkDevice dev, const int* moved, int numMoved, const int* updated = nullptr, int numUpdated = 0, bool refit = false)
{
  int rc;
  SceneState& state = dev->kept;
  const SceneLayout& layout = state.layout;
  dropAdaptive(dev);
  dev->built = false; // until this update has succeeded
  const auto start = std::chrono::steady_clock::now();
  if ((rc = checkInstanceTables(dev))) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));

  UpdatePlans plans;
  if (const char* why = planUpdate(dev, moved, numMoved, updated, numUpdated, refit, plans)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string("twk_build: the refit batch: ") + why);
  const UpdatePlan& plan = plans.plan;
  const std::vector<int>& instanceGeometry = plans.instanceGeometry;
  const std::vector<int>& geometryTriangles = plans.geometryTriangles;
  const size_t numNodes = layout.numNodes, numTris = layout.numTriangles;

  // the records of the moved instances only (the new object-to-world matrix and its inverse); they live until the first synchronise
  std::vector<DevInstance> records((size_t) numMoved);
  for (int k = 0; k < numMoved; ++k)
  {
    instanceRecord(dev, layout, moved[k], records[k]);
    HIP_TRY(hipMemcpyAsync(dev->d_instances + moved[k], &records[k], sizeof(DevInstance), hipMemcpyHostToDevice, dev->stream));
  }

  NodeCostScope nodeCostScope{dev->builder};
  dev->builder.setNodeCost(dev->d_nodeCost);
  // the new vertices
  for (int k = 0; k < numUpdated; ++k)
  {
    const GeometryHost& g = dev->geometries[updated[k]];
    if (mirrorStale(g)) continue; // a device-pointer source has written the slice already (vertex_source_device.h): it is what the upload would bring
    HIP_TRY(hipMemcpyAsync(dev->d_attributes + 12 * (size_t) g.attributeBase, g.attributes.data(), sizeof(TwkTriangleAttributes) * g.attributes.size(), hipMemcpyHostToDevice, dev->stream));
  }
  // the bottom-level tree of every updated geometry that is entered: buildScene's call on the range it has. A fresh build starts
  // from zeroed node arrays and pair flags, and what a tree leaves unused of its range must stay zero
  if (!refit) for (int k : plan.geometries)
  {
    GeometryHost& g = dev->geometries[k];
    const int nodes = treeNodes(g.numTriangles);
    HIP_TRY(hipMemsetAsync(dev->d_nodes + g.nodeBase, 0, sizeof(BvhNode) * (size_t) nodes, dev->stream));
    HIP_TRY(hipMemsetAsync(dev->d_wideNodes + 2 * (size_t) g.nodeBase, 0, sizeof(BvhNode) * 2 * (size_t) nodes, dev->stream));
    if (state.pairs) HIP_TRY(hipMemsetAsync(dev->d_pairFlags + g.triangleBase, 0, sizeof(int) * (size_t) g.numTriangles, dev->stream));
    HIP_TRY(dev->builder.buildTriangles(dev->stream, dev->d_attributes + 12 * (size_t) g.attributeBase, dev->d_indices + g.indexBase, g.numTriangles,
                                        dev->d_nodes + g.nodeBase, dev->d_wideNodes + 2 * (size_t) g.nodeBase, g.nodeBase, dev->d_triangles, dev->d_shadeTriangles, g.triangleBase, g.rootBounds,
                                        nullptr, nullptr, state.pairs ? state.primFirst[k].data() : nullptr, (int) state.primFirst[k].size(), dev->d_pairFlags));
    state.geometryTerms[k] = lastTerms(dev->builder);
  }
  // the world-space tree of every flattened instance the plan names, at the bases it has — of a refit, the direct leaves only
  const std::vector<int>& rebuilt = refit ? plans.refit.directLeaves : plan.trees;
  int maxTriangles = 0;
  for (int i : rebuilt) maxTriangles = std::max(maxTriangles, geometryTriangles[instanceGeometry[i]]);
  if (maxTriangles > 0 && (rc = dev->d_updateSoup.ensure((size_t) maxTriangles))) return rc;
  for (int i : rebuilt)
  {
    const int nodeBase = layout.flatNodeBase[i], triangleBase = layout.flatTriangleBase[i], triangles = geometryTriangles[instanceGeometry[i]], nodes = treeNodes(triangles);
    HIP_TRY(hipMemsetAsync(dev->d_nodes + nodeBase, 0, sizeof(BvhNode) * (size_t) nodes, dev->stream));
    HIP_TRY(hipMemsetAsync(dev->d_wideNodes + 2 * (size_t) nodeBase, 0, sizeof(BvhNode) * 2 * (size_t) nodes, dev->stream));
    if (state.pairs) HIP_TRY(hipMemsetAsync(dev->d_pairFlags + triangleBase, 0, sizeof(int) * (size_t) triangles, dev->stream));
    if ((rc = buildFlattenedTree(dev, state, i, dev->d_updateSoup))) return rc;
    // its payload in the top level (its root, or its slots as a direct leaf) names bases, which do not move
  }
  TwkRefitInfo refitInfo;
  memset(&refitInfo, 0, sizeof(refitInfo));
  if (refit && (rc = refitTrees(dev, state, plans.refit, refitInfo))) return rc;
  // a moved entered instance: its box in the top level, nothing else — no bottom-level tree is rebuilt
  for (int k = 0; k < numMoved; ++k)
    if (!layout.flattened[moved[k]])
      enteredWorldBox(dev->geometries[dev->instances[moved[k]].geometry].rootBounds, dev->instances[moved[k]].transform, state.boxLo[moved[k]], state.boxHi[moved[k]]);
  // an entered instance of an updated geometry: the new root box through its transform
  for (int i : plan.boxes) enteredWorldBox(dev->geometries[dev->instances[i].geometry].rootBounds, dev->instances[i].transform, state.boxLo[i], state.boxHi[i]);

  // the top level over the kept and the new boxes; the depth, from the kept and the new heights
  int traversalDepth = 0;
  if ((rc = buildTopLevel(dev, state)) || (rc = checkDepth(dev, state, &traversalDepth))) return rc;
  // the 8-wide root again, from zeroed root slots as in a fresh build
  HIP_TRY(hipMemsetAsync(dev->d_wideNodes + 2 * numNodes, 0, sizeof(BvhNode) * 4, dev->stream));
  if ((rc = openWideRoot(dev, numNodes, dev->d_updateResult))) return rc;

  // the ranged tail: the quantised copy and the pair references of the changed node ranges, in one launch. The records of pairs a
  // rebuilt tree no longer has stay in d_trianglePairs (sized by slots, it does not move): nothing references them.
  std::vector<int2> table(plan.ranges.size());
  int position = 0;
  for (size_t r = 0; r < plan.ranges.size(); ++r) { table[r] = make_int2(plan.ranges[r].first, position); position += plan.ranges[r].count; }
  if ((rc = dev->d_updateRanges.ensure(table.size()))) return rc;
  HIP_TRY(hipMemcpyAsync(dev->d_updateRanges, table.data(), sizeof(int2) * table.size(), hipMemcpyHostToDevice, dev->stream));
  launchRangedTail(dev->d_wideNodes, dev->d_wideQ, dev->d_updateRanges, (int) table.size(), position, state.pairRewrite ? dev->d_pairFlags.get() : nullptr, (int) numTris,
                   dev->d_triangles, dev->d_trianglePairs, dev->stream);
  if ((rc = fillTopCaches(dev))) return rc; // waits for the stream: `table` and `records` may go away

  // the build info: counts, pair leaves, quality — no transform changes them — and what the changed trees change
  finishBuild(dev, state, dev->buildInfo, traversalDepth, start);
  recordUpdate(dev, true, numMoved, (int) ((refit ? 0 : plan.geometries.size()) + rebuilt.size()), plan.topLevel, plan.totalNodes, plan.totalSlots, (size_t) numMoved);
  if (refit)
  {
    refitInfo.treesRebuilt = (int) rebuilt.size(); refitInfo.topLevelRebuilt = plan.topLevel ? 1 : 0; refitInfo.slotsRewritten = (uint64_t) plan.totalSlots; refitInfo.milliseconds = dev->buildInfo.buildMilliseconds;
    dev->refitInfo = refitInfo; dev->refitInfoValid = true;
  }
  return TWK_SUCCESS;
}

// The entries of a transform call on a built handle, each refused with the transform update's text (batch: "entry k: " in front)
static int checkTransformEntries(TwkDevice dev, const char* name, bool batch, int count, const int* ids, const float* transforms)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  for (int k = 0; k < count; ++k)
  {
    const std::string entry = batch ? "entry " + std::to_string(k) + ": " : "";
    const int id = ids[k];
    const float* transform = transforms + 12 * (size_t) k;
    if (id < 0 || id >= (int) dev->instances.size()) return refuse(TWK_ERROR_INVALID_VALUE, entry + "bad instance id");
    if (!instanceTransformUsable(transform)) return refuse(TWK_ERROR_INVALID_VALUE, entry + "the transform is not finite, or its 3 x 3 determinant is zero or not finite");
    if (dev->instances[id].light >= 0 && !dev->emitterMotion)
      return refuse(TWK_ERROR_INVALID_VALUE, entry + "the instance carries a light (idLight >= 0): its light definition holds the emitter's position and would disagree; moving emitters is not supported");
    for (int j = 0; j < k; ++j) if (ids[j] == id) return refuse(TWK_ERROR_INVALID_VALUE, entry + "instance " + std::to_string(id) + " is listed twice (also entry " + std::to_string(j) + ")");
  }
  return TWK_SUCCESS;
}

// Emitters among the entries of a transform call that checkTransformEntries has passed, with twk_enable_emitter_motion on
// (light_motion.h): per entry that carries a light, in entry order, the refusals — a light that is no parallelogram, a light a second
// instance carries, a derived definition that is degenerate — and what applyEmitterMoves will write. Changes nothing.
struct EmitterMove { int light; bool anchors; LightAnchor anchor; TwkLightDefinition moved; };
static int planEmitterMoves(TwkDevice dev, const char* name, bool batch, int count, const int* ids, const float* transforms, std::vector<EmitterMove>& moves)
{
  const auto refuse = [name](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  moves.clear();
  for (int k = 0; k < count; ++k)
  {
    const int id = ids[k], light = dev->instances[id].light;
    if (light < 0) continue;
    const std::string entry = (batch ? "entry " + std::to_string(k) + ": " : std::string()) + "instance " + std::to_string(id) + " carries light " + std::to_string(light) + ": ";
    if (dev->lights[light].type != TWK_LIGHT_PARALLELOGRAM) return refuse(entry + lightNotParallelogram);
    for (size_t j = 0; j < dev->instances.size(); ++j)
      if ((int) j != id && dev->instances[j].light == light)
        return refuse(entry + "the light is carried by more than one instance (instances " + std::to_string(std::min((int) j, id)) + " and " + std::to_string(std::max((int) j, id)) +
                      "): one definition cannot follow both");
    EmitterMove m;
    m.light = light;
    m.anchors = !((size_t) light < dev->lightAnchors.size() && dev->lightAnchors[light].valid);
    if (m.anchors) { m.anchor.valid = true; m.anchor.definition = dev->lights[light]; memcpy(m.anchor.transform, dev->instances[id].transform, sizeof(float) * 12); }
    else m.anchor = dev->lightAnchors[light];
    if (const char* why = lightMoved(m.anchor.definition, m.anchor.transform, transforms + 12 * (size_t) k, m.moved)) return refuse(entry + why);
    moves.push_back(m);
  }
  return TWK_SUCCESS;
}

// ... and, once nothing is refused any more and the instances have their transforms: the anchors taken, the definitions set, each
// uploaded on the handle's stream (in stream order behind everything that still reads the table, before the rebuild or refit)
static int applyEmitterMoves(TwkDevice dev, const std::vector<EmitterMove>& moves)
{
  for (const EmitterMove& m : moves)
  {
    if (m.anchors)
    {
      if (dev->lightAnchors.size() < dev->lights.size()) dev->lightAnchors.resize(dev->lights.size());
      dev->lightAnchors[m.light] = m.anchor;
    }
    dev->lights[m.light] = m.moved;
    HIP_TRY(hipMemcpyAsync(dev->d_lights + m.light, &dev->lights[m.light], sizeof(DevLight), hipMemcpyHostToDevice, dev->stream));
  }
  return TWK_SUCCESS;
}

// The body of twk_update_instance_transform (batch false: its texts) and of twk_update_instance_transforms (each refusal names its entry)
// and of twk_refit_instance_transform[s] (refit: the same refusals in the same order and the refit's one more, then the refit path)
static int updateTransforms(TwkDevice dev, const char* name, bool batch, int count, const int* ids, const float* transforms, bool refit = false)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  // the batch's own arguments first, so that they are refused without the handle being looked at; the single call keeps its order
  if (batch && count < 1) return refuse(TWK_ERROR_INVALID_VALUE, "count must be at least 1");
  if (batch && (!ids || !transforms)) return refuse(TWK_ERROR_INVALID_VALUE, "NULL array of ids or transforms");
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  if (!batch && !transforms) return refuse(TWK_ERROR_INVALID_VALUE, "NULL transform");
  int rc = activate(dev, name); if (rc) return rc;
  if (!dev->built) return refuse(TWK_ERROR_INVALID_STATE, "twk_build has not been called");
  if (refit && !dev->kept.valid)
    return refuse(TWK_ERROR_INVALID_STATE, "the scene was not built in TWK_UPDATE_SELECTIVE (twk_set_update_mode before twk_build): nothing a refit needs was kept");
  if ((rc = checkTransformEntries(dev, name, batch, count, ids, transforms))) return rc;
  std::vector<EmitterMove> emitters;
  if ((rc = planEmitterMoves(dev, name, batch, count, ids, transforms, emitters))) return rc;
  // nothing was changed up to here: a refused batch changes nothing
  for (int k = 0; k < count; ++k) memcpy(dev->instances[ids[k]].transform, transforms + 12 * (size_t) k, sizeof(float) * 12);
  if ((rc = applyEmitterMoves(dev, emitters))) return rc;
  dev->updateInfoValid = false; // an update that fails from here on leaves no record: twk_get_update_info describes a finished update
  // the temporal history stays: the merges look it up where the instance was (device_temporal.hip ownMotion)
  if (dev->kept.valid) return updateSelective(dev, ids, count, nullptr, 0, refit);
  return updateFull(dev, count, dev->instances.size());
}

// The body of twk_update_plan_host (no updated geometry) and of twk_vertex_update_plan_host
static int updatePlanHost(const char* name, const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries, int flattenMaxTriangles,
                          int flattenMaxReferences, int maxLeaf, const int* moved, int numMoved, const int* updated, int numUpdated,
                          TwkUpdatePlan* plan, unsigned char* flattened, int* trees, int* ranges)
{
  const auto refuse = [name](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!instanceGeometry || !geometryTriangles || !plan || (numMoved > 0 && !moved) || (numUpdated > 0 && !updated)) return refuse("NULL argument");
  if (numInstances < 1 || numGeometries < 1 || numMoved < 0 || numUpdated < 0 || flattenMaxTriangles < 0 || flattenMaxReferences < 0) return refuse("counts must be at least 1 and limits at least 0");
  for (int k = 0; k < numGeometries; ++k) if (geometryTriangles[k] < 1) return refuse("geometry " + std::to_string(k) + " has no triangle");
  for (int i = 0; i < numInstances; ++i) if (instanceGeometry[i] < 0 || instanceGeometry[i] >= numGeometries) return refuse("instance " + std::to_string(i) + ": bad geometry index");
  for (int k = 0; k < numMoved; ++k)
  {
    if (moved[k] < 0 || moved[k] >= numInstances) return refuse("entry " + std::to_string(k) + ": bad instance id");
    for (int j = 0; j < k; ++j) if (moved[j] == moved[k]) return refuse("entry " + std::to_string(k) + ": instance " + std::to_string(moved[k]) + " is listed twice");
  }
  for (int k = 0; k < numUpdated; ++k)
  {
    if (updated[k] < 0 || updated[k] >= numGeometries) return refuse("updated entry " + std::to_string(k) + ": bad geometry id");
    for (int j = 0; j < k; ++j) if (updated[j] == updated[k]) return refuse("updated entry " + std::to_string(k) + ": geometry " + std::to_string(updated[k]) + " is listed twice");
  }
  SceneLayout layout;
  sceneLayout(instanceGeometry, numInstances, geometryTriangles, numGeometries, flattenMaxTriangles, flattenMaxReferences, std::max(1, std::min(4, maxLeaf)) /* BvhBuilder::setMaxLeaf */, true, layout);
  UpdatePlan p;
  updatePlanWith(layout, instanceGeometry, geometryTriangles, moved, numMoved, updated, numUpdated, p);
  memset(plan, 0, sizeof(*plan));
  plan->instances = numInstances; plan->flattenedInstances = numInstances - layout.numEntered; plan->tlasBase = layout.tlasBase;
  for (int i = 0; i < numInstances; ++i) plan->directLeafInstances += layout.directLeaf[i] ? 1 : 0;
  for (int k = 0; k < numGeometries; ++k) plan->enteredGeometries += layout.needsBlas[k] ? 1 : 0;
  plan->nodes = layout.numNodes; plan->triangleSlots = layout.numTriangles;
  if (numMoved > 0 || numUpdated > 0)
  {
    plan->treesRebuilt = (int) (p.geometries.size() + p.trees.size()); plan->topLevelRebuilt = p.topLevel ? 1 : 0; plan->numRanges = (int) p.ranges.size();
    plan->nodesRequantised = p.totalNodes; plan->slotsRewritten = p.totalSlots;
    // a rebuilt bottom-level tree is listed as ~geometry, before the flattened instances
    if (trees) for (size_t k = 0; k < p.geometries.size(); ++k) trees[k] = ~p.geometries[k];
    if (trees) for (size_t k = 0; k < p.trees.size(); ++k) trees[p.geometries.size() + k] = p.trees[k];
    if (ranges) for (size_t k = 0; k < p.ranges.size(); ++k) { ranges[2 * k] = p.ranges[k].first; ranges[2 * k + 1] = p.ranges[k].count; }
  }
  if (flattened) for (int i = 0; i < numInstances; ++i) flattened[i] = layout.flattened[i] ? 1 : 0;
  return TWK_SUCCESS;
}

// A geometry's new host records, refused with the vertex update's texts behind `where` (the call's name, and its entry in twk_refit_scene)
static int checkVertices(TwkDevice dev, const std::string& where, int idGeometry, const TwkTriangleAttributes* attributes, size_t numAttributes)
{
  const auto refuse = [&where](int code, const std::string& text) { return twkSetError(code, where + text); };
  if (idGeometry < 0 || idGeometry >= (int) dev->geometries.size()) return refuse(TWK_ERROR_INVALID_VALUE, "bad geometry id");
  const GeometryHost& g = dev->geometries[idGeometry];
  if (numAttributes != g.attributes.size())
    return refuse(TWK_ERROR_INVALID_VALUE, "the geometry has " + std::to_string(g.attributes.size()) + " vertices, not " + std::to_string(numAttributes) + " (the indices stay: no topology change)");
  for (size_t v = 0; v < numAttributes; ++v)
    if (!std::isfinite(attributes[v].vertex[0]) || !std::isfinite(attributes[v].vertex[1]) || !std::isfinite(attributes[v].vertex[2]))
      return refuse(TWK_ERROR_INVALID_VALUE, "vertex " + std::to_string(v) + ": the position is not finite");
  for (size_t i = 0; i < dev->instances.size(); ++i)
    if (dev->instances[i].geometry == idGeometry && dev->instances[i].light >= 0)
      return refuse(TWK_ERROR_INVALID_VALUE, "instance " + std::to_string(i) + " of the geometry carries a light (idLight >= 0): its light definition holds the emitter's shape and would disagree; deforming emitters is not supported");
  return TWK_SUCCESS;
}

// ... and, once nothing is refused any more, the previous positions kept and the new vertices on the host
static int storeVertices(TwkDevice dev, int idGeometry, const TwkTriangleAttributes* attributes, size_t numAttributes)
{
  int rc;
  GeometryHost& g = dev->geometries[idGeometry];
  if (dev->temporalHasHistory && (rc = refreshMirror(dev, idGeometry))) return rc; // keepPreviousPositions reads the mirror
  keepPreviousPositions(dev, idGeometry); // the positions as of the history's frame, before the first update since (device_temporal.hip)
  g.attributes.assign(attributes, attributes + numAttributes);
  if (g.device) g.device->mirrorStale = false; // whole again, and newer than the slice a device-pointer source wrote: the upload brings it
  dev->updateInfoValid = false;
  return TWK_SUCCESS;
}

// The front half of twk_update_geometry_vertices and of twk_refit_geometry_vertices (refit: its one refusal more): the refusals under
// the caller's name, then — nothing was changed up to there — the previous positions kept and the new vertices on the host
static int replaceVertices(TwkDevice dev, const char* name, bool refit, int idGeometry, const TwkTriangleAttributes* attributes, size_t numAttributes)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  if (!attributes) return refuse(TWK_ERROR_INVALID_VALUE, "NULL attributes");
  int rc = activate(dev, name); if (rc) return rc;
  if (!dev->built) return refuse(TWK_ERROR_INVALID_STATE, "twk_build has not been called");
  if (refit && !dev->kept.valid)
    return refuse(TWK_ERROR_INVALID_STATE, "the scene was not built in TWK_UPDATE_SELECTIVE (twk_set_update_mode before twk_build): nothing a refit needs was kept");
  if ((rc = checkVertices(dev, std::string(name) + ": ", idGeometry, attributes, numAttributes))) return rc;
  // nothing was changed up to here: a refused call changes nothing
  return storeVertices(dev, idGeometry, attributes, numAttributes);
}

extern "C" {

int twk_update_geometry_vertices(TwkDevice dev, int idGeometry, const TwkTriangleAttributes* attributes, size_t numAttributes)
try
{
  int rc = replaceVertices(dev, "twk_update_geometry_vertices", false, idGeometry, attributes, numAttributes); if (rc) return rc;
  // the temporal history stays: the merges look it up where the surface was (twk_render_geometry_motion, temporal_carry_device.h)
  if (dev->kept.valid) return updateSelective(dev, nullptr, 0, &idGeometry, 1);
  return updateFull(dev, 0, 0);
}
TWK_CATCH("twk_update_geometry_vertices")

int twk_refit_geometry_vertices(TwkDevice dev, int idGeometry, const TwkTriangleAttributes* attributes, size_t numAttributes)
try
{
  int rc = replaceVertices(dev, "twk_refit_geometry_vertices", true, idGeometry, attributes, numAttributes); if (rc) return rc;
  return updateSelective(dev, nullptr, 0, &idGeometry, 1, true);
}
TWK_CATCH("twk_refit_geometry_vertices")

// The two calls with a device-pointer source (vertex_source_device.h; device_vertex_source.hip ingestVertexSource): the slice of
// d_attributes is written on the device, and the rebuild or refit that follows is the one above
int twk_update_geometry_vertices_device(TwkDevice dev, int idGeometry, const TwkVertexSource* source, size_t numVertices)
try
{
  int rc = ingestVertexSource(dev, "twk_update_geometry_vertices_device", false, idGeometry, source, numVertices); if (rc) return rc;
  if (dev->kept.valid) return updateSelective(dev, nullptr, 0, &idGeometry, 1);
  return updateFull(dev, 0, 0); // the build reads the slice back into the mirror before the arrays are allocated again
}
TWK_CATCH("twk_update_geometry_vertices_device")

int twk_refit_geometry_vertices_device(TwkDevice dev, int idGeometry, const TwkVertexSource* source, size_t numVertices)
try
{
  int rc = ingestVertexSource(dev, "twk_refit_geometry_vertices_device", true, idGeometry, source, numVertices); if (rc) return rc;
  return updateSelective(dev, nullptr, 0, &idGeometry, 1, true);
}
TWK_CATCH("twk_refit_geometry_vertices_device")

int twk_get_refit_info(TwkDevice dev, TwkRefitInfo* info)
try
{
  if (!dev || !info) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_refit_info: NULL argument");
  if (!dev->refitInfoValid) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_refit_info: no refit has been made on this handle since it was last built");
  *info = dev->refitInfo;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_refit_info")

int twk_refit_tree_host(float* nodes, float* wideNodes, float* nodeCost, float* slots, float* shadeRecords, const int* pairFlags,
                        const TwkTriangleAttributes* attributes, size_t numAttributes, const unsigned int* indices, size_t numIndices,
                        int nodeBase, int numNodes, int slotBase, int numSlots, int leafFlag, const float* transform, int idInstance,
                        double* terms, float* rootBounds)
try
{
  const auto refuse = [](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_refit_tree_host: " + text); };
  if (!nodes || !wideNodes || !slots || !shadeRecords || !attributes || !indices) return refuse("NULL argument");
  if (numNodes < 1 || numSlots < 1 || nodeBase < 0 || slotBase < 0 || numAttributes < 1 || (size_t) numSlots >= ((size_t) 1 << 28) || (size_t) slotBase + (size_t) numSlots > ((size_t) 1 << 28) ||
      (size_t) nodeBase + (size_t) numNodes > (size_t) TWK_BVH_SENTINEL)
    return refuse("counts must be at least 1, bases at least 0, and the ranges within what a reference holds");
  if (numIndices != 3 * (size_t) numSlots) return refuse("numIndices is " + std::to_string(numIndices) + ", not three per slot (" + std::to_string(3 * (size_t) numSlots) + ")");
  if (leafFlag != 0 && leafFlag != TWK_LEAF_WORLD) return refuse("leafFlag is neither 0 nor TWK_LEAF_WORLD");
  if (leafFlag != 0 && (!transform || idInstance < 0 || idInstance >= (1 << 24))) return refuse("a world-space tree needs its transform and an instance id of at least 0 (and below 2^24)");
  for (size_t i = 0; i < numIndices; ++i) if (indices[i] >= numAttributes) return refuse("index " + std::to_string(i) + " is beyond the attributes");
  // the caller's arrays need not be 16-byte aligned: the header's code works on copies
  std::vector<BvhNode> n((size_t) numNodes), w(2 * (size_t) numNodes);
  std::vector<float4> t(3 * (size_t) numSlots), shade(TWK_SHADE_RECORD * (size_t) numSlots);
  memcpy(n.data(), nodes, sizeof(BvhNode) * n.size()); memcpy(w.data(), wideNodes, sizeof(BvhNode) * w.size()); memcpy(t.data(), slots, sizeof(float4) * t.size());
  std::vector<float> cost;
  if (nodeCost) cost.assign(nodeCost, nodeCost + numNodes);
  RefitTree tree;
  tree.nodes = n.data(); tree.wide = w.data(); tree.nodeCost = nodeCost ? cost.data() : nullptr; tree.triangles = t.data(); tree.pairFlags = pairFlags;
  tree.nodeBase = nodeBase; tree.numNodes = numNodes; tree.slotBase = slotBase; tree.numSlots = numSlots;
  std::vector<int> parents;
  if (const char* why = refitTreeRefusal(tree, (size_t) numSlots, parents)) return refuse(why);
  for (int i = 0; i < numNodes; ++i)
  {
    int c[2];
    refitChildren(tree.nodes + i, c[0], c[1]);
    if (refitUnused(c[0], c[1])) continue;
    for (int k = 0; k < 2; ++k)
      if (c[k] < 0 && !(k == 1 && refitNeverHit(tree.nodes + i)) && ((~c[k]) & TWK_LEAF_WORLD) != leafFlag) return refuse("node " + std::to_string(nodeBase + i) + ": a leaf reference's TWK_LEAF_WORLD is not leafFlag");
  }
  // a world-space tree: the soup descriptors and the one instance record emitTriangle reads, as buildFlattenedTree makes them
  std::vector<int4> soup;
  std::vector<DevInstance> instances;
  if (leafFlag != 0) refitSoupHost(numSlots, idInstance, transform, soup, instances);
  double sums[2];
  float bounds[6];
  refitTreeHost(tree, parents, reinterpret_cast<const float*>(attributes), indices, leafFlag ? soup.data() : nullptr, leafFlag ? instances.data() : nullptr, t.data(), shade.data(), sums, bounds);
  memcpy(nodes, n.data(), sizeof(BvhNode) * n.size()); memcpy(wideNodes, w.data(), sizeof(BvhNode) * w.size()); memcpy(slots, t.data(), sizeof(float4) * t.size());
  memcpy(shadeRecords, shade.data(), sizeof(float4) * shade.size());
  if (nodeCost) memcpy(nodeCost, cost.data(), sizeof(float) * cost.size());
  if (terms) { terms[0] = sums[0]; terms[1] = sums[1]; }
  if (rootBounds) memcpy(rootBounds, bounds, sizeof(bounds));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_refit_tree_host")

int twk_vertex_update_plan_host(const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries, int flattenMaxTriangles,
                                int flattenMaxReferences, int maxLeaf, const int* moved, int numMoved, const int* updatedGeometries, int numUpdated,
                                TwkUpdatePlan* plan, unsigned char* flattened, int* trees, int* ranges)
try
{
  return updatePlanHost("twk_vertex_update_plan_host", instanceGeometry, numInstances, geometryTriangles, numGeometries, flattenMaxTriangles, flattenMaxReferences, maxLeaf,
                        moved, numMoved, updatedGeometries, numUpdated, plan, flattened, trees, ranges);
}
TWK_CATCH("twk_vertex_update_plan_host")

int twk_update_instance_transform(TwkDevice dev, int idInstance, const float transform[12])
try
{
  return updateTransforms(dev, "twk_update_instance_transform", false, 1, &idInstance, transform);
}
TWK_CATCH("twk_update_instance_transform")

int twk_update_instance_transforms(TwkDevice dev, int count, const int* idInstances, const float* transforms)
try
{
  return updateTransforms(dev, "twk_update_instance_transforms", true, count, idInstances, transforms);
}
TWK_CATCH("twk_update_instance_transforms")

int twk_refit_instance_transform(TwkDevice dev, int idInstance, const float transform[12])
try
{
  return updateTransforms(dev, "twk_refit_instance_transform", false, 1, &idInstance, transform, true);
}
TWK_CATCH("twk_refit_instance_transform")

int twk_refit_instance_transforms(TwkDevice dev, int count, const int* idInstances, const float* transforms)
try
{
  return updateTransforms(dev, "twk_refit_instance_transforms", true, count, idInstances, transforms, true);
}
TWK_CATCH("twk_refit_instance_transforms")

int twk_refit_batch_plan_host(const int* treeNodes, const int* treeSlots, int numTrees, TwkRefitBatchPlan* plan, int* nodeOffsets, int* slotOffsets,
                              int* nodeBlockFirst, int* slotBlockFirst, int* nodeBlocks, int* slotBlocks)
try
{
  const auto refuse = [](const std::string& text) { return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_refit_batch_plan_host: " + text); };
  if (!plan || (numTrees > 0 && (!treeNodes || !treeSlots))) return refuse("NULL argument");
  RefitBatchPlan p;
  if (const char* why = refitBatchPlan(treeNodes, treeSlots, numTrees, p)) return refuse(why);
  memset(plan, 0, sizeof(*plan));
  plan->trees = numTrees; plan->nodeBlocks = p.totalNodeBlocks; plan->slotBlocks = p.totalSlotBlocks; plan->blockThreads = REFIT_BATCH_BLOCK;
  plan->nodes = (uint64_t) p.totalNodes; plan->slots = (uint64_t) p.totalSlots;
  for (int k = 0; k < numTrees; ++k)
  {
    if (nodeOffsets) nodeOffsets[k] = p.nodeOffset[(size_t) k];
    if (slotOffsets) slotOffsets[k] = p.slotOffset[(size_t) k];
    if (nodeBlockFirst) nodeBlockFirst[k] = p.nodeBlockFirst[(size_t) k];
    if (slotBlockFirst) slotBlockFirst[k] = p.slotBlockFirst[(size_t) k];
  }
  if (nodeBlocks) for (size_t b = 0; b < p.nodeBlocks.size(); ++b) { nodeBlocks[2 * b] = p.nodeBlocks[b].tree; nodeBlocks[2 * b + 1] = p.nodeBlocks[b].first; }
  if (slotBlocks) for (size_t b = 0; b < p.slotBlocks.size(); ++b) { slotBlocks[2 * b] = p.slotBlocks[b].tree; slotBlocks[2 * b + 1] = p.slotBlocks[b].first; }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_refit_batch_plan_host")

// A frame's edits in one call (include/tweeker_hip.h "A frame's edits in one call"): every entry is checked before anything is
// written — the call's own arguments, the handle, the geometry entries in order, the instance entries, last the finite check of all
// device sources (one launch per source into one result array, ONE read-back and wait) — then the vertices are stored as the vertex
// calls store them, the transforms as the transform calls do, and updateSelective refits every tree once.
int twk_refit_scene(TwkDevice dev, int numGeometries, const TwkGeometryEdit* geometries, int numInstances, const int* idInstances, const float* transforms)
try
{
  const char* name = "twk_refit_scene";
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (numGeometries < 0 || numInstances < 0) return refuse(TWK_ERROR_INVALID_VALUE, "the counts must be at least 0");
  if (numGeometries == 0 && numInstances == 0) return refuse(TWK_ERROR_INVALID_VALUE, "both counts are 0: nothing to refit");
  if (numGeometries > 0 && !geometries) return refuse(TWK_ERROR_INVALID_VALUE, "NULL array of geometry entries");
  if (numInstances > 0 && (!idInstances || !transforms)) return refuse(TWK_ERROR_INVALID_VALUE, "NULL array of ids or transforms");
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  int rc = activate(dev, name); if (rc) return rc;
  if (!dev->built) return refuse(TWK_ERROR_INVALID_STATE, "twk_build has not been called");
  if (!dev->kept.valid)
    return refuse(TWK_ERROR_INVALID_STATE, "the scene was not built in TWK_UPDATE_SELECTIVE (twk_set_update_mode before twk_build): nothing a refit needs was kept");
  std::vector<VertexSourceView> views((size_t) numGeometries);
  std::vector<int> updated((size_t) numGeometries);
  int numSources = 0;
  for (int k = 0; k < numGeometries; ++k)
  {
    const TwkGeometryEdit& e = geometries[k];
    const std::string entry = std::string(name) + ": geometry entry " + std::to_string(k) + ": ";
    if ((e.attributes != nullptr) == (e.source != nullptr)) return twkSetError(TWK_ERROR_INVALID_VALUE, entry + "the entry sets exactly one of attributes and source");
    if (e.reserved != 0) return twkSetError(TWK_ERROR_INVALID_VALUE, entry + "the reserved word is not 0");
    for (int j = 0; j < k; ++j)
      if (geometries[j].idGeometry == e.idGeometry) return twkSetError(TWK_ERROR_INVALID_VALUE, entry + "geometry " + std::to_string(e.idGeometry) + " is listed twice (also geometry entry " + std::to_string(j) + ")");
    if (e.attributes) rc = checkVertices(dev, entry, e.idGeometry, e.attributes, (size_t) e.numVertices);
    else { rc = checkVertexSource(dev, entry, e.idGeometry, e.source, (size_t) e.numVertices, views[(size_t) k]); ++numSources; }
    if (rc) return rc;
    updated[(size_t) k] = e.idGeometry;
  }
  if ((rc = checkTransformEntries(dev, name, true, numInstances, idInstances, transforms))) return rc;
  if (numSources > 0)
  {
    // read-only, and read before anything is written: word k is the lowest vertex of entry k whose position is not finite
    std::vector<unsigned int> lowest((size_t) numGeometries, 0xffffffffu);
    if ((rc = dev->d_sourceCheck.ensure((size_t) numGeometries))) return rc;
    HIP_TRY(hipMemsetAsync(dev->d_sourceCheck, 0xff, sizeof(unsigned int) * (size_t) numGeometries, dev->stream));
    for (int k = 0; k < numGeometries; ++k)
      if (geometries[k].source) launchVertexSourceCheck(views[(size_t) k].pointer, views[(size_t) k].stride, (unsigned int) geometries[k].numVertices, dev->d_sourceCheck + k, dev->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lowest.data(), dev->d_sourceCheck, sizeof(unsigned int) * (size_t) numGeometries, hipMemcpyDeviceToHost, dev->stream));
    HIP_TRY(hipStreamSynchronize(dev->stream));
    for (int k = 0; k < numGeometries; ++k)
      if (lowest[(size_t) k] != 0xffffffffu)
        return refuse(TWK_ERROR_INVALID_VALUE, "geometry entry " + std::to_string(k) + ": vertex " + std::to_string(lowest[(size_t) k]) + ": the position is not finite");
  }
  {
    // the batch as updateSelective will plan it: a batch that cannot be planned is refused here, before anything is stored
    UpdatePlans plans;
    if (const char* why = planUpdate(dev, idInstances, numInstances, updated.data(), numGeometries, true, plans)) return refuse(TWK_ERROR_INVALID_VALUE, std::string("the refit batch: ") + why);
  }
  std::vector<EmitterMove> emitters;
  if ((rc = planEmitterMoves(dev, name, true, numInstances, idInstances, transforms, emitters))) return rc;
  // nothing was changed up to here: a refused call changes nothing
  for (int k = 0; k < numGeometries; ++k)
  {
    const TwkGeometryEdit& e = geometries[k];
    if ((rc = e.attributes ? storeVertices(dev, e.idGeometry, e.attributes, (size_t) e.numVertices) : storeVertexSource(dev, e.idGeometry, views[(size_t) k]))) return rc;
  }
  for (int k = 0; k < numInstances; ++k) memcpy(dev->instances[idInstances[k]].transform, transforms + 12 * (size_t) k, sizeof(float) * 12);
  if ((rc = applyEmitterMoves(dev, emitters))) return rc;
  dev->updateInfoValid = false;
  // the temporal history stays, as after the calls this one stands for
  return updateSelective(dev, idInstances, numInstances, updated.data(), numGeometries, true);
}
TWK_CATCH("twk_refit_scene")

int twk_scene_refit_plan_host(const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries, int flattenMaxTriangles,
                              int flattenMaxReferences, int maxLeaf, const int* moved, int numMoved, const int* updatedGeometries, int numUpdated,
                              TwkSceneRefitPlan* plan, int* trees, int* kinds, int* nodeBases, int* nodeCounts, int* slotBases, int* slotCounts,
                              int* nodeOffsets, int* slotOffsets, int* nodeBlockFirst, int* slotBlockFirst, int* nodeBlocks, int* slotBlocks)
try
{
  const char* name = "twk_scene_refit_plan_host";
  if (!plan) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  TwkUpdatePlan update; // the inputs' refusals are the update plan's, under this call's name
  int rc = updatePlanHost(name, instanceGeometry, numInstances, geometryTriangles, numGeometries, flattenMaxTriangles, flattenMaxReferences, maxLeaf, moved, numMoved,
                          updatedGeometries, numUpdated, &update, nullptr, nullptr, nullptr);
  if (rc) return rc;
  SceneLayout layout;
  sceneLayout(instanceGeometry, numInstances, geometryTriangles, numGeometries, flattenMaxTriangles, flattenMaxReferences, std::max(1, std::min(4, maxLeaf)), true, layout);
  UpdatePlan u;
  updatePlanWith(layout, instanceGeometry, geometryTriangles, moved, numMoved, updatedGeometries, numUpdated, u);
  RefitScenePlan p;
  if (const char* why = refitScenePlan(layout, instanceGeometry, geometryTriangles, u, moved, numMoved, updatedGeometries, numUpdated, p)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + why);
  memset(plan, 0, sizeof(*plan));
  plan->trees = (int) p.tree.size(); plan->nodeBlocks = p.batch.totalNodeBlocks; plan->slotBlocks = p.batch.totalSlotBlocks; plan->blockThreads = REFIT_BATCH_BLOCK;
  plan->directLeaves = (int) p.directLeaves.size(); plan->topLevelRebuilt = u.topLevel ? 1 : 0;
  plan->boxes = (int) p.boxes.size();
  plan->nodes = (uint64_t) p.batch.totalNodes; plan->slots = (uint64_t) p.batch.totalSlots; plan->slotsRewritten = (uint64_t) u.totalSlots; plan->slotBytes = (uint64_t) p.slotBytes;
  for (size_t k = 0; k < p.tree.size(); ++k)
  {
    if (trees) trees[k] = p.tree[k];
    if (kinds) kinds[k] = p.kind[k];
    if (nodeBases) nodeBases[k] = p.nodeBase[k];
    if (nodeCounts) nodeCounts[k] = p.nodes[k];
    if (slotBases) slotBases[k] = p.slotBase[k];
    if (slotCounts) slotCounts[k] = p.slots[k];
    if (nodeOffsets) nodeOffsets[k] = p.batch.nodeOffset[k];
    if (slotOffsets) slotOffsets[k] = p.batch.slotOffset[k];
    if (nodeBlockFirst) nodeBlockFirst[k] = p.batch.nodeBlockFirst[k];
    if (slotBlockFirst) slotBlockFirst[k] = p.batch.slotBlockFirst[k];
  }
  if (nodeBlocks) for (size_t b = 0; b < p.batch.nodeBlocks.size(); ++b) { nodeBlocks[2 * b] = p.batch.nodeBlocks[b].tree; nodeBlocks[2 * b + 1] = p.batch.nodeBlocks[b].first; }
  if (slotBlocks) for (size_t b = 0; b < p.batch.slotBlocks.size(); ++b) { slotBlocks[2 * b] = p.batch.slotBlocks[b].tree; slotBlocks[2 * b + 1] = p.batch.slotBlocks[b].first; }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_scene_refit_plan_host")

int twk_set_update_mode(TwkDevice dev, int mode)
try
{
  if (!dev) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_update_mode: NULL device handle");
  if (mode != TWK_UPDATE_FULL && mode != TWK_UPDATE_SELECTIVE) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_set_update_mode: unknown mode " + std::to_string(mode));
  dev->updateMode = mode; // read by the next twk_build: the built scene keeps updating the way it was built
  return TWK_SUCCESS;
}
TWK_CATCH("twk_set_update_mode")

int twk_get_update_info(TwkDevice dev, TwkUpdateInfo* info)
try
{
  if (!dev || !info) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_get_update_info: NULL argument");
  if (!dev->updateInfoValid) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_get_update_info: no update has been made on this handle");
  *info = dev->updateInfo;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_update_info")

int twk_update_plan_host(const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries, int flattenMaxTriangles,
                         int flattenMaxReferences, int maxLeaf, const int* moved, int numMoved, TwkUpdatePlan* plan, unsigned char* flattened, int* trees, int* ranges)
try
{
  return updatePlanHost("twk_update_plan_host", instanceGeometry, numInstances, geometryTriangles, numGeometries, flattenMaxTriangles, flattenMaxReferences, maxLeaf,
                        moved, numMoved, nullptr, 0, plan, flattened, trees, ranges);
}
TWK_CATCH("twk_update_plan_host")

int twk_get_instance_transform(TwkDevice dev, int idInstance, float transform[12])
try
{
  const char* name = "twk_get_instance_transform";
  if (!dev || !transform) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + (dev ? ": NULL transform" : ": NULL device handle"));
  if (idInstance < 0 || idInstance >= (int) dev->instances.size()) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": bad instance id");
  memcpy(transform, dev->instances[idInstance].transform, sizeof(float) * 12);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_instance_transform")

} // extern "C"
