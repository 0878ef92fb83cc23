// Measurement probes and parity taps of the C ABI: nothing a renderer needs, everything the tests and the profiles do.
#include "device_handle.h"

#include <algorithm>
#include <cstring>

static int collectTimed(TwkDevice dev)
{
  if (dev->timedUsed == 0) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  for (size_t i = 0; i < dev->timedUsed; ++i)
  {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, dev->timed[i].start, dev->timed[i].stop));
    dev->profileMs[dev->timed[i].kind] += ms;
    dev->profileLaunches[dev->timed[i].kind] += 1;
  }
  dev->timedUsed = 0;
  return TWK_SUCCESS;
}

// =============================================================================================
extern "C" {

// ---- measurement ------------------------------------------------------------------------------
int twk_profile_enable(TwkDevice dev, int enable)
try
{
  int rc = activate(dev, "twk_profile_enable"); if (rc) return rc;
  if ((rc = collectTimed(dev))) return rc;
  dev->profileEnabled = (enable != 0);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_profile_enable")

int twk_profile_reset(TwkDevice dev)
try
{
  int rc = activate(dev, "twk_profile_reset"); if (rc) return rc;
  if ((rc = collectTimed(dev))) return rc;
  for (int k = 0; k < TWK_KERNEL_COUNT; ++k) { dev->profileMs[k] = 0.0f; dev->profileLaunches[k] = 0; }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_profile_reset")

int twk_profile_get(TwkDevice dev, float ms[TWK_KERNEL_COUNT], int launches[TWK_KERNEL_COUNT])
try
{
  int rc = activate(dev, "twk_profile_get"); if (rc) return rc;
  if ((rc = collectTimed(dev))) return rc;
  for (int k = 0; k < TWK_KERNEL_COUNT; ++k) { if (ms) ms[k] = dev->profileMs[k]; if (launches) launches[k] = dev->profileLaunches[k]; }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_profile_get")

int twk_stats_enable(TwkDevice dev, int enable)
try
{
  return setSwitch(dev, "twk_stats_enable", &TwkDevice_t::statsEnabled, enable);
}
TWK_CATCH("twk_stats_enable")

int twk_stats_get(TwkDevice dev, TwkLaunchStats* stats, int reset)
try
{
  int rc = activate(dev, "twk_stats_get"); if (rc) return rc;
  if (!stats) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_stats_get: NULL argument");
  memset(stats, 0, sizeof(*stats));
  if (!dev->d_stats) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  unsigned long long h[TWK_STATS_WORDS / 2];
  HIP_TRY(hipMemcpy(h, dev->d_stats, sizeof(h), hipMemcpyDeviceToHost));
  // the words by name: device_types.h StatWord
  stats->radianceRays = h[TWK_STAT_RADIANCE_RAYS]; stats->shadowRays = h[TWK_STAT_SHADOW_RAYS]; stats->nodesVisited = h[TWK_STAT_NODES_VISITED]; stats->trianglesTested = h[TWK_STAT_TRIANGLES_TESTED];
  stats->instancesEntered = h[TWK_STAT_INSTANCES_ENTERED]; stats->shadedHits = h[TWK_STAT_SHADED_HITS]; stats->missed = h[TWK_STAT_MISSED]; stats->maxNodesPerRay = h[TWK_STAT_MAX_NODES_PER_RAY];
  stats->overflowRays = h[TWK_STAT_OVERFLOW_RAYS]; // tailRays .. tailInstancesEntered (words 8-11): the tail kernel is not part of this build, they stay 0
  stats->nodeWaveSteps = h[TWK_STAT_NODE_WAVE_STEPS]; stats->triangleWaveSteps = h[TWK_STAT_TRIANGLE_WAVE_STEPS]; stats->leafWaveSteps = h[TWK_STAT_LEAF_WAVE_STEPS];
  stats->cachedNodesVisited = h[TWK_STAT_CACHED_NODES]; stats->droppedStackPushes = dev->h_dropped ? *dev->h_dropped : 0u;
  for (int i = 0; i < 6; ++i) stats->waveCycles[i] = h[TWK_STAT_WAVE_CYCLES + i];
  const int TWK_SHADE_PHASES = TWK_SHADE_PHASE_COUNT; static_assert(TWK_STAT_SHADE_PHASES + 3 * TWK_SHADE_PHASE_COUNT <= TWK_STATS_WORDS / 2, "shade phase words"); // shade_device.h asserts TWK_SHADE_PHASES == TWK_SHADE_PHASE_COUNT
  for (int i = 0; i < TWK_SHADE_PHASES; ++i) { stats->shadePhaseWaveSteps[i] = h[TWK_STAT_SHADE_PHASES + i]; stats->shadePhaseLanes[i] = h[TWK_STAT_SHADE_PHASES + TWK_SHADE_PHASES + i]; stats->shadePhaseCycles[i] = h[TWK_STAT_SHADE_PHASES + 2 * TWK_SHADE_PHASES + i]; }
  if (reset) HIP_TRY(hipMemset(dev->d_stats, 0, sizeof(h)));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_stats_get")

int twk_stream_peak_gbps(TwkDevice dev, size_t bytes, int repeats, float* gbps)
try
{
  int rc = activate(dev, "twk_stream_peak_gbps"); if (rc) return rc;
  if (!gbps || bytes < 4096 || repeats < 1) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_stream_peak_gbps: bad arguments");
  const size_t n = (bytes / sizeof(float4)) & ~(size_t) 1023; // whole 16 KiB pieces of the copy kernel
  float4 *a = nullptr, *b = nullptr;
  HIP_TRY(hipMalloc(&a, n * sizeof(float4)));
  if (hipMalloc(&b, n * sizeof(float4)) != hipSuccess) { (void) hipFree(a); return twkSetError(TWK_ERROR_OUT_OF_MEMORY, "twk_stream_peak_gbps: out of memory"); }
  (void) hipMemsetAsync(a, 0, n * sizeof(float4), dev->stream);
  hipEvent_t e0, e1;
  (void) hipEventCreate(&e0); (void) hipEventCreate(&e1);
  launchStreamCopy(a, b, n, dev->stream); // warm-up
  (void) hipEventRecord(e0, dev->stream);
  for (int i = 0; i < repeats; ++i) launchStreamCopy(a, b, n, dev->stream);
  (void) hipEventRecord(e1, dev->stream);
  hipError_t e = hipStreamSynchronize(dev->stream);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
  (void) hipFree(a); (void) hipFree(b);
  if (e != hipSuccess) return twkSetError(TWK_ERROR_HIP, std::string("twk_stream_peak_gbps: ") + hipGetErrorString(e));
  *gbps = (float) (2.0 * (double) (n * sizeof(float4)) * repeats / ((double) ms * 1.0e-3) / 1.0e9);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_stream_peak_gbps")

int twk_gather_peak(TwkDevice dev, size_t tableBytes, float* gigaLaneLoadsPerSecond)
try
{
  int rc = activate(dev, "twk_gather_peak"); if (rc) return rc;
  if (!gigaLaneLoadsPerSecond || tableBytes < 128 * 1024 || tableBytes > ((size_t) 1 << 36)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_gather_peak: bad arguments");
  const unsigned int lines = (unsigned int) (tableBytes / 128);
  DeviceArray<float4> table; DeviceArray<float> out;
  if ((rc = table.allocate((size_t) lines * 8))) return rc;
  if ((rc = out.allocate(1))) return rc;
  launchGatherProbeFill(table, (size_t) lines * 8, lines, dev->stream);
  const int blocks = dev->numCUs * 6, steps = 1000; // 6 waves per SIMD, as the traversal kernel runs
  launchGatherProbe(table, lines, 50, out, blocks, dev->stream); // warm-up: table into the caches
  hipEvent_t e0, e1;
  (void) hipEventCreate(&e0); (void) hipEventCreate(&e1);
  (void) hipEventRecord(e0, dev->stream);
  launchGatherProbe(table, lines, steps, out, blocks, dev->stream);
  (void) hipEventRecord(e1, dev->stream);
  hipError_t e = hipStreamSynchronize(dev->stream);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
  if (e != hipSuccess) return twkSetError(TWK_ERROR_HIP, std::string("twk_gather_peak: ") + hipGetErrorString(e));
  *gigaLaneLoadsPerSecond = (float) ((double) blocks * 256.0 * steps * 8.0 / ((double) ms * 1.0e-3) / 1.0e9);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_gather_peak")

// ---- parity taps ------------------------------------------------------------------------------
int twk_debug_capture(TwkDevice dev, int enable)
try
{
  return setSwitch(dev, "twk_debug_capture", &TwkDevice_t::captureFirstHits, enable);
}
TWK_CATCH("twk_debug_capture")

int twk_debug_read_path_radiance(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_debug_read_path_radiance"); if (rc) return rc; // deferred launches run first: the last pass is theirs
  if (!host) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_read_path_radiance: NULL buffer");
  if (dev->lastPassCount <= 0 || !dev->d_streamBlock) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_debug_read_path_radiance: no pass has been rendered (or its streams have been overwritten since)");
  const size_t n = (size_t) dev->lastPassCount * dev->lastPassPixels;
  if (numFloats != n * 4) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_read_path_radiance: buffer must hold " + std::to_string(dev->lastPassCount) + " x launchWidth*height*4 floats (the samples per launch index of the last pass)");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  HIP_TRY(hipMemcpy(host, dev->params.pathRadiance, n * sizeof(float4), hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_read_path_radiance")

int twk_debug_shade_builds(TwkDevice dev, uint64_t mask[2], int reset)
try
{
  int rc = activate(dev, "twk_debug_shade_builds"); if (rc) return rc; // deferred launches are enqueued, and recorded, first
  if (!mask) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_shade_builds: NULL mask");
  mask[0] = dev->shadeBuilds[0]; mask[1] = dev->shadeBuilds[1];
  if (reset) dev->shadeBuilds[0] = dev->shadeBuilds[1] = 0;
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_shade_builds")

int twk_debug_shade_build_slots(uint64_t mask[2])
try
{
  if (!mask) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_shade_build_slots: NULL mask");
  twk::shadeBuildSlots(mask);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_shade_build_slots")

int twk_debug_read_first_hits(TwkDevice dev, float* tBetaGamma, int* instPrim, size_t numPixels)
try
{
  int rc = activate(dev, "twk_debug_read_first_hits"); if (rc) return rc;
  const size_t n = (size_t) dev->launchWidth * dev->state.resolution[1];
  if (!tBetaGamma || !instPrim || numPixels != n) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_read_first_hits: size mismatch");
  if (!dev->d_firstHit) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_debug_read_first_hits: nothing captured");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  std::vector<float4> h(n); std::vector<int> inst(n);
  HIP_TRY(hipMemcpy(h.data(), dev->d_firstHit, n * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(inst.data(), dev->d_firstHitInstance, n * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i)
  {
    tBetaGamma[3 * i] = h[i].x; tBetaGamma[3 * i + 1] = h[i].y; tBetaGamma[3 * i + 2] = h[i].z;
    instPrim[2 * i] = inst[i];
    int prim; memcpy(&prim, &h[i].w, 4);
    instPrim[2 * i + 1] = (inst[i] < 0) ? -1 : prim;
  }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_read_first_hits")

int twk_trace_rays(TwkDevice dev, const float* rays, size_t numRays, int anyHit, float* tBetaGamma, int* ids)
try
{
  int rc = activate(dev, "twk_trace_rays"); if (rc) return rc;
  if (!dev->built) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_trace_rays: twk_build has not been called");
  if (!rays || !tBetaGamma || !ids) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_trace_rays: NULL buffer");
  if (numRays == 0) return TWK_SUCCESS;
  if (!dev->stateSet) { dev->launchWidth = 1; }
  if ((rc = ensureStreams(dev))) return rc;
  refreshParams(dev);
  DeviceArray<float> d_rays, d_out; DeviceArray<int> d_ids;
  if ((rc = d_rays.allocate(numRays * 8))) return rc;
  if ((rc = d_out.allocate(numRays * 3))) return rc;
  if ((rc = d_ids.allocate(numRays * 2))) return rc;
  HIP_TRY(hipMemcpyAsync(d_rays, rays, numRays * 8 * sizeof(float), hipMemcpyHostToDevice, dev->stream));
  int grid = (int) ((numRays + TWK_TRACE_BLOCK - 1) / TWK_TRACE_BLOCK);
  if (grid > dev->numCUs * TWK_TRACE_WAVES) grid = dev->numCUs * TWK_TRACE_WAVES;
  launchTraceQuery(dev->params, d_rays, (unsigned int) numRays, anyHit, d_out, d_ids, grid, dev->stream);
  HIP_TRY(hipMemcpyAsync(tBetaGamma, d_out, numRays * 3 * sizeof(float), hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipMemcpyAsync(ids, d_ids, numRays * 2 * sizeof(int), hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  return checkDroppedPushes(dev, "twk_trace_rays");
}
TWK_CATCH("twk_trace_rays")

int twk_debug_trace_queue(TwkDevice dev, const float* closestRays, size_t numClosest, const float* shadowRays, size_t numShadow,
                          float* tBetaGammaSlot, int* instance, int* occluded)
try
{
  int rc = activate(dev, "twk_debug_trace_queue"); if (rc) return rc;
  if (!dev->built) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_debug_trace_queue: twk_build has not been called");
  if ((numClosest && (!closestRays || !tBetaGammaSlot || !instance)) || (numShadow && (!shadowRays || !occluded))) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_trace_queue: NULL buffer");
  for (const DevMaterial& m : dev->materials) if (m.textureCutout) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_debug_trace_queue: geometric query only, not for scenes with cutout opacity");
  const size_t n = std::max(numClosest, numShadow);
  if (n == 0) return TWK_SUCCESS;
  if (n >= ((size_t) 1 << 30)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_trace_queue: too many rays");
  if (!dev->stateSet) { dev->launchWidth = 1; }
  const size_t pixels = (size_t) dev->launchWidth * (size_t) dev->state.resolution[1];
  if ((rc = ensureStreams(dev, (int) std::min<size_t>((n + pixels - 1) / pixels, (size_t) 1 << 30)))) return rc;
  if (dev->d_streamBlock.capacity() < n) return twkSetError(TWK_ERROR_OUT_OF_MEMORY, "twk_debug_trace_queue: path streams too small");
  dev->lastPassCount = 0; // the streams of the last pass are overwritten below
  refreshParams(dev);
  LaunchParams p = dev->params;
  p.numPaths = (int) dev->d_streamBlock.capacity(); p.batchCount = 1; p.firstHit = nullptr; p.firstHitInstance = nullptr; p.pathTime = nullptr;
  p.stats = dev->statsEnabled ? dev->d_stats : nullptr; // twk_stats_enable: visit counts and the number of rays that overflowed the LDS stack (tests/test_gpu_big_scenes.py)
  // the rays of one bounce: radiance rays in queue 1, the shadow rays "emitted by shade 0" in the shadow queue
  std::vector<float4> org(n), dir(n);
  std::vector<unsigned int> index(n);
  for (size_t i = 0; i < n; ++i) index[i] = (unsigned int) i;
  auto split = [&](const float* rays, size_t count)
  {
    for (size_t i = 0; i < count; ++i)
    {
      const float* r = rays + 8 * i;
      org[i] = make_float4(r[0], r[1], r[2], r[3]); dir[i] = make_float4(r[4], r[5], r[6], r[7]);
    }
  };
  HIP_TRY(hipStreamSynchronize(dev->stream));
  HIP_TRY(hipMemset(dev->d_counters, 0, sizeof(unsigned int) * TWK_COUNTER_WORDS));
  if (numClosest)
  {
    split(closestRays, numClosest);
    HIP_TRY(hipMemcpy(p.rayOrg[1], org.data(), numClosest * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p.rayDir[1], dir.data(), numClosest * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p.rayPixel[1], index.data(), numClosest * sizeof(unsigned int), hipMemcpyHostToDevice));
    const unsigned int c = (unsigned int) numClosest;
    HIP_TRY(hipMemcpy(dev->d_counters + 1 * TWK_COUNTERS_PER_DEPTH + TWK_COUNTER_CLOSEST, &c, sizeof(c), hipMemcpyHostToDevice)); // everything in segment 0
  }
  if (numShadow)
  {
    split(shadowRays, numShadow);
    std::vector<float4> pending(numShadow, make_float4(1.0f, 0.0f, 0.0f, 0.0f));
    HIP_TRY(hipMemcpy(p.shadowOrg, org.data(), numShadow * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p.shadowDir, dir.data(), numShadow * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p.shadowPixel, index.data(), numShadow * sizeof(unsigned int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p.shadowPending, pending.data(), numShadow * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(p.pathRadiance, 0, numShadow * sizeof(float4)));
    const unsigned int c = (unsigned int) numShadow;
    HIP_TRY(hipMemcpy(dev->d_counters + 0 * TWK_COUNTERS_PER_DEPTH + TWK_COUNTER_SHADOW, &c, sizeof(c), hipMemcpyHostToDevice));
  }
  const TraceBuild build = traceBuild(dev, false);
  launchTrace(p, 1, dev->statsEnabled, build, dev->numCUs * build.blocksPerCU, dev->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if ((rc = checkDroppedPushes(dev, "twk_debug_trace_queue"))) return rc;
  if (numClosest)
  {
    HIP_TRY(hipMemcpy(tBetaGammaSlot, p.hitRecord, numClosest * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(instance, p.hitInstance, numClosest * sizeof(int), hipMemcpyDeviceToHost));
  }
  if (numShadow)
  {
    std::vector<float4> radiance(numShadow);
    HIP_TRY(hipMemcpy(radiance.data(), p.pathRadiance, numShadow * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < numShadow; ++i) occluded[i] = (radiance[i].x == 0.0f) ? 1 : 0; // an unoccluded shadow ray adds its pending contribution (1, 0, 0)
  }
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_trace_queue")

} // extern "C"

// The references of pair leaves (device_types.h "triangle pairs") in a host copy of the quantised wide nodes, back in the form the
// build gave them: whoever reads the acceleration structure on the host walks slots, not pair records. References are rewritten
// in flattened scenes only, where every leaf is a world-space leaf.
static void canonicalLeafReferences(TwkDevice dev, void* wideQ, size_t nodes)
{
  if (dev->d_trianglePairs.capacity() == 0) return;
  int* words = static_cast<int*>(wideQ);
  for (size_t i = 0; i < nodes; ++i)
    for (int k = 12; k < 16; ++k)
      if (words[16 * i + k] < 0) words[16 * i + k] = ~(~words[16 * i + k] | TWK_LEAF_WORLD);
}

extern "C" {

int twk_debug_read_acceleration(TwkDevice dev, TwkAccelerationInfo* info, void* wideNodes, void* triangles, void* instances)
try
{
  int rc = activate(dev, "twk_debug_read_acceleration"); if (rc) return rc;
  if (!info) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_read_acceleration: NULL info");
  if (!dev->built) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_debug_read_acceleration: twk_build has not been called");
  info->root = dev->wideRoot1; info->twoLevel = dev->twoLevel ? 1 : 0;
  info->root2 = (dev->wideRoot2 == TWK_BVH_SENTINEL) ? -1 : dev->wideRoot2; info->nodeFloats = 16;
  info->numNodes = (uint64_t) dev->wideNodesTotal; info->numTriangleSlots = dev->totalTriangles; info->numInstances = dev->instances.size(); // 4-ary nodes: the binary nodes' + the two of an 8-wide root
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if (wideNodes)
  {
    HIP_TRY(hipMemcpy(wideNodes, dev->d_wideQ, sizeof(float) * (size_t) info->nodeFloats * info->numNodes, hipMemcpyDeviceToHost));
    canonicalLeafReferences(dev, wideNodes, (size_t) info->numNodes);
  }
  if (triangles) HIP_TRY(hipMemcpy(triangles, dev->d_triangles, sizeof(float4) * 3 * dev->totalTriangles, hipMemcpyDeviceToHost));
  if (instances) HIP_TRY(hipMemcpy(instances, dev->d_instances, sizeof(DevInstance) * dev->instances.size(), hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_read_acceleration")

int twk_debug_read_kept_build(TwkDevice dev, float* wide, size_t numWideFloats, float* nodeCost, size_t numNodeCost, int* pairFlags, size_t numPairFlags)
try
{
  const char* name = "twk_debug_read_kept_build";
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev) return refuse(TWK_ERROR_INVALID_VALUE, "NULL device handle");
  int rc = activate(dev, name); if (rc) return rc;
  if (!dev->built || !dev->kept.valid) return refuse(TWK_ERROR_INVALID_STATE, "the handle holds no scene built in TWK_UPDATE_SELECTIVE (twk_set_update_mode before twk_build)");
  const size_t wideFloats = 32 * (dev->totalNodes + 2);
  if (wide && (!dev->d_wideNodes.holds(2 * (dev->totalNodes + 2)))) return refuse(TWK_ERROR_INVALID_STATE, "the full-precision wide nodes are not kept");
  if (nodeCost && !dev->d_nodeCost.holds(dev->totalNodes)) return refuse(TWK_ERROR_INVALID_STATE, "no node costs are kept (costed cuts are off)");
  if (pairFlags && !dev->d_pairFlags.holds(dev->totalTriangles)) return refuse(TWK_ERROR_INVALID_STATE, "no pair flags are kept (the scene was built without pairs)");
  if ((wide && numWideFloats != wideFloats) || (nodeCost && numNodeCost != dev->totalNodes) || (pairFlags && numPairFlags != dev->totalTriangles))
    return refuse(TWK_ERROR_INVALID_VALUE, "the arrays hold " + std::to_string(wideFloats) + " wide-node floats, " + std::to_string(dev->totalNodes) + " node costs and " + std::to_string(dev->totalTriangles) + " pair flags");
  HIP_TRY(hipStreamSynchronize(dev->stream));
  if (wide) HIP_TRY(hipMemcpy(wide, dev->d_wideNodes, sizeof(float) * wideFloats, hipMemcpyDeviceToHost));
  if (nodeCost) HIP_TRY(hipMemcpy(nodeCost, dev->d_nodeCost, sizeof(float) * dev->totalNodes, hipMemcpyDeviceToHost));
  if (pairFlags) HIP_TRY(hipMemcpy(pairFlags, dev->d_pairFlags, sizeof(int) * dev->totalTriangles, hipMemcpyDeviceToHost));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_read_kept_build")

int twk_debug_snapshot_scene(TwkDevice dev, void* launchParams, size_t paramsBytes)
try
{
  int rc = activate(dev, "twk_debug_snapshot_scene"); if (rc) return rc;
  if (!dev->built) return twkSetError(TWK_ERROR_INVALID_STATE, "twk_debug_snapshot_scene: twk_build has not been called");
  if (!launchParams || paramsBytes != sizeof(LaunchParams)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_snapshot_scene: paramsBytes must be sizeof(LaunchParams) = " + std::to_string(sizeof(LaunchParams)));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  refreshParams(dev);
  LaunchParams q = dev->params;
  dev->hostScene.clear();
  rc = TWK_SUCCESS;
  auto host = [&](const void* devicePointer, size_t bytes) -> const void*
  {
    if (!devicePointer || bytes == 0) return nullptr;
    dev->hostScene.emplace_back(bytes);
    if (hipMemcpy(dev->hostScene.back().data(), devicePointer, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = TWK_ERROR_HIP;
    return dev->hostScene.back().data();
  };
  q.nodes          = static_cast<const BvhNode*>(host(dev->d_nodes, sizeof(BvhNode) * dev->totalNodes));
  q.wideQ          = static_cast<const float4*>(host(dev->d_wideQ, sizeof(float4) * 4 * dev->wideNodesTotal));
  if (q.wideQ) canonicalLeafReferences(dev, dev->hostScene.back().data(), dev->wideNodesTotal);
  q.trianglePairs  = nullptr; // the host build walks the binary nodes and the slots
  q.topNodes       = static_cast<const float4*>(host(dev->d_topNodes, sizeof(float4) * 4 * TWK_TOP_NODES));
  q.topNodes7      = static_cast<const float4*>(host(dev->d_topNodes7, sizeof(float4) * 4 * TWK_TOP_NODES7));
  q.triangles      = static_cast<const float4*>(host(dev->d_triangles, sizeof(float4) * 3 * dev->totalTriangles));
  q.shadeTriangles = static_cast<const float4*>(host(dev->d_shadeTriangles, sizeof(float4) * TWK_SHADE_RECORD * dev->totalTriangles));
  q.instances      = static_cast<const DevInstance*>(host(dev->d_instances, sizeof(DevInstance) * dev->instances.size()));
  q.materials      = static_cast<const DevMaterial*>(host(dev->d_materials, sizeof(DevMaterial) * dev->materials.size()));
  q.lights         = static_cast<const DevLight*>(host(dev->d_lights, sizeof(DevLight) * dev->lights.size()));
  q.camera         = static_cast<const float*>(host(dev->d_camera, sizeof(float) * 12));
  q.attributes = nullptr; q.indices = nullptr; // build input only
  for (int k = 0; k < 3; ++k)
    q.textures[k].texels = static_cast<const float4*>(host(dev->d_texels[k], sizeof(float4) * (size_t) q.textures[k].width * (size_t) q.textures[k].height));
  q.envCDF_U = static_cast<const float*>(host(dev->d_envCDF_U, sizeof(float) * ((size_t) q.envWidth + 1) * q.envHeight));
  q.envCDF_V = static_cast<const float*>(host(dev->d_envCDF_V, sizeof(float) * ((size_t) q.envHeight + 1)));
  if (rc) return twkSetError(rc, "twk_debug_snapshot_scene: device-to-host copy failed");
  // streams, counters, outputs: the host build allocates its own
  q.tileEntries = nullptr; q.tilesX = 0;
#define TWK_STREAM_CLEAR(member, type, perPath, index) q.member = nullptr;
  TWK_PATH_STREAMS(TWK_STREAM_CLEAR) TWK_OPTIONAL_PATH_STREAMS(TWK_STREAM_CLEAR)
#undef TWK_STREAM_CLEAR
  q.aovAlbedo = nullptr; q.aovNormal = nullptr; q.moments = nullptr;
  q.output = nullptr; q.counters = nullptr; q.stats = nullptr; q.firstHit = nullptr; q.firstHitInstance = nullptr; q.traceStackSpill = nullptr;
  q.droppedPushes = nullptr;
  memcpy(launchParams, &q, sizeof(q));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_snapshot_scene")

int twk_debug_math(TwkDevice dev, int op, const float* x, const float* y, float* out, size_t n)
try
{
  int rc = activate(dev, "twk_debug_math"); if (rc) return rc;
  if (op < 0 || op > 9 || !x || !out || ((op == 3 || op == 9) && !y)) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_math: bad arguments");
  if (n == 0) return TWK_SUCCESS;
  DeviceArray<float> dx, dy, dout;
  if ((rc = dx.allocate(n))) return rc;
  if ((rc = dy.allocate(n))) return rc;
  if ((rc = dout.allocate(n))) return rc;
  HIP_TRY(hipMemcpyAsync(dx, x, n * sizeof(float), hipMemcpyHostToDevice, dev->stream));
  HIP_TRY(hipMemcpyAsync(dy, y ? y : x, n * sizeof(float), hipMemcpyHostToDevice, dev->stream));
  launchMathTap(op, dx, dy, dout, n, dev->stream);
  HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(float), hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_math")

int twk_debug_exact_division(TwkDevice dev, int mode, uint32_t first, uint64_t count, const float* x, const float* d,
                             uint64_t* mismatches, uint64_t* fallbacks, uint32_t offenders[16])
try
{
  int rc = activate(dev, "twk_debug_exact_division"); if (rc) return rc;
  if (mode < 0 || mode > 2 || !mismatches || !fallbacks || (mode == 1 && count && (!x || !d)) || (mode == 0 && count > ((uint64_t) 1 << 32)))
    return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_debug_exact_division: bad arguments");
  *mismatches = 0; *fallbacks = 0;
  if (offenders) memset(offenders, 0, 16 * sizeof(uint32_t));
  if (count == 0) return TWK_SUCCESS;
  DeviceArray<float> dx, dd;
  DeviceArray<unsigned long long> tally;
  if ((rc = tally.allocate(18, true, dev->stream))) return rc;
  if (mode == 1)
  {
    if ((rc = dx.allocate(count))) return rc;
    if ((rc = dd.allocate(count))) return rc;
    HIP_TRY(hipMemcpyAsync(dx, x, count * sizeof(float), hipMemcpyHostToDevice, dev->stream));
    HIP_TRY(hipMemcpyAsync(dd, d, count * sizeof(float), hipMemcpyHostToDevice, dev->stream));
  }
  launchExactDivisionTap(mode, first, count, dx, dd, tally, dev->stream);
  unsigned long long host[18];
  HIP_TRY(hipMemcpyAsync(host, tally, sizeof(host), hipMemcpyDeviceToHost, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream));
  *mismatches = host[0]; *fallbacks = host[1];
  if (offenders) for (int k = 0; k < 16; ++k) offenders[k] = (uint32_t) host[2 + k];
  return TWK_SUCCESS;
}
TWK_CATCH("twk_debug_exact_division")

} // extern "C"
