// ORACLE-SIDE TEST INFRASTRUCTURE — not part of the product, never linked into libtweeker_hip.so.
//
// Host build of the product's kernels: BASELINE.json north_star's "single-threaded C++ CPU fallback of the same kernels
// timed on the host cores". The SAME source the GPU runs — tweeker_raytracer_amd/csrc/shade_device.h (generatePath,
// shadePath with every BSDF / light / miss program, accumulateLaunchIndex), trace_device.h (traverse: the single-ray
// two-level traversal of the overflow, query and tail kernels, slab test, watertight triangle test), device_math.h —
// compiled by g++ with -ffp-contract=off (host_kernels_shim.h supplies the dozen device intrinsics), driven as the same
// wavefront: generate -> [trace -> shade] x depth -> trace -> accumulate over the same SoA queues, on the BVH the DEVICE
// built (twk_debug_snapshot_scene). What is not the same source is what cannot exist on a CPU: the persistent kernel's
// wave-level ray dealing and while-while loop (every ray is walked by traverse() instead — same hits by construction of
// the tie rule, tests/test_gpu_host_kernels.py holds the images equal bit for bit) and the block-aggregated queue
// appends (a plain sequential append: another queue order, the same paths).
// The records between the stages are read and written by the product's own path_queue.h, in its full form (no packed queue,
// no slim streams: the pool below carves every stream).
// Used by tests (-m gpu: it needs a device-built scene) and by bench.py's cpu_baseline leg, never by the product.
#include "host_kernels_shim.h"
#include "../tweeker_raytracer_amd/csrc/shade_device.h"
#include "../tweeker_raytracer_amd/csrc/trace_device.h"

#include <chrono>
#include <vector>

using namespace twk;

extern "C" {

// launchParams: what twk_debug_snapshot_scene wrote. Renders iterations [firstIteration, firstIteration + batch) as ONE
// wavefront pass on the calling thread into `output` (launchWidth x height float4 running mean, read and written like
// the device's accumulation buffer). counts (may be null): radiance rays, shadow rays, node visits, triangle tests,
// instance entries, shaded segments. Returns 0, or 1 for bad arguments / a scene the host build does not cover.
int hostk_render(const void* launchParams, size_t paramsBytes, unsigned int firstIteration, int batch, float* output, double* seconds, unsigned long long* counts)
{
  if (!launchParams || paramsBytes != sizeof(LaunchParams) || !output || batch < 1) return 1;
  LaunchParams p;
  memcpy(&p, launchParams, sizeof(p));
  if (p.hasCutout) return 1; // the stochastic any-hit candidate loop lives in trace_kernels.hip (device only)
  const size_t numPixels = (size_t) p.numPixels, n = numPixels * (size_t) batch;
  const int maxDepth = p.pathLengths[1];

  // streams and counters of its own: the list and the bytes per path of device_types.h TWK_PATH_STREAMS, no padding (one segment per queue)
  std::vector<float4> pool((n * kPathStreamBytes + sizeof(float4) - 1) / sizeof(float4));
  carvePathStreams(p, pool.data(), n);
  std::vector<unsigned int> counters(TWK_COUNTERS_PER_DEPTH * (TWK_MAX_DEPTH + 2), 0u);
  p.counters = counters.data();
  unsigned int dropped = 0;
  p.droppedPushes = &dropped;
  p.output = reinterpret_cast<float4*>(output);
  p.outputFrame = 0;
  p.iterationIndex = firstIteration; p.batchCount = batch; p.numPaths = (int) n; p.pathBase = 0;

  std::vector<int> ldsStack((size_t) TWK_TRACE_STACK_LDS * TWK_TRACE_BLOCK, 0), spill(TWK_TRACE_STACK_SPILL, 0);
  unsigned int nodeCount = 0, triCount = 0, instCount = 0;
  unsigned long long radianceRays = 0, shadowRays = 0, nodes = 0, tris = 0, insts = 0, shaded = 0;
  const auto t0 = std::chrono::steady_clock::now();

  // generateKernel
  for (size_t index = 0; index < n; ++index) generatePath(p, (unsigned int) index);

  auto trace = [&](int depth)
  {
    // traceKernel's job for bounce `depth`: closest hits of queue depth & 1, then the shadow rays shade(depth - 1) emitted
    // (the host build appends in slot order to ONE segment of each queue — segment 0: device_types.h "queue segments")
    const unsigned int numClosest = p.counters[depth * TWK_COUNTERS_PER_DEPTH + TWK_COUNTER_CLOSEST];
    const unsigned int numShadow = (depth > 0) ? p.counters[(depth - 1) * TWK_COUNTERS_PER_DEPTH + TWK_COUNTER_SHADOW] : 0u;
    const int q = depth & 1;
    for (unsigned int slot = 0; slot < numClosest + numShadow; ++slot)
    {
      // one segment per queue: a slot is its own record
      const bool isShadow = !(slot < numClosest);
      const unsigned int record = isShadow ? slot - numClosest : slot;
      const QueuedRay ray = isShadow ? loadShadowRay(p, record) : loadClosestRay(p, q, record, false);
      TraceResult res;
      nodeCount = triCount = instCount = 0;
      traverse<true>(p, v3(ray.o), v3(ray.d), ray.o.w, ray.d.w, isShadow, ldsStack.data(), spill.data(), res, nodeCount, triCount, instCount);
      nodes += nodeCount; tris += triCount; insts += instCount;
      if (isShadow) ++shadowRays; else ++radianceRays;
      // the hit record, or a visible shadow ray's pending contribution: what both trace kernels leave behind
      storeRayResult<false>(p, depth, /* primary */ false, /* packed */ false, /* slim */ false, slot, isShadow, res, 0u, [&]() { return record; });
    }
  };

  for (int depth = 0; depth < maxDepth; ++depth)
  {
    trace(depth);
    // shadeKernel: shadePath per queue slot, continuation and shadow rays appended in slot order
    const unsigned int numRays = p.counters[depth * TWK_COUNTERS_PER_DEPTH + TWK_COUNTER_CLOSEST];
    const int q = depth & 1, qn = q ^ 1;
    unsigned int& nextCount = p.counters[(depth + 1) * TWK_COUNTERS_PER_DEPTH + TWK_COUNTER_CLOSEST];
    unsigned int& shadowCount = p.counters[depth * TWK_COUNTERS_PER_DEPTH + TWK_COUNTER_SHADOW];
    for (unsigned int slot = 0; slot < numRays; ++slot)
    {
      float4 ro, rd, hit;
      unsigned int pixel;
      int instanceIndex;
      ShadeOutput out;
      out.alive = false; out.wantShadow = false;
      loadQueuedPath(p, q, slot, false, ro, rd, out.throughputPdf, out.seedFlags, pixel);
      if (!(rd.w >= 0.0f)) continue; // an inactive launch index (tile column beyond the image)
      loadHit(p, slot, false, hit, instanceIndex);
      shadePath<true, true>(p, depth, pixel, ro, rd, hit, instanceIndex, out);
      ++shaded;
      if (out.wantShadow) storeShadowRay(p, shadowCount++, false, out.nextPos, out.shadowDir, out.shadowTmax, out.pending, pixel, out.shadowSeed);
      if (out.alive) storeContinuation(p, qn, nextCount++, false, out.nextPos, out.nextDir, pixel, out.seedFlags, out.throughputPdf);
    }
  }
  if (maxDepth > 0) trace(maxDepth); // the shadow rays of the last shade

  // accumulateKernel
  for (size_t index = 0; index < numPixels; ++index) accumulateLaunchIndex(p, (unsigned int) index);

  if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (counts) { counts[0] = radianceRays; counts[1] = shadowRays; counts[2] = nodes; counts[3] = tris; counts[4] = insts; counts[5] = shaded; }
  return dropped ? 1 : 0;
}

size_t hostk_params_bytes(void) { return sizeof(LaunchParams); }

} // extern "C"
