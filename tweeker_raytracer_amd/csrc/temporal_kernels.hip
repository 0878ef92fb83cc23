// Kernels of twk_render_geometry, twk_render_geometry_tile and twk_temporal_accumulate: the geometry AOV and the temporal merge defined in temporal_device.h.
#include "temporal_device.h"
#include "trace_device.h"
#include "shade_device.h" // distribute(): the pixel column of a launch index
#include "temporal_store.h"

namespace twk {

// One closest-hit ray through the centre of every pixel with the single-ray traversal (the routine, LDS stack and spill of
// traceQueryKernel; the grid is at most numCUs x TWK_TRACE_WAVES blocks, within the per-lane spill stacks). Tiled = false: the
// handle's buffer is the picture, element i is pixel i. Tiled = true (twk_render_geometry_tile on a packed tile buffer): element i
// is launch index (lx, ly) of launchWidth x height, its pixel column is distribute(lx, ly), and padding (x >= width) is written as
// a miss without a ray. A build of its own, so that the single-device kernel is the code it was.
template<bool Tiled>
__global__ void __launch_bounds__(TWK_TRACE_BLOCK)
geometryKernel(LaunchParams p, float4* __restrict__ geometry)
{
  __shared__ int stackStorage[TWK_TRACE_STACK_LDS * TWK_TRACE_BLOCK];
  int* ldsStack = stackStorage + threadIdx.x;
  int* spill = p.traceStackSpill + (size_t) (blockIdx.x * blockDim.x + threadIdx.x) * TWK_TRACE_STACK_SPILL;
  unsigned int n0 = 0, n1 = 0, n2 = 0;
  const unsigned int columns = (unsigned int) (Tiled ? p.launchWidth : p.resolution[0]);
  const unsigned int numPixels = columns * (unsigned int) p.resolution[1];
  const float* cam = p.camera;
  const V3 P = v3(cam[0], cam[1], cam[2]);
  for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < numPixels; i += gridDim.x * blockDim.x)
  {
    int x = (int) (i % columns);
    const int y = (int) (i / columns);
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (Tiled)
    {
      x = (int) distribute(p, (unsigned int) x, (unsigned int) y);
      if (x >= p.resolution[0]) { geometry[i] = g; continue; }
    }
    const V3 d = centreRay(cam, x, y, p.resolution[0], p.resolution[1]);
    TraceResult res;
    traverse<false>(p, P, d, p.sceneEpsilon, RT_DEFAULT_MAX, false, ldsStack, spill, res, n0, n1, n2);
    if (res.instance >= 0)
      g = make_float4(P.x + res.t * d.x, P.y + res.t * d.y, P.z + res.t * d.z, __uint_as_float((unsigned int) res.instance + 1u));
    geometry[i] = g;
  }
}

// One thread per pixel. The current frame's three streams and the three outputs are coalesced 16-byte (RGBA16F: 8-byte) accesses;
// the history is four neighbouring 16-byte gathers per stream around the reprojected position, the geometry first: colour and
// moments are fetched only at the taps that belong to the surface.
template<typename Pixel>
__global__ void __launch_bounds__(256) temporalKernel(const Pixel* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ geometry,
                                                      const float4* __restrict__ historyColour, const float4* __restrict__ historyMoments, const float4* __restrict__ historyGeometry,
                                                      Pixel* __restrict__ colourOut, float4* __restrict__ historyOut, float4* __restrict__ momentsOut, TemporalConstants k)
{
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  const Pixel raw = colour[p];
  const float4 cur = widen(raw);
  const float4 mc = moments[p];
  const float4 g = geometry[p];
  TemporalSums s;
  temporalGather(k, cur, mc, g, historyColour, historyMoments, historyGeometry, s);
  if (s.ws > 0.0f)
  {
    float4 c, m;
    temporalMerge(k, s, cur, mc, c, m);
    temporalStoreMerged(p, c, m, colourOut, historyOut, momentsOut);
  }
  else
    temporalStorePassThrough(p, raw, cur, mc, colourOut, historyOut, momentsOut);
}

// temporalKernel's Moving build (temporal_motion_device.h): the same thread per pixel and the same streams, plus one 64-byte record
// of the table per candidate pixel, read before the projection — a wave's pixels see one or two instances, so its loads fall into
// one or two cache lines. Staged: the table from the block's LDS copy (motionTable). A kernel of its own, so that the one above is
// the code it was.
template<typename Pixel, bool Staged>
__global__ void __launch_bounds__(256) temporalMovingKernel(const Pixel* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ geometry,
                                                            const float4* __restrict__ historyColour, const float4* __restrict__ historyMoments, const float4* __restrict__ historyGeometry,
                                                            const TwkInstanceMotion* __restrict__ motion, unsigned int numMotion,
                                                            Pixel* __restrict__ colourOut, float4* __restrict__ historyOut, float4* __restrict__ momentsOut, TemporalConstants k)
{
  __shared__ TwkInstanceMotion staged[Staged ? TWK_MOTION_LDS_RECORDS : 1];
  const TwkInstanceMotion* table = motionTable<Staged>(motion, numMotion, staged, 256u);
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  const Pixel raw = colour[p];
  const float4 cur = widen(raw);
  const float4 mc = moments[p];
  const float4 g = geometry[p];
  TemporalSums s;
  temporalGather<true>(k, cur, mc, g, historyColour, historyMoments, historyGeometry, s, table, numMotion);
  if (s.ws > 0.0f)
  {
    float4 c, m;
    temporalMerge(k, s, cur, mc, c, m);
    temporalStoreMerged(p, c, m, colourOut, historyOut, momentsOut);
  }
  else
    temporalStorePassThrough(p, raw, cur, mc, colourOut, historyOut, momentsOut);
}

// temporalKernel's Carried build (temporal_carry_device.h): the same thread per pixel and the same streams, plus one coalesced 16-byte
// read of the previous-position plane per pixel; no table. A kernel of its own, so that the ones above are the code they were.
template<typename Pixel>
__global__ void __launch_bounds__(256) temporalCarriedKernel(const Pixel* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ geometry,
                                                             const float4* __restrict__ historyColour, const float4* __restrict__ historyMoments, const float4* __restrict__ historyGeometry,
                                                             const float4* __restrict__ plane, Pixel* __restrict__ colourOut, float4* __restrict__ historyOut, float4* __restrict__ momentsOut,
                                                             TemporalConstants k)
{
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  const Pixel raw = colour[p];
  const float4 cur = widen(raw);
  const float4 mc = moments[p];
  const float4 g = geometry[p];
  TemporalSums s;
  temporalGather<false, true>(k, cur, mc, g, historyColour, historyMoments, historyGeometry, s, nullptr, 0u, plane[p]);
  if (s.ws > 0.0f)
  {
    float4 c, m;
    temporalMerge(k, s, cur, mc, c, m);
    temporalStoreMerged(p, c, m, colourOut, historyOut, momentsOut);
  }
  else
    temporalStorePassThrough(p, raw, cur, mc, colourOut, historyOut, momentsOut);
}

template<typename Pixel, bool Staged>
static void launchMoving(const void* colour, const float4* moments, const float4* geometry, const float4* historyColour, const float4* historyMoments, const float4* historyGeometry,
                         const TwkInstanceMotion* motion, unsigned int numMotion, void* colourOut, float4* historyOut, float4* momentsOut, const TemporalConstants& k, hipStream_t stream)
{
  const size_t numPixels = (size_t) k.width * k.height;
  hipLaunchKernelGGL((temporalMovingKernel<Pixel, Staged>), dim3((unsigned int) ((numPixels + 255) / 256)), dim3(256), 0, stream, static_cast<const Pixel*>(colour), moments, geometry,
                     historyColour, historyMoments, historyGeometry, motion, numMotion, static_cast<Pixel*>(colourOut), historyOut, momentsOut, k);
}

void launchGeometry(const LaunchParams& p, float4* geometry, bool tiled, int gridBlocks, hipStream_t stream)
{
  if (tiled) hipLaunchKernelGGL(geometryKernel<true>, dim3(gridBlocks), dim3(TWK_TRACE_BLOCK), 0, stream, p, geometry);
  else       hipLaunchKernelGGL(geometryKernel<false>, dim3(gridBlocks), dim3(TWK_TRACE_BLOCK), 0, stream, p, geometry);
}

void launchTemporal(const void* colour, bool half, const float4* moments, const float4* geometry, const float4* historyColour, const float4* historyMoments,
                    const float4* historyGeometry, void* colourOut, float4* historyOut, float4* momentsOut, const TemporalConstants& k, hipStream_t stream,
                    const TwkInstanceMotion* motion, unsigned int numMotion, const float4* carried)
{
  if (carried) // the Carried build: g' from the plane, no table
  {
    const size_t pixels = (size_t) k.width * k.height;
    const dim3 blocks((unsigned int) ((pixels + 255) / 256));
    if (half)
      hipLaunchKernelGGL(temporalCarriedKernel<Half4>, blocks, dim3(256), 0, stream, static_cast<const Half4*>(colour), moments, geometry, historyColour, historyMoments, historyGeometry,
                         carried, static_cast<Half4*>(colourOut), historyOut, momentsOut, k);
    else
      hipLaunchKernelGGL(temporalCarriedKernel<float4>, blocks, dim3(256), 0, stream, static_cast<const float4*>(colour), moments, geometry, historyColour, historyMoments, historyGeometry,
                         carried, static_cast<float4*>(colourOut), historyOut, momentsOut, k);
    return;
  }
  if (motion && numMotion > 0u) // the Moving build; without a table the kernel below, as it always was
  {
#if TWK_MOTION_STAGED_RECORDS > 0
    if (numMotion <= TWK_MOTION_STAGED_RECORDS)
    {
      if (half) launchMoving<Half4, true>(colour, moments, geometry, historyColour, historyMoments, historyGeometry, motion, numMotion, colourOut, historyOut, momentsOut, k, stream);
      else      launchMoving<float4, true>(colour, moments, geometry, historyColour, historyMoments, historyGeometry, motion, numMotion, colourOut, historyOut, momentsOut, k, stream);
      return;
    }
#endif
    if (half) launchMoving<Half4, false>(colour, moments, geometry, historyColour, historyMoments, historyGeometry, motion, numMotion, colourOut, historyOut, momentsOut, k, stream);
    else      launchMoving<float4, false>(colour, moments, geometry, historyColour, historyMoments, historyGeometry, motion, numMotion, colourOut, historyOut, momentsOut, k, stream);
    return;
  }
  const size_t numPixels = (size_t) k.width * k.height;
  const dim3 grid((unsigned int) ((numPixels + 255) / 256));
  if (half)
    hipLaunchKernelGGL(temporalKernel<Half4>, grid, dim3(256), 0, stream, static_cast<const Half4*>(colour), moments, geometry, historyColour, historyMoments, historyGeometry,
                       static_cast<Half4*>(colourOut), historyOut, momentsOut, k);
  else
    hipLaunchKernelGGL(temporalKernel<float4>, grid, dim3(256), 0, stream, static_cast<const float4*>(colour), moments, geometry, historyColour, historyMoments, historyGeometry,
                       static_cast<float4*>(colourOut), historyOut, momentsOut, k);
}

} // namespace twk
