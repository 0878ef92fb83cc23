// Kernel of twk_temporal_accumulate_cascade: the cascade's layers reprojected through the previous camera and added to the frame's,
// as temporal_cascade_device.h defines it. A stream plus four-tap gathers.
#include "temporal_cascade_device.h"

namespace twk {

// One thread per pixel. The projection, the four taps' validity and their weights are computed once and serve every layer; the
// layers are visited in ascending order. Per lane: the current geometry and K current layers are coalesced 16-byte loads, the K
// outputs coalesced 16-byte stores (layer-major: a wave touches 1 KiB of each layer), the history four neighbouring 16-byte gathers
// of the geometry and of each layer around the reprojected position — layers 0 and K-1 are fetched once, for their counts, and kept
// in registers for their sums. Neighbouring lanes reproject to neighbouring history pixels, so a wave's gathers fall into a few
// rows of cache lines. (A thread per (pixel, layer) would repeat the projection, the geometry gathers and the two count gathers
// K times: 12 extra 16-byte gathers per thread against the 4 it is there for.)
__global__ void __launch_bounds__(256) temporalCascadeKernel(const float4* __restrict__ layers, const float4* __restrict__ geometry, const float4* __restrict__ historyLayers,
                                                             const float4* __restrict__ historyGeometry, float4* __restrict__ layersOut, TemporalConstants k, CascadeConstants c)
{
  const size_t numPixels = (size_t) k.width * k.height;
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= numPixels) return;
  temporalCascadePixel(k, c, layers, geometry, historyLayers, historyGeometry, numPixels, p, layersOut);
}

// The trusted build (twk_temporal_accumulate_cascade_trusted): the same thread per pixel, plus one coalesced 4-byte load of the trust
// where the pixel has history. A kernel of its own, so that the one above is the code it was.
__global__ void __launch_bounds__(256) temporalCascadeTrustedKernel(const float4* __restrict__ layers, const float4* __restrict__ geometry, const float4* __restrict__ historyLayers,
                                                                    const float4* __restrict__ historyGeometry, const float* __restrict__ trust, float4* __restrict__ layersOut,
                                                                    TemporalConstants k, CascadeConstants c)
{
  const size_t numPixels = (size_t) k.width * k.height;
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= numPixels) return;
  temporalCascadePixel<true>(k, c, layers, geometry, historyLayers, historyGeometry, numPixels, p, layersOut, trust);
}

// The Moving builds of the two kernels above (temporal_motion_device.h): the same thread per pixel, plus one 64-byte record of the
// table per candidate pixel, read before the projection; Staged: from the block's LDS copy (motionTable). Kernels of their own, so
// that the two above are the code they were.
template<bool Trusted, bool Staged>
__global__ void __launch_bounds__(256) temporalCascadeMovingKernel(const float4* __restrict__ layers, const float4* __restrict__ geometry, const float4* __restrict__ historyLayers,
                                                                   const float4* __restrict__ historyGeometry, const float* __restrict__ trust,
                                                                   const TwkInstanceMotion* __restrict__ motion, unsigned int numMotion, float4* __restrict__ layersOut,
                                                                   TemporalConstants k, CascadeConstants c)
{
  __shared__ TwkInstanceMotion staged[Staged ? TWK_MOTION_LDS_RECORDS : 1];
  const TwkInstanceMotion* table = motionTable<Staged>(motion, numMotion, staged, 256u);
  const size_t numPixels = (size_t) k.width * k.height;
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= numPixels) return;
  temporalCascadePixel<Trusted, true>(k, c, layers, geometry, historyLayers, historyGeometry, numPixels, p, layersOut, trust, table, numMotion);
}

// The Carried builds (temporal_carry_device.h): the same thread per pixel, plus one coalesced 16-byte read of the previous-position
// plane where the pixel is a candidate; no table. Kernels of their own, so that the ones above are the code they were.
template<bool Trusted>
__global__ void __launch_bounds__(256) temporalCascadeCarriedKernel(const float4* __restrict__ layers, const float4* __restrict__ geometry, const float4* __restrict__ historyLayers,
                                                                    const float4* __restrict__ historyGeometry, const float* __restrict__ trust, const float4* __restrict__ plane,
                                                                    float4* __restrict__ layersOut, TemporalConstants k, CascadeConstants c)
{
  const size_t numPixels = (size_t) k.width * k.height;
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= numPixels) return;
  temporalCascadePixel<Trusted, false, true>(k, c, layers, geometry, historyLayers, historyGeometry, numPixels, p, layersOut, trust, nullptr, 0u, plane);
}

template<bool Trusted>
static void launchCascadeCarried(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, const float* trust, const float4* plane,
                                 float4* layersOut, const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream)
{
  const size_t numPixels = (size_t) k.width * k.height;
  hipLaunchKernelGGL(temporalCascadeCarriedKernel<Trusted>, dim3((unsigned int) ((numPixels + 255) / 256)), dim3(256), 0, stream, layers, geometry, historyLayers, historyGeometry, trust,
                     plane, layersOut, k, c);
}

template<bool Trusted>
static void launchCascadeMoving(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, const float* trust,
                                const TwkInstanceMotion* motion, unsigned int numMotion, float4* layersOut, const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream)
{
  const size_t numPixels = (size_t) k.width * k.height;
  const dim3 grid((unsigned int) ((numPixels + 255) / 256));
#if TWK_MOTION_STAGED_RECORDS > 0
  if (numMotion <= TWK_MOTION_STAGED_RECORDS)
  {
    hipLaunchKernelGGL((temporalCascadeMovingKernel<Trusted, true>), grid, dim3(256), 0, stream, layers, geometry, historyLayers, historyGeometry, trust, motion, numMotion, layersOut, k, c);
    return;
  }
#endif
  hipLaunchKernelGGL((temporalCascadeMovingKernel<Trusted, false>), grid, dim3(256), 0, stream, layers, geometry, historyLayers, historyGeometry, trust, motion, numMotion, layersOut, k, c);
}

// trust: k.width x k.height floats, not nullptr. motion, numMotion: the table of the Moving build; nullptr or 0: the kernel above
void launchTemporalCascadeTrusted(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, const float* trust, float4* layersOut,
                                  const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream, const TwkInstanceMotion* motion, unsigned int numMotion, const float4* carried)
{
  if (carried) { launchCascadeCarried<true>(layers, geometry, historyLayers, historyGeometry, trust, carried, layersOut, k, c, stream); return; }
  if (motion && numMotion > 0u) { launchCascadeMoving<true>(layers, geometry, historyLayers, historyGeometry, trust, motion, numMotion, layersOut, k, c, stream); return; }
  const size_t numPixels = (size_t) k.width * k.height;
  hipLaunchKernelGGL(temporalCascadeTrustedKernel, dim3((unsigned int) ((numPixels + 255) / 256)), dim3(256), 0, stream, layers, geometry, historyLayers, historyGeometry, trust,
                     layersOut, k, c);
}

// layers, layersOut and historyLayers [c.layers][k.width x k.height] float4; historyLayers / historyGeometry nullptr with k.hasHistory 0.
// motion, numMotion: the table of the Moving build; nullptr or 0: the kernel above
void launchTemporalCascade(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, float4* layersOut,
                           const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream, const TwkInstanceMotion* motion, unsigned int numMotion, const float4* carried)
{
  if (carried) { launchCascadeCarried<false>(layers, geometry, historyLayers, historyGeometry, nullptr, carried, layersOut, k, c, stream); return; }
  if (motion && numMotion > 0u) { launchCascadeMoving<false>(layers, geometry, historyLayers, historyGeometry, nullptr, motion, numMotion, layersOut, k, c, stream); return; }
  const size_t numPixels = (size_t) k.width * k.height;
  hipLaunchKernelGGL(temporalCascadeKernel, dim3((unsigned int) ((numPixels + 255) / 256)), dim3(256), 0, stream, layers, geometry, historyLayers, historyGeometry, layersOut, k, c);
}

} // namespace twk
