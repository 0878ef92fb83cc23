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

// trust: k.width x k.height floats, not nullptr
void launchTemporalCascadeTrusted(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, const float* trust, float4* layersOut,
                                  const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream)
{
  const size_t numPixels = (size_t) k.width * k.height;
  hipLaunchKernelGGL(temporalCascadeTrustedKernel, dim3((unsigned int) ((numPixels + 255) / 256)), dim3(256), 0, stream, layers, geometry, historyLayers, historyGeometry, trust,
                     layersOut, k, c);
}

// layers, layersOut and historyLayers [c.layers][k.width x k.height] float4; historyLayers / historyGeometry nullptr with k.hasHistory 0
void launchTemporalCascade(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, float4* layersOut,
                           const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream)
{
  const size_t numPixels = (size_t) k.width * k.height;
  hipLaunchKernelGGL(temporalCascadeKernel, dim3((unsigned int) ((numPixels + 255) / 256)), dim3(256), 0, stream, layers, geometry, historyLayers, historyGeometry, layersOut, k, c);
}

} // namespace twk
