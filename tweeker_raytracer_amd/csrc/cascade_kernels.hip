// Kernels of twk_cascade_resolve: the resolve of the firefly cascade defined in cascade_device.h, in two launches. The first turns
// every layer of every element into its luminance lambda, an f32 stream [K][width x height]; the second computes the resolve per
// pixel from lambda (9 taps x K layers, 4 B each, neighbouring lanes share them in the cache), the pixel's own K layers and n. Stream
// order is the only dependency: no block waits for another. The fold is not here: it is the CASCADE build of the accumulate kernels
// (shade_kernels.hip).
#include "cascade_device.h"
#include "pixel_formats.h"

namespace twk {

// One thread per element of [K][numElements]: a coalesced 16 B load and a coalesced 4 B store per lane
__global__ void __launch_bounds__(256) cascadeLambdaKernel(const float4* __restrict__ layers, float* __restrict__ lambda, size_t total)
{
  const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  lambda[i] = cascadeLambda(layers[i]);
}

// One thread per pixel, rows of the grid along the lanes
template<typename Pixel>
__global__ void __launch_bounds__(256) cascadeResolveKernel(CascadeConstants k, float kappa, const float4* __restrict__ layers, const float* __restrict__ lambda,
                                                            int width, int height, Pixel* __restrict__ out)
{
  const size_t numPixels = (size_t) width * height;
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= numPixels) return;
  const int y = (int) (p / (size_t) width), x = (int) (p - (size_t) y * width);
  out[p] = pixelOf<Pixel>(cascadeResolvePixel(k, kappa, layers, lambda, numPixels, width, height, x, y));
}

// layers [k.layers][width x height] float4, lambda k.layers x width x height floats of scratch, resolved
// width x height pixels, Half4 when `half`
void launchCascadeResolve(const CascadeConstants& k, float kappa, const float4* layers, float* lambda, int width, int height, void* resolved, bool half, hipStream_t stream)
{
  const size_t numPixels = (size_t) width * height, total = numPixels * (size_t) k.layers;
  hipLaunchKernelGGL(cascadeLambdaKernel, dim3((unsigned int) ((total + 255) / 256)), dim3(256), 0, stream, layers, lambda, total);
  const dim3 grid((unsigned int) ((numPixels + 255) / 256));
  if (half) hipLaunchKernelGGL(cascadeResolveKernel<Half4>, grid, dim3(256), 0, stream, k, kappa, layers, lambda, width, height, static_cast<Half4*>(resolved));
  else      hipLaunchKernelGGL(cascadeResolveKernel<float4>, grid, dim3(256), 0, stream, k, kappa, layers, lambda, width, height, static_cast<float4*>(resolved));
}

} // namespace twk
