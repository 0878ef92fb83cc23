// Kernels of twk_denoise, twk_denoise_variance and twk_denoise_variance_sampled: the edge-avoiding a-trous wavelet filter defined in denoise_device.h (prepare, the
// moments pass of the variance-guided mode, one launch per level, finish). Stands where Optix7Gui calls optixDenoiserInvoke (apps/Optix7Gui/src/Application.cpp:942-1001).
// What a pixel does in a pass is written once, in denoise_device.h (denoisePreparePixel, denoiseMomentsPixel, denoiseLevelPixel, denoiseFinishPixel); a kernel here is
// index arithmetic, staging where it stages, a tap source and one call.
#include "denoise_device.h"
#include "pixel_formats.h"
#include "../../include/tweeker_hip.h"
#include <type_traits>

namespace twk {

// The level exists in two builds that call the one body denoiseLevelPixel and differ in where it finds its taps, so they compute
// the same bits; twk_denoise picks one per level by its step (the LDS-staged build is faster at steps 1, 2 and 4,
// the direct-load build from step 8 on).
//
// Direct-load build: a block is a 32 x 8 pixel tile, a wave two rows of 32 pixels: every tap of a wave is two runs of 512
// contiguous bytes per stream, whatever the step. What a level reads beyond its one compulsory float4 per stream and pixel (24 of
// 25 taps) comes out of L2 / Infinity Cache: neighbouring lanes, rows and blocks read the same lines.
#define TWK_DENOISE_TILE_X 32
#define TWK_DENOISE_TILE_Y 8

template<typename Pixel>
__global__ void __launch_bounds__(256) denoisePrepareKernel(const Pixel* __restrict__ beauty, const Pixel* __restrict__ albedo, const Pixel* __restrict__ normal,
                                                            float4* __restrict__ colour, float4* __restrict__ guideNormal, float4* __restrict__ guideAlbedo,
                                                            DenoiseConstants k)
{
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  denoisePreparePixel(k, p, beauty, albedo, normal, colour, guideNormal, guideAlbedo);
}

// VAR: the level of the variance-guided mode (denoise_device.h): luminance edge-stop scaled by the 3 x 3 binomial of the variance in
// in[].w at the level's own step (the inner 3 x 3 of the taps the level loads anyway), the variance filtered along into out[].w
// GEO: the geometry guide (denoise_device.h; KIND 2 only): one more 16-byte stream per tap, read where the caller keeps it; the
// centre's normal and invG once per thread. The GEO = false builds read neither of the two last arguments.
template<int KIND, bool VAR, bool GEO>
__global__ void __launch_bounds__(256) denoiseLevelKernel(const float4* __restrict__ in, const float4* __restrict__ guideNormal, const float4* __restrict__ guideAlbedo,
                                                          float4* __restrict__ out, DenoiseConstants k, int step, const float4* __restrict__ geometry, DenoiseGeometryConstants g)
{
  const int x = (int) blockIdx.x * TWK_DENOISE_TILE_X + (int) (threadIdx.x % TWK_DENOISE_TILE_X);
  const int y = (int) blockIdx.y * TWK_DENOISE_TILE_Y + (int) (threadIdx.x / TWK_DENOISE_TILE_X);
  if (x >= k.width || y >= k.height) return;
  const DenoiseGlobalTaps taps(in, guideNormal, guideAlbedo, geometry, k.width, k.height, x, y, step);
  out[taps.centre] = denoiseLevelPixel<KIND, VAR, GEO>(k, g, taps);
}

// LDS-staged build: the same level with the block's taps staged in LDS. A block takes 32 x 8 pixels of ONE residue class modulo the step — pixels
// (rx + step i, ry + step j) — so that its taps are a dense 5 x 5 again and the staged region is the tile plus a halo of 2 in
// every direction, 36 x 12 = 432 pixels per 256, whatever the step (at step 1 this is the plain tile with its halo). Pixels
// outside the picture are staged with a NaN colour, which denoiseTap skips like any non-finite tap: the body is
// denoiseLevelKernel's, so are the bits (tests/test_gpu_denoise.py runs every case with every level on either build).
// The staging loads of a wave are 32-pixel runs with a stride of `step` pixels: at step >= 8 every lane reads a 128-byte line of
// its own, which is where this build stops paying.
#define TWK_DENOISE_LDS_X (TWK_DENOISE_TILE_X + 4)
#define TWK_DENOISE_LDS_Y (TWK_DENOISE_TILE_Y + 4)
// GEO: the geometry is staged as a fourth 36 x 12 array (27.6 KB per block instead of 20.7); outside the picture it is staged as a
// miss, and the tap is skipped for its NaN colour before the geometry is looked at.
template<int KIND, bool VAR, bool GEO>
__global__ void __launch_bounds__(256) denoiseLevelLdsKernel(const float4* __restrict__ in, const float4* __restrict__ guideNormal, const float4* __restrict__ guideAlbedo,
                                                             float4* __restrict__ out, DenoiseConstants k, int step, const float4* __restrict__ geometry, DenoiseGeometryConstants g)
{
  constexpr int STAGED = TWK_DENOISE_LDS_X * TWK_DENOISE_LDS_Y;
  __shared__ float4 colour[STAGED];
  __shared__ float4 normal[KIND >= 2 ? STAGED : 1];
  __shared__ float4 albedo[KIND >= 1 ? STAGED : 1];
  __shared__ float4 position[GEO ? STAGED : 1];
  const int rx = (int) blockIdx.x % step, tx = (int) blockIdx.x / step;
  const int ry = (int) blockIdx.y % step, ty = (int) blockIdx.y / step;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int i = (int) threadIdx.x; i < STAGED; i += 256)
  {
    const int gx = rx + (tx * TWK_DENOISE_TILE_X - 2 + i % TWK_DENOISE_LDS_X) * step;
    const int gy = ry + (ty * TWK_DENOISE_TILE_Y - 2 + i / TWK_DENOISE_LDS_X) * step;
    float4 c = make_float4(asFloat(0x7fc00000u), 0.0f, 0.0f, 0.0f), n = zero, a = zero, gg = zero;
    if (gx >= 0 && gx < k.width && gy >= 0 && gy < k.height)
    {
      const size_t q = (size_t) gy * k.width + gx;
      c = in[q];
      if (KIND >= 2) n = guideNormal[q];
      if (KIND >= 1) a = guideAlbedo[q];
      if (GEO) gg = geometry[q];
    }
    colour[i] = c;
    if (KIND >= 2) normal[i] = n;
    if (KIND >= 1) albedo[i] = a;
    if (GEO) position[i] = gg;
  }
  __syncthreads();
  const int lx = (int) (threadIdx.x % TWK_DENOISE_TILE_X), ly = (int) (threadIdx.x / TWK_DENOISE_TILE_X);
  const int x = rx + (tx * TWK_DENOISE_TILE_X + lx) * step;
  const int y = ry + (ty * TWK_DENOISE_TILE_Y + ly) * step;
  if (x >= k.width || y >= k.height) return;
  const size_t p = (size_t) y * k.width + x;
  const int centre = (ly + 2) * TWK_DENOISE_LDS_X + lx + 2; // an array the build does not use has one entry
  const DenoiseStagedTaps<TWK_DENOISE_LDS_X, float4> taps = {colour + centre, normal + (KIND >= 2 ? centre : 0), albedo + (KIND >= 1 ? centre : 0), position + (GEO ? centre : 0)};
  out[p] = denoiseLevelPixel<KIND, VAR, GEO>(k, g, taps);
}

// Moments pass of the variance-guided mode (denoise_device.h): 48 dense taps around every pixel, so the block's 32 x 8 tile is
// staged with a halo of 3, 38 x 14 = 532 pixels per 256: of the colour only its luminance (one float; NaN where the colour is not
// finite or the pixel lies outside the picture, which is what a tap is skipped for: the luminance of a finite colour is never NaN),
// and the guides in use. The centre's own colour is one coalesced global load. Writes the clamped colour and the variance (.w) to
// another stream: neighbours read the unclamped value.
#define TWK_DENOISE_MOMENTS_X (TWK_DENOISE_TILE_X + 2 * TWK_DENOISE_MOMENTS_RADIUS)
#define TWK_DENOISE_MOMENTS_Y (TWK_DENOISE_TILE_Y + 2 * TWK_DENOISE_MOMENTS_RADIUS)
// SAMPLED (twk_denoise_variance_sampled): one more coalesced load per pixel, its luminance moments (mean, M2, n, .) as the
// accumulate kernels fold them; momentsFinish writes the measured variance of the pixel's mean where n >= minSamples.
// GEO: the geometry guide, staged beside the other guides (8.5 KB more); the GEO = false builds read neither of the two last arguments
template<int KIND, bool SAMPLED, bool GEO>
__global__ void __launch_bounds__(256) denoiseMomentsKernel(const float4* __restrict__ in, const float4* __restrict__ guideNormal, const float4* __restrict__ guideAlbedo,
                                                            float4* __restrict__ out, DenoiseConstants k, const float4* __restrict__ sampled, float minSamples,
                                                            const float4* __restrict__ geometry, DenoiseGeometryConstants g)
{
  constexpr int STAGED = TWK_DENOISE_MOMENTS_X * TWK_DENOISE_MOMENTS_Y;
  __shared__ float  lum[STAGED];
  __shared__ float4 normal[KIND >= 2 ? STAGED : 1];
  __shared__ float4 albedo[KIND >= 1 ? STAGED : 1];
  __shared__ float4 position[GEO ? STAGED : 1];
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int x0 = (int) blockIdx.x * TWK_DENOISE_TILE_X, y0 = (int) blockIdx.y * TWK_DENOISE_TILE_Y;
  for (int i = (int) threadIdx.x; i < STAGED; i += 256)
  {
    const int gx = x0 - TWK_DENOISE_MOMENTS_RADIUS + i % TWK_DENOISE_MOMENTS_X;
    const int gy = y0 - TWK_DENOISE_MOMENTS_RADIUS + i / TWK_DENOISE_MOMENTS_X;
    float l = asFloat(0x7fc00000u);
    float4 n = zero, a = zero, gg = zero;
    if (gx >= 0 && gx < k.width && gy >= 0 && gy < k.height)
    {
      const size_t q = (size_t) gy * k.width + gx;
      const float4 c = in[q];
      if (finite3(c)) l = luminance(c);
      if (KIND >= 2) n = guideNormal[q];
      if (KIND >= 1) a = guideAlbedo[q];
      if (GEO) gg = geometry[q];
    }
    lum[i] = l;
    if (KIND >= 2) normal[i] = n;
    if (KIND >= 1) albedo[i] = a;
    if (GEO) position[i] = gg;
  }
  __syncthreads();
  const int lx = (int) (threadIdx.x % TWK_DENOISE_TILE_X), ly = (int) (threadIdx.x / TWK_DENOISE_TILE_X);
  const int x = x0 + lx, y = y0 + ly;
  if (x >= k.width || y >= k.height) return;
  const size_t p = (size_t) y * k.width + x;
  const int centre = (ly + TWK_DENOISE_MOMENTS_RADIUS) * TWK_DENOISE_MOMENTS_X + lx + TWK_DENOISE_MOMENTS_RADIUS;
  const DenoiseStagedTaps<TWK_DENOISE_MOMENTS_X, float> taps = {lum + centre, normal + (KIND >= 2 ? centre : 0), albedo + (KIND >= 1 ? centre : 0), position + (GEO ? centre : 0)};
  out[p] = denoiseMomentsPixel<KIND, SAMPLED, GEO>(k, g, taps, in[p], SAMPLED ? sampled + p : nullptr, minSamples);
}

template<typename Pixel>
__global__ void __launch_bounds__(256) denoiseFinishKernel(const Pixel* __restrict__ beauty, const float4* __restrict__ colour, const float4* __restrict__ guideNormal,
                                                           const float4* __restrict__ guideAlbedo, Pixel* __restrict__ denoised, DenoiseConstants k)
{
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  denoiseFinishPixel(k, p, beauty, colour, guideNormal, guideAlbedo, denoised);
}

static unsigned int pixelBlocks(const DenoiseConstants& k) { return (unsigned int) (((size_t) k.width * k.height + 255) / 256); }

// albedo / normal NULL: the kind does not use the guide
void launchDenoisePrepare(const void* beauty, const void* albedo, const void* normal, bool half, float4* colour, float4* guideNormal, float4* guideAlbedo,
                          const DenoiseConstants& k, hipStream_t stream)
{
  if (half) hipLaunchKernelGGL(denoisePrepareKernel<Half4>, dim3(pixelBlocks(k)), dim3(256), 0, stream, static_cast<const Half4*>(beauty), static_cast<const Half4*>(albedo),
                               static_cast<const Half4*>(normal), colour, guideNormal, guideAlbedo, k);
  else      hipLaunchKernelGGL(denoisePrepareKernel<float4>, dim3(pixelBlocks(k)), dim3(256), 0, stream, static_cast<const float4*>(beauty), static_cast<const float4*>(albedo),
                               static_cast<const float4*>(normal), colour, guideNormal, guideAlbedo, k);
}

// The builds of the level and of the moments pass: f(kind, geo), both compile-time constants. GEO builds exist for kind RGB_ALBEDO_NORMAL only
template<typename F>
static void withDenoiseBuild(int kind, bool geo, F f)
{
  using std::integral_constant;
  if (geo)                                         f(integral_constant<int, TWK_DENOISER_RGB_ALBEDO_NORMAL>(), std::true_type());
  else if (kind == TWK_DENOISER_RGB_ALBEDO_NORMAL) f(integral_constant<int, TWK_DENOISER_RGB_ALBEDO_NORMAL>(), std::false_type());
  else if (kind == TWK_DENOISER_RGB_ALBEDO)        f(integral_constant<int, TWK_DENOISER_RGB_ALBEDO>(), std::false_type());
  else                                             f(integral_constant<int, TWK_DENOISER_RGB>(), std::false_type());
}

template<int KIND, bool VAR, bool GEO>
static void launchDenoiseLevelOf(bool lds, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k, int step, hipStream_t stream,
                                 const float4* geometry, const DenoiseGeometryConstants& g)
{
  if (lds)
  {
    const dim3 ldsGrid(((k.width + step - 1) / step + TWK_DENOISE_TILE_X - 1) / TWK_DENOISE_TILE_X * step, ((k.height + step - 1) / step + TWK_DENOISE_TILE_Y - 1) / TWK_DENOISE_TILE_Y * step);
    hipLaunchKernelGGL((denoiseLevelLdsKernel<KIND, VAR, GEO>), ldsGrid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, step, geometry, g);
    return;
  }
  const dim3 grid((k.width + TWK_DENOISE_TILE_X - 1) / TWK_DENOISE_TILE_X, (k.height + TWK_DENOISE_TILE_Y - 1) / TWK_DENOISE_TILE_Y);
  hipLaunchKernelGGL((denoiseLevelKernel<KIND, VAR, GEO>), grid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, step, geometry, g);
}

// lds: the LDS-staged build of the level (one residue class modulo the step per block); variance: the level of the variance-guided mode
// geometry != NULL (kind RGB_ALBEDO_NORMAL only, the caller's check): the GEO builds, with the camera and sigma of *g (all zero without the guide)
void launchDenoiseLevel(int kind, bool lds, bool variance, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k, int step, hipStream_t stream,
                        const float4* geometry, const DenoiseGeometryConstants* g)
{
  withDenoiseBuild(kind, geometry != nullptr, [&](auto K, auto GEO)
  {
    if (variance) launchDenoiseLevelOf<decltype(K)::value, true, decltype(GEO)::value>(lds, in, guideNormal, guideAlbedo, out, k, step, stream, geometry, *g);
    else          launchDenoiseLevelOf<decltype(K)::value, false, decltype(GEO)::value>(lds, in, guideNormal, guideAlbedo, out, k, step, stream, geometry, *g);
  });
}

// the moments + firefly-clamp pass of the variance-guided mode, between prepare and level 0. sampled != NULL: the SAMPLED build —
// width x height luminance moments (mean, M2, n, .), whose measured variance stands in for the spatial one from minSamples samples on
// geometry != NULL (kind RGB_ALBEDO_NORMAL only): the GEO builds
void launchDenoiseMoments(int kind, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k,
                          const float4* sampled, float minSamples, hipStream_t stream, const float4* geometry, const DenoiseGeometryConstants* g)
{
  const dim3 grid((k.width + TWK_DENOISE_TILE_X - 1) / TWK_DENOISE_TILE_X, (k.height + TWK_DENOISE_TILE_Y - 1) / TWK_DENOISE_TILE_Y);
  withDenoiseBuild(kind, geometry != nullptr, [&](auto K, auto GEO)
  {
    if (sampled) hipLaunchKernelGGL((denoiseMomentsKernel<decltype(K)::value, true, decltype(GEO)::value>), grid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, sampled, minSamples, geometry, *g);
    else         hipLaunchKernelGGL((denoiseMomentsKernel<decltype(K)::value, false, decltype(GEO)::value>), grid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, sampled, 0.0f, geometry, *g);
  });
}

// guideNormal / guideAlbedo NULL: the kind does not use the guide
void launchDenoiseFinish(const void* beauty, bool half, const float4* colour, const float4* guideNormal, const float4* guideAlbedo, void* denoised, const DenoiseConstants& k, hipStream_t stream)
{
  if (half) hipLaunchKernelGGL(denoiseFinishKernel<Half4>, dim3(pixelBlocks(k)), dim3(256), 0, stream, static_cast<const Half4*>(beauty), colour, guideNormal, guideAlbedo, static_cast<Half4*>(denoised), k);
  else      hipLaunchKernelGGL(denoiseFinishKernel<float4>, dim3(pixelBlocks(k)), dim3(256), 0, stream, static_cast<const float4*>(beauty), colour, guideNormal, guideAlbedo, static_cast<float4*>(denoised), k);
}

} // namespace twk
