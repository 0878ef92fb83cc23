// Kernels of twk_denoise, twk_denoise_variance and twk_denoise_variance_sampled: the edge-avoiding a-trous wavelet filter defined in denoise_device.h (prepare, the
// moments pass of the variance-guided mode, one launch per level, finish). Stands where Optix7Gui calls optixDenoiserInvoke (apps/Optix7Gui/src/Application.cpp:942-1001).
#include "denoise_device.h"
#include "pixel_formats.h"
#include "../../include/tweeker_hip.h"

namespace twk {

// The level exists in two builds that compute the same bits; twk_denoise picks one per level by its step (the
// LDS-staged build is faster at steps 1, 2 and 4, the direct-load build from step 8 on).
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
  const float4 b = widen(beauty[p]);
  float4 c = b;
  if (albedo)
  {
    const float4 a = widen(albedo[p]);
    guideAlbedo[p] = make_float4(a.x, a.y, a.z, 0.0f);
    if (k.demodulate)
    {
      const float3 d = clampedAlbedo(a);
      c.x = b.x / d.x; c.y = b.y / d.y; c.z = b.z / d.z;
    }
  }
  if (normal)
  {
    const float4 n = widen(normal[p]);
    guideNormal[p] = make_float4(n.x, n.y, n.z, 0.0f);
  }
  colour[p] = c;
}

// VAR: the level of the variance-guided mode (denoise_device.h): luminance edge-stop scaled by the 3 x 3 binomial of the variance in
// in[].w at the level's own step (the inner 3 x 3 of the taps the level loads anyway), the variance filtered along into out[].w
// GEO: the geometry guide (denoise_device.h; KIND 2 only): one more 16-byte stream per tap, read where the caller keeps it; the
// centre's normal and invG once per thread. The GEO = false builds read neither of the two last arguments.
template<int KIND, bool VAR, bool GEO = false>
__global__ void __launch_bounds__(256) denoiseLevelKernel(const float4* __restrict__ in, const float4* __restrict__ guideNormal, const float4* __restrict__ guideAlbedo,
                                                          float4* __restrict__ out, DenoiseConstants k, int step, const float4* __restrict__ geometry, DenoiseGeometryConstants g)
{
  const int x = (int) blockIdx.x * TWK_DENOISE_TILE_X + (int) (threadIdx.x % TWK_DENOISE_TILE_X);
  const int y = (int) blockIdx.y * TWK_DENOISE_TILE_Y + (int) (threadIdx.x / TWK_DENOISE_TILE_X);
  if (x >= k.width || y >= k.height) return;
  const size_t p = (size_t) y * k.width + x;
  const float4 cp = in[p];
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 np = (KIND >= 2) ? guideNormal[p] : zero;
  const float4 ap = (KIND >= 1) ? guideAlbedo[p] : zero;
  if (!finite3(cp) || !finite3(np) || !finite3(ap)) { out[p] = cp; return; }
  DenoiseGeometryCentre gc;
  if (GEO) { if (!denoiseGeometryCentre(g, geometry[p], np, gc)) { out[p] = cp; return; } }
  float lp = 0.0f, invL = 0.0f, vsum = 0.0f;
  if (VAR)
  {
    lp = luminance(cp);
    if (!finite1(lp)) { out[p] = cp; return; }
    float vs = 0.0f, bs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
    {
      const int qy = y + dy * step;
      if (qy < 0 || qy >= k.height) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
      {
        const int qx = x + dx * step;
        if (qx < 0 || qx >= k.width) continue;
        varianceBlurTap(dx, dy, in[(size_t) qy * k.width + qx], vs, bs);
      }
    }
    invL = inverseLuminanceSigma(k, vs, bs);
  }
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
  {
    const int qy = y + dy * step;
    if (qy < 0 || qy >= k.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx)
    {
      const int qx = x + dx * step;
      if (qx < 0 || qx >= k.width) continue;
      const size_t q = (size_t) qy * k.width + qx;
      const float4 cq = in[q];
      const float4 nq = (KIND >= 2) ? guideNormal[q] : zero;
      const float4 aq = (KIND >= 1) ? guideAlbedo[q] : zero;
      if (GEO)
      {
        const float4 gq = geometry[q];
        if (VAR) denoiseVarianceTap<KIND, true>(k, dx, dy, lp, invL, np, ap, cq, nq, aq, sx, sy, sz, wsum, vsum, gc, gq);
        else     denoiseTap<KIND, true>(k, dx, dy, cp, np, ap, cq, nq, aq, sx, sy, sz, wsum, gc, gq);
      }
      else if (VAR) denoiseVarianceTap<KIND>(k, dx, dy, lp, invL, np, ap, cq, nq, aq, sx, sy, sz, wsum, vsum);
      else          denoiseTap<KIND>(k, dx, dy, cp, np, ap, cq, nq, aq, sx, sy, sz, wsum);
    }
  }
  out[p] = make_float4(sx / wsum, sy / wsum, sz / wsum, VAR ? vsum / (wsum * wsum) : cp.w);
}

// LDS-staged build: the same level with the block's taps staged in LDS. A block takes 32 x 8 pixels of ONE residue class modulo the step — pixels
// (rx + step i, ry + step j) — so that its taps are a dense 5 x 5 again and the staged region is the tile plus a halo of 2 in
// every direction, 36 x 12 = 432 pixels per 256, whatever the step (at step 1 this is the plain tile with its halo). Pixels
// outside the picture are staged with a NaN colour, which denoiseTap skips like any non-finite tap. Same operations in the same
// order as denoiseLevelKernel: the same bits (tests/test_gpu_denoise.py runs every case with every level on either build).
// The staging loads of a wave are 32-pixel runs with a stride of `step` pixels: at step >= 8 every lane reads a 128-byte line of
// its own, which is where this build stops paying.
#define TWK_DENOISE_LDS_X (TWK_DENOISE_TILE_X + 4)
#define TWK_DENOISE_LDS_Y (TWK_DENOISE_TILE_Y + 4)
// GEO: the geometry is staged as a fourth 36 x 12 array (27.6 KB per block instead of 20.7); outside the picture it is staged as a
// miss, and the tap is skipped for its NaN colour before the geometry is looked at.
template<int KIND, bool VAR, bool GEO = false>
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
  const int centre = (ly + 2) * TWK_DENOISE_LDS_X + lx + 2;
  const float4 cp = colour[centre];
  const float4 np = (KIND >= 2) ? normal[centre] : zero;
  const float4 ap = (KIND >= 1) ? albedo[centre] : zero;
  if (!finite3(cp) || !finite3(np) || !finite3(ap)) { out[p] = cp; return; }
  DenoiseGeometryCentre gc;
  if (GEO) { if (!denoiseGeometryCentre(g, position[centre], np, gc)) { out[p] = cp; return; } }
  float lp = 0.0f, invL = 0.0f, vsum = 0.0f;
  if (VAR)
  {
    lp = luminance(cp);
    if (!finite1(lp)) { out[p] = cp; return; }
    float vs = 0.0f, bs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
    {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) varianceBlurTap(dx, dy, colour[centre + dy * TWK_DENOISE_LDS_X + dx], vs, bs); // outside the picture: NaN colour, skipped
    }
    invL = inverseLuminanceSigma(k, vs, bs);
  }
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
  {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx)
    {
      const int q = centre + dy * TWK_DENOISE_LDS_X + dx;
      const float4 cq = colour[q];
      const float4 nq = (KIND >= 2) ? normal[q] : zero;
      const float4 aq = (KIND >= 1) ? albedo[q] : zero;
      if (GEO)
      {
        const float4 gq = position[q];
        if (VAR) denoiseVarianceTap<KIND, true>(k, dx, dy, lp, invL, np, ap, cq, nq, aq, sx, sy, sz, wsum, vsum, gc, gq);
        else     denoiseTap<KIND, true>(k, dx, dy, cp, np, ap, cq, nq, aq, sx, sy, sz, wsum, gc, gq);
      }
      else if (VAR) denoiseVarianceTap<KIND>(k, dx, dy, lp, invL, np, ap, cq, nq, aq, sx, sy, sz, wsum, vsum);
      else          denoiseTap<KIND>(k, dx, dy, cp, np, ap, cq, nq, aq, sx, sy, sz, wsum);
    }
  }
  out[p] = make_float4(sx / wsum, sy / wsum, sz / wsum, VAR ? vsum / (wsum * wsum) : cp.w);
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
template<int KIND, bool SAMPLED, bool GEO = false>
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
  const float4 cp = in[p];
  const float4 np = (KIND >= 2) ? normal[centre] : zero;
  const float4 ap = (KIND >= 1) ? albedo[centre] : zero;
  if (!finite3(cp) || !finite1(lum[centre]) || !finite3(np) || !finite3(ap)) { out[p] = make_float4(cp.x, cp.y, cp.z, 0.0f); return; }
  DenoiseGeometryCentre gc;
  if (GEO) { if (!denoiseGeometryCentre(g, position[centre], np, gc)) { out[p] = make_float4(cp.x, cp.y, cp.z, 0.0f); return; } }
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int dy = -TWK_DENOISE_MOMENTS_RADIUS; dy <= TWK_DENOISE_MOMENTS_RADIUS; ++dy)
  {
#pragma unroll
    for (int dx = -TWK_DENOISE_MOMENTS_RADIUS; dx <= TWK_DENOISE_MOMENTS_RADIUS; ++dx)
    {
      if (dx == 0 && dy == 0) continue;
      const int q = centre + dy * TWK_DENOISE_MOMENTS_X + dx;
      const float lq = lum[q];
      if ((asUint(lq) & 0x7fffffffu) > 0x7f800000u) continue; // NaN: outside, or a colour that is not finite
      const float4 nq = (KIND >= 2) ? normal[q] : zero;
      const float4 aq = (KIND >= 1) ? albedo[q] : zero;
      if (GEO) momentsTap<KIND, true>(k, np, ap, lq, nq, aq, s0, s1, s2, gc, position[q]);
      else     momentsTap<KIND>(k, np, ap, lq, nq, aq, s0, s1, s2);
    }
  }
  if (SAMPLED) out[p] = momentsFinish<true>(k, cp, s0, s1, s2, sampled[p], minSamples);
  else         out[p] = momentsFinish(k, cp, s0, s1, s2);
}

template<typename Pixel>
__global__ void __launch_bounds__(256) denoiseFinishKernel(const Pixel* __restrict__ beauty, const float4* __restrict__ colour, const float4* __restrict__ guideNormal,
                                                           const float4* __restrict__ guideAlbedo, Pixel* __restrict__ denoised, DenoiseConstants k)
{
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  const Pixel raw = beauty[p];
  const float4 b = widen(raw);
  float4 r = colour[p];
  bool through = !finite3(b);
  if (guideNormal) through = through || !finite3(guideNormal[p]);
  if (guideAlbedo)
  {
    const float4 a = guideAlbedo[p];
    through = through || !finite3(a);
    if (k.demodulate)
    {
      const float3 d = clampedAlbedo(a);
      r.x = r.x * d.x; r.y = r.y * d.y; r.z = r.z * d.z;
    }
  }
  if (through || !finite3(r)) { denoised[p] = raw; return; } // !finite3(r): the demodulated colour overflowed
  float4 o;
  o.x = r.x + k.blendFactor * (b.x - r.x);
  o.y = r.y + k.blendFactor * (b.y - r.y);
  o.z = r.z + k.blendFactor * (b.z - r.z);
  o.w = b.w;
  denoised[p] = pixelOf<Pixel>(o);
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

template<int KIND, bool VAR, bool GEO = false>
static void launchDenoiseLevelOf(bool lds, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k, int step, hipStream_t stream,
                                 const float4* geometry = nullptr, const DenoiseGeometryConstants& g = DenoiseGeometryConstants())
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
// geometry != NULL (kind RGB_ALBEDO_NORMAL only, the caller's check): the GEO builds, with the camera and sigma of *g
void launchDenoiseLevel(int kind, bool lds, bool variance, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k, int step, hipStream_t stream,
                        const float4* geometry, const DenoiseGeometryConstants* g)
{
  if (geometry)
  {
    if (variance) launchDenoiseLevelOf<TWK_DENOISER_RGB_ALBEDO_NORMAL, true, true>(lds, in, guideNormal, guideAlbedo, out, k, step, stream, geometry, *g);
    else          launchDenoiseLevelOf<TWK_DENOISER_RGB_ALBEDO_NORMAL, false, true>(lds, in, guideNormal, guideAlbedo, out, k, step, stream, geometry, *g);
    return;
  }
  if (variance)
  {
    if (kind == TWK_DENOISER_RGB_ALBEDO_NORMAL) launchDenoiseLevelOf<TWK_DENOISER_RGB_ALBEDO_NORMAL, true>(lds, in, guideNormal, guideAlbedo, out, k, step, stream);
    else if (kind == TWK_DENOISER_RGB_ALBEDO)   launchDenoiseLevelOf<TWK_DENOISER_RGB_ALBEDO, true>(lds, in, guideNormal, guideAlbedo, out, k, step, stream);
    else                                        launchDenoiseLevelOf<TWK_DENOISER_RGB, true>(lds, in, guideNormal, guideAlbedo, out, k, step, stream);
    return;
  }
  if (kind == TWK_DENOISER_RGB_ALBEDO_NORMAL) launchDenoiseLevelOf<TWK_DENOISER_RGB_ALBEDO_NORMAL, false>(lds, in, guideNormal, guideAlbedo, out, k, step, stream);
  else if (kind == TWK_DENOISER_RGB_ALBEDO)   launchDenoiseLevelOf<TWK_DENOISER_RGB_ALBEDO, false>(lds, in, guideNormal, guideAlbedo, out, k, step, stream);
  else                                        launchDenoiseLevelOf<TWK_DENOISER_RGB, false>(lds, in, guideNormal, guideAlbedo, out, k, step, stream);
}

template<bool SAMPLED>
static void launchDenoiseMomentsOf(int kind, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k,
                                   const float4* sampled, float minSamples, hipStream_t stream, const float4* geometry, const DenoiseGeometryConstants* g)
{
  const dim3 grid((k.width + TWK_DENOISE_TILE_X - 1) / TWK_DENOISE_TILE_X, (k.height + TWK_DENOISE_TILE_Y - 1) / TWK_DENOISE_TILE_Y);
  const DenoiseGeometryConstants none = DenoiseGeometryConstants();
  if (geometry)                                    hipLaunchKernelGGL((denoiseMomentsKernel<TWK_DENOISER_RGB_ALBEDO_NORMAL, SAMPLED, true>), grid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, sampled, minSamples, geometry, *g);
  else if (kind == TWK_DENOISER_RGB_ALBEDO_NORMAL) hipLaunchKernelGGL((denoiseMomentsKernel<TWK_DENOISER_RGB_ALBEDO_NORMAL, SAMPLED>), grid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, sampled, minSamples, geometry, none);
  else if (kind == TWK_DENOISER_RGB_ALBEDO)        hipLaunchKernelGGL((denoiseMomentsKernel<TWK_DENOISER_RGB_ALBEDO, SAMPLED>), grid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, sampled, minSamples, geometry, none);
  else                                             hipLaunchKernelGGL((denoiseMomentsKernel<TWK_DENOISER_RGB, SAMPLED>), grid, dim3(256), 0, stream, in, guideNormal, guideAlbedo, out, k, sampled, minSamples, geometry, none);
}

// the moments + firefly-clamp pass of the variance-guided mode, between prepare and level 0. sampled != NULL: the SAMPLED build —
// width x height luminance moments (mean, M2, n, .), whose measured variance stands in for the spatial one from minSamples samples on
// geometry != NULL (kind RGB_ALBEDO_NORMAL only): the GEO builds
void launchDenoiseMoments(int kind, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k,
                          const float4* sampled, float minSamples, hipStream_t stream, const float4* geometry, const DenoiseGeometryConstants* g)
{
  if (sampled) launchDenoiseMomentsOf<true>(kind, in, guideNormal, guideAlbedo, out, k, sampled, minSamples, stream, geometry, g);
  else         launchDenoiseMomentsOf<false>(kind, in, guideNormal, guideAlbedo, out, k, nullptr, 0.0f, stream, geometry, g);
}

// guideNormal / guideAlbedo NULL: the kind does not use the guide
void launchDenoiseFinish(const void* beauty, bool half, const float4* colour, const float4* guideNormal, const float4* guideAlbedo, void* denoised, const DenoiseConstants& k, hipStream_t stream)
{
  if (half) hipLaunchKernelGGL(denoiseFinishKernel<Half4>, dim3(pixelBlocks(k)), dim3(256), 0, stream, static_cast<const Half4*>(beauty), colour, guideNormal, guideAlbedo, static_cast<Half4*>(denoised), k);
  else      hipLaunchKernelGGL(denoiseFinishKernel<float4>, dim3(pixelBlocks(k)), dim3(256), 0, stream, static_cast<const float4*>(beauty), colour, guideNormal, guideAlbedo, static_cast<float4*>(denoised), k);
}

} // namespace twk
