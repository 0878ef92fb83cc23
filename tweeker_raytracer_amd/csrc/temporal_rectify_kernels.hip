// Kernels of twk_temporal_accumulate_rectified: the two launches temporal_rectify_device.h defines.
#include "temporal_rectify_device.h"
#include "temporal_store.h"

// The window radius of the test kernel: below TWK_RECTIFY_RUNTIME_FROM it is a template parameter (one build per radius and format,
// the window loops unrolled, the window's d held in registers between the two passes), from there on a run-time value (one build
// per format that reads the window from LDS twice, LDS sized for the largest radius). Decided by an A/B on the MI355X
// (tools/temporal_rectify_time.py on builds of tools/ab_variant.sh with -DTWK_RECTIFY_RUNTIME_FROM=1 and =5;
// profiles/r22_temporal_rectify.md): the template build wins at radius 1..3 by 0 - 4 % of the call, and loses at radius 4 by 11 - 13 %, where its 81
// held taps cost 104 - 106 VGPRs and half the occupancy. Both builds compute the same bits.
#ifndef TWK_RECTIFY_RUNTIME_FROM
#define TWK_RECTIFY_RUNTIME_FROM 4
#endif

namespace twk {

// Launch 1. One thread per pixel, the access pattern of temporalKernel (temporal_kernels.hip): three coalesced loads of the frame,
// four neighbouring 16-byte gathers per history stream, the geometry first; two coalesced 16-byte stores of the scratch words.
template<typename Pixel>
__global__ void __launch_bounds__(256) rectifyReprojectKernel(const Pixel* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ geometry,
                                                              const float4* __restrict__ historyColour, const float4* __restrict__ historyMoments,
                                                              const float4* __restrict__ historyGeometry, float4* __restrict__ scratchA, float4* __restrict__ scratchB, TemporalConstants k)
{
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  float4 A, B;
  rectifyReproject(k, widen(colour[p]), moments[p], geometry[p], historyColour, historyMoments, historyGeometry, A, B);
  scratchA[p] = A;
  scratchB[p] = B;
}

// Launch 1's Moving build (temporal_motion_device.h): as above, plus one 64-byte record of the table per candidate pixel, read
// before the projection; Staged: from the block's LDS copy (motionTable). Launch 2 is the same for both. A kernel of its own, so
// that the one above is the code it was.
template<typename Pixel, bool Staged>
__global__ void __launch_bounds__(256) rectifyReprojectMovingKernel(const Pixel* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ geometry,
                                                                    const float4* __restrict__ historyColour, const float4* __restrict__ historyMoments,
                                                                    const float4* __restrict__ historyGeometry, const TwkInstanceMotion* __restrict__ motion, unsigned int numMotion,
                                                                    float4* __restrict__ scratchA, float4* __restrict__ scratchB, TemporalConstants k)
{
  __shared__ TwkInstanceMotion staged[Staged ? TWK_MOTION_LDS_RECORDS : 1];
  const TwkInstanceMotion* table = motionTable<Staged>(motion, numMotion, staged, 256u);
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  float4 A, B;
  rectifyReproject<true>(k, widen(colour[p]), moments[p], geometry[p], historyColour, historyMoments, historyGeometry, A, B, table, numMotion);
  scratchA[p] = A;
  scratchB[p] = B;
}

// Launch 1's Carried build (temporal_carry_device.h): as the first kernel, plus one coalesced 16-byte read of the previous-position
// plane per pixel; no table. Launch 2 is the same for all three. A kernel of its own, so that the ones above are the code they were.
template<typename Pixel>
__global__ void __launch_bounds__(256) rectifyReprojectCarriedKernel(const Pixel* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ geometry,
                                                                     const float4* __restrict__ historyColour, const float4* __restrict__ historyMoments,
                                                                     const float4* __restrict__ historyGeometry, const float4* __restrict__ plane,
                                                                     float4* __restrict__ scratchA, float4* __restrict__ scratchB, TemporalConstants k)
{
  const size_t p = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t) k.width * k.height) return;
  float4 A, B;
  rectifyReproject<false, true>(k, widen(colour[p]), moments[p], geometry[p], historyColour, historyMoments, historyGeometry, A, B, nullptr, 0u, plane[p]);
  scratchA[p] = A;
  scratchB[p] = B;
}

// Launch 2. A block is a 32 x 8 pixel tile: thread t is pixel (t % 32, t / 32) of it, so a wave is two rows of 32 pixels and every
// global access of the merge is a coalesced 16-byte (RGBA16F colour: 8-byte) one. The block first stages d and key of the tile and
// a halo of `radius` pixels into LDS, (32 + 2 radius) x (8 + 2 radius) pairs of words — at radius 4, 40 x 16 x 8 = 5120 bytes; the
// halo is read from the moments (one word) and the scratch word B only. A window tap is then two ds_read_b32 whose 32 lanes of a
// half-wave read 32 consecutive words: no bank conflict at any pitch. R > 0: the radius at compile time; R = 0: r.radius, LDS for 4.
template<typename Pixel, int R>
__global__ void __launch_bounds__(TWK_RECTIFY_TILE_X * TWK_RECTIFY_TILE_Y)
rectifyMergeKernel(const Pixel* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ scratchA, const float4* __restrict__ scratchB,
                   Pixel* __restrict__ colourOut, float4* __restrict__ historyOut, float4* __restrict__ momentsOut, float* __restrict__ trustOut, TemporalConstants k, RectifyConstants r)
{
  constexpr int HALO = R > 0 ? R : TWK_RECTIFY_MAX_RADIUS;
  constexpr int PITCH = TWK_RECTIFY_TILE_X + 2 * HALO, ROWS = TWK_RECTIFY_TILE_Y + 2 * HALO;
  __shared__ float        sd[PITCH * ROWS];
  __shared__ unsigned int sk[PITCH * ROWS];
  const int radius = R > 0 ? R : r.radius; // 1 .. TWK_RECTIFY_MAX_RADIUS (refused otherwise before the launch)
  const int tid = (int) threadIdx.x;
  const int bx = (int) blockIdx.x * TWK_RECTIFY_TILE_X - radius, by = (int) blockIdx.y * TWK_RECTIFY_TILE_Y - radius; // the staged region's corner
  const int stagedWidth = TWK_RECTIFY_TILE_X + 2 * radius, staged = stagedWidth * (TWK_RECTIFY_TILE_Y + 2 * radius);
  for (int i = tid; i < staged; i += TWK_RECTIFY_TILE_X * TWK_RECTIFY_TILE_Y)
  {
    const int sy = i / stagedWidth, sx = i - sy * stagedWidth;
    const int qx = bx + sx, qy = by + sy;
    float d = 0.0f;
    unsigned int key = 0u;
    if (qx >= 0 && qx < k.width && qy >= 0 && qy < k.height)
    {
      const size_t q = (size_t) qy * k.width + qx;
      rectifyStage(moments[q], scratchB[q], d, key);
    }
    sd[sy * PITCH + sx] = d;
    sk[sy * PITCH + sx] = key;
  }
  __syncthreads();
  const int lx = tid % TWK_RECTIFY_TILE_X, ly = tid / TWK_RECTIFY_TILE_X;
  const int x = bx + radius + lx, y = by + radius + ly;
  if (x >= k.width || y >= k.height) return;
  const size_t p = (size_t) y * k.width + x;
  const Pixel raw = colour[p];
  const float4 cur = widen(raw);
  const float4 mc = moments[p];
  const float4 A = scratchA[p], B = scratchB[p];
  const float t = rectifyTrust<R>(r, sd, sk, PITCH, (ly + radius) * PITCH + lx + radius, B.z, mc.z);
  float4 c, m;
  float trust;
  if (rectifyMerge(t, cur, mc, A, B, c, m, trust)) temporalStoreMerged(p, c, m, colourOut, historyOut, momentsOut);
  else temporalStorePassThrough(p, raw, cur, mc, colourOut, historyOut, momentsOut);
  if (trustOut) trustOut[p] = trust;
}

template<typename Pixel>
static void launchRectify(const void* colour, const float4* moments, const float4* geometry, const float4* historyColour, const float4* historyMoments, const float4* historyGeometry,
                          float4* scratchA, float4* scratchB, void* colourOut, float4* historyOut, float4* momentsOut, float* trustOut, const TemporalConstants& k,
                          const RectifyConstants& r, hipStream_t stream, const TwkInstanceMotion* motion, unsigned int numMotion, const float4* carried)
{
  const size_t numPixels = (size_t) k.width * k.height;
  const Pixel* in = static_cast<const Pixel*>(colour);
  Pixel* out = static_cast<Pixel*>(colourOut);
  const dim3 pixels((unsigned int) ((numPixels + 255) / 256));
  if (carried) // the Carried build: g' from the plane, no table
    hipLaunchKernelGGL(rectifyReprojectCarriedKernel<Pixel>, pixels, dim3(256), 0, stream, in, moments, geometry, historyColour, historyMoments, historyGeometry, carried, scratchA, scratchB, k);
  else if (!(motion && numMotion > 0u)) // without a table launch 1 as it always was
    hipLaunchKernelGGL(rectifyReprojectKernel<Pixel>, pixels, dim3(256), 0, stream, in, moments, geometry, historyColour, historyMoments, historyGeometry, scratchA, scratchB, k);
#if TWK_MOTION_STAGED_RECORDS > 0
  else if (numMotion <= TWK_MOTION_STAGED_RECORDS)
    hipLaunchKernelGGL((rectifyReprojectMovingKernel<Pixel, true>), pixels, dim3(256), 0, stream, in, moments, geometry, historyColour, historyMoments, historyGeometry, motion, numMotion,
                       scratchA, scratchB, k);
#endif
  else
    hipLaunchKernelGGL((rectifyReprojectMovingKernel<Pixel, false>), pixels, dim3(256), 0, stream, in, moments, geometry, historyColour, historyMoments, historyGeometry, motion, numMotion,
                       scratchA, scratchB, k);
  const dim3 grid((unsigned int) ((k.width + TWK_RECTIFY_TILE_X - 1) / TWK_RECTIFY_TILE_X), (unsigned int) ((k.height + TWK_RECTIFY_TILE_Y - 1) / TWK_RECTIFY_TILE_Y));
  const dim3 block(TWK_RECTIFY_TILE_X * TWK_RECTIFY_TILE_Y);
#define TWK_RECTIFY_LAUNCH(R) hipLaunchKernelGGL((rectifyMergeKernel<Pixel, R>), grid, block, 0, stream, in, moments, scratchA, scratchB, out, historyOut, momentsOut, trustOut, k, r)
  if (r.radius >= TWK_RECTIFY_RUNTIME_FROM) TWK_RECTIFY_LAUNCH(0);
#if TWK_RECTIFY_RUNTIME_FROM > 1
  else if (r.radius == 1) TWK_RECTIFY_LAUNCH(1);
#endif
#if TWK_RECTIFY_RUNTIME_FROM > 2
  else if (r.radius == 2) TWK_RECTIFY_LAUNCH(2);
#endif
#if TWK_RECTIFY_RUNTIME_FROM > 3
  else if (r.radius == 3) TWK_RECTIFY_LAUNCH(3);
#endif
#if TWK_RECTIFY_RUNTIME_FROM > 4
  else TWK_RECTIFY_LAUNCH(4);
#endif
#undef TWK_RECTIFY_LAUNCH
}

// Both launches on `stream`. scratchA, scratchB: k.width x k.height float4 each, the handle's; history* nullptr with k.hasHistory 0
// (every pixel then passes through with trust 1). r.radius in 1 .. TWK_RECTIFY_MAX_RADIUS: the caller has refused anything else.
// motion, numMotion: the table of launch 1's Moving build; nullptr or 0: none, the launches as they always were.
void launchTemporalRectify(const void* colour, bool half, const float4* moments, const float4* geometry, const float4* historyColour, const float4* historyMoments,
                           const float4* historyGeometry, float4* scratchA, float4* scratchB, void* colourOut, float4* historyOut, float4* momentsOut, float* trustOut,
                           const TemporalConstants& k, const RectifyConstants& r, hipStream_t stream, const TwkInstanceMotion* motion, unsigned int numMotion, const float4* carried)
{
  if (half) launchRectify<Half4>(colour, moments, geometry, historyColour, historyMoments, historyGeometry, scratchA, scratchB, colourOut, historyOut, momentsOut, trustOut, k, r, stream, motion, numMotion, carried);
  else      launchRectify<float4>(colour, moments, geometry, historyColour, historyMoments, historyGeometry, scratchA, scratchB, colourOut, historyOut, momentsOut, trustOut, k, r, stream, motion, numMotion, carried);
}

} // namespace twk
