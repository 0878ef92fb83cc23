// Kernel of twk_estimate_noise: classifies every element of a stream of luminance moments and reduces the stream to the integer
// summary defined in noise_device.h (three counts, a 256-bin histogram of the relative standard error e, its fixed-point sum and
// its largest bits), optionally writing e per element.
//
// One kernel, a grid-stride loop. A lane reads its (mean, M2, n, .) with one coalesced load of its 16-byte element (the compiler
// narrows it to the 12 bytes the definition uses: global_load_dwordx3, the same lines), the next iteration's load issued before
// this one's arithmetic. The block's histogram lives in LDS (256 words, LDS atomics; a wave whose valid lanes all fall into one
// bin, a flat or a black region, adds its count once instead of 64 times to one address). Counts, sum and maximum stay in
// registers over the loop, are reduced per wave with shuffles and per block through LDS. At its end a block issues one global
// atomic per NON-EMPTY bin (lanes 0..255, one bin each: contiguous words), and one each for the sum, the maximum and the counts
// that are not zero; none of them uses its result, so they compile to the forms that return nothing.
//
// The grid is at most numCUs x TWK_NOISE_BLOCKS_PER_CU = 1 blocks of 1024 lanes. What bounds it from above is the contention on
// the summary: every block adds to the same few words, and one word takes about 88 atomics per microsecond (measured for the
// returning form on this part), so 256 blocks cost a word about 3 microseconds, where a block per 256 elements (8100 at
// 1920 x 1080) would cost it 90. What bounds it from below is the memory latency, which only waves in flight hide: the kernel
// holds 100 vector registers, so 16 waves, one block of 1024, is what a CU can hold of it anyway, each lane with one load in
// flight over its arithmetic. A block of 1024 rather than two of 512 halves the atomics for the same waves. Its time against the
// floor of its compulsory bytes is measured by tools/noise_time.py (profiles/r12_noise.md).
#include "noise_device.h"

namespace twk {

#define TWK_NOISE_BLOCK 1024
#define TWK_NOISE_BLOCKS_PER_CU 1
#define TWK_NOISE_WAVES (TWK_NOISE_BLOCK / 64)

__global__ void __launch_bounds__(TWK_NOISE_BLOCK)
noiseKernel(const float4* __restrict__ moments, size_t numElements, float* __restrict__ errorMap, TwkNoiseSummary* __restrict__ summary, NoiseConstants k)
{
  __shared__ unsigned int bins[256];
  __shared__ unsigned int waveCounts[TWK_NOISE_WAVES][3];
  __shared__ unsigned int waveMax[TWK_NOISE_WAVES];
  __shared__ unsigned long long waveSum[TWK_NOISE_WAVES];
  if (threadIdx.x < 256) bins[threadIdx.x] = 0u;
  __syncthreads();

  const int lane = (int) (threadIdx.x & 63u);
  const size_t stride = (size_t) gridDim.x * TWK_NOISE_BLOCK;
  unsigned int valid = 0u, unknown = 0u, empty = 0u, maxBits = 0u;
  unsigned long long sum = 0ull;
  size_t i = (size_t) blockIdx.x * TWK_NOISE_BLOCK + threadIdx.x;
  float4 next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i < numElements) next = moments[i];
  // `base` is the same in every lane of the block: no lane leaves the loop before the others, the wave operations below see whole waves
  for (size_t base = (size_t) blockIdx.x * TWK_NOISE_BLOCK; base < numElements; base += stride, i += stride)
  {
    const float4 m = next;
    if (i + stride < numElements) next = moments[i + stride];
    bool isValid = false;
    int bin = 0;
    if (i < numElements)
    {
      float e;
      const int c = noiseClassify(k, m, e);
      valid += (c == TWK_NOISE_VALID) ? 1u : 0u; unknown += (c == TWK_NOISE_UNKNOWN) ? 1u : 0u; empty += (c == TWK_NOISE_EMPTY) ? 1u : 0u;
      if (c == TWK_NOISE_VALID)
      {
        isValid = true;
        bin = noiseBin(e);
        sum += noiseFixed(e);
        maxBits = max(maxBits, asUint(e));
      }
      if (errorMap) errorMap[i] = noiseMapValue(c, e);
    }
    const unsigned long long mask = __ballot(isValid);
    if (mask != 0ull)
    {
      const int first = __ffsll((long long) mask) - 1;
      const int firstBin = __shfl(bin, first);
      if (__all(!isValid || bin == firstBin))
      {
        if (lane == first) atomicAdd(&bins[firstBin], (unsigned int) __popcll(mask));
      }
      else if (isValid) atomicAdd(&bins[bin], 1u);
    }
  }

#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1)
  {
    valid += __shfl_down(valid, offset);
    unknown += __shfl_down(unknown, offset);
    empty += __shfl_down(empty, offset);
    sum += __shfl_down(sum, offset);
    maxBits = max(maxBits, __shfl_down(maxBits, offset));
  }
  const int wave = (int) (threadIdx.x >> 6);
  if (lane == 0)
  {
    waveCounts[wave][TWK_NOISE_VALID] = valid; waveCounts[wave][TWK_NOISE_UNKNOWN] = unknown; waveCounts[wave][TWK_NOISE_EMPTY] = empty;
    waveSum[wave] = sum; waveMax[wave] = maxBits;
  }
  __syncthreads();

  if (threadIdx.x < 256)
  {
    const unsigned int h = bins[threadIdx.x];
    if (h != 0u) atomicAdd(&summary->histogram[threadIdx.x], h);
  }
  if (threadIdx.x == 0)
  {
    unsigned long long total[3] = {0ull, 0ull, 0ull}, blockSum = 0ull;
    unsigned int blockMax = 0u;
    for (int w = 0; w < TWK_NOISE_WAVES; ++w)
    {
      total[0] += waveCounts[w][0]; total[1] += waveCounts[w][1]; total[2] += waveCounts[w][2];
      blockSum += waveSum[w]; blockMax = max(blockMax, waveMax[w]);
    }
    if (total[TWK_NOISE_VALID])   atomicAdd(reinterpret_cast<unsigned long long*>(&summary->valid), total[TWK_NOISE_VALID]);
    if (total[TWK_NOISE_UNKNOWN]) atomicAdd(reinterpret_cast<unsigned long long*>(&summary->unknown), total[TWK_NOISE_UNKNOWN]);
    if (total[TWK_NOISE_EMPTY])   atomicAdd(reinterpret_cast<unsigned long long*>(&summary->empty), total[TWK_NOISE_EMPTY]);
    if (blockSum) atomicAdd(reinterpret_cast<unsigned long long*>(&summary->sumFixed), blockSum);
    if (blockMax) atomicMax(&summary->maxErrorBits, blockMax);
  }
}

// The summary must have been zeroed on `stream` before: the kernel only adds to it
void launchNoise(const float4* moments, size_t numElements, float* errorMap, TwkNoiseSummary* summary, const NoiseConstants& k, int numCUs, hipStream_t stream)
{
  size_t grid = (numElements + TWK_NOISE_BLOCK - 1) / TWK_NOISE_BLOCK;
  const size_t most = (size_t) (numCUs > 0 ? numCUs : 1) * TWK_NOISE_BLOCKS_PER_CU;
  if (grid > most) grid = most;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(noiseKernel, dim3((unsigned int) grid), dim3(TWK_NOISE_BLOCK), 0, stream, moments, numElements, errorMap, summary, k);
}

} // namespace twk
