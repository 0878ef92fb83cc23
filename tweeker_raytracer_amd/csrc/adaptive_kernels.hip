// Kernels of twk_adaptive_select: the predicate of adaptive_device.h over a stream of luminance moments and sample counts, and the
// compaction of the selected indices into an ascending list.
//
// Three launches on one stream, and no block ever waits for another (no look-back, no flag anybody spins on: the order of the
// launches is the only dependency):
//   1. ballotKernel   grid-stride over tiles of 1024 elements, a block of 1024 lanes per tile at a time. A lane reads its 16-byte
//                     moments element and its count word (coalesced), every wave ballots its predicate and stores the 64-bit word,
//                     the tile's population count goes through LDS into one word.
//   2. scanKernel     ONE block scans the tile counts exclusively, 1024 at a time with a running carry when there are more tiles
//                     than lanes, and stores the total.
//   3. scatterKernel  reads only the ballot words and the tile offsets: a selected lane writes its index at the tile's offset + the
//                     population count of the lower waves' words + that of the lower lanes' bits. Offsets and ranks are sums over
//                     ascending indices, so the list is ascending and does not depend on the grid.
// The list is written below `total` <= numElements only: every write index is offset + rank of a selected element.
#include "adaptive_device.h"

namespace twk {

__global__ void __launch_bounds__(TWK_ADAPTIVE_TILE)
adaptiveBallotKernel(const float4* __restrict__ moments, const unsigned int* __restrict__ counts, size_t numElements, size_t numTiles,
                     unsigned long long* __restrict__ ballots, unsigned int* __restrict__ tileCounts, AdaptiveConstants k)
{
  __shared__ unsigned int wavePop[TWK_ADAPTIVE_TILE_WAVES];
  const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  // `tile` is the same in every lane of the block: no lane leaves the loop before the others (barriers and ballots see whole blocks)
  for (size_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x)
  {
    const size_t i = tile * TWK_ADAPTIVE_TILE + threadIdx.x;
    bool selected = false;
    if (i < numElements) selected = adaptiveSelected(k, moments[i], counts[i]);
    const unsigned long long word = __ballot(selected);
    if (lane == 0u)
    {
      ballots[tile * TWK_ADAPTIVE_TILE_WAVES + wave] = word;
      wavePop[wave] = (unsigned int) __popcll(word);
    }
    __syncthreads();
    if (threadIdx.x == 0u)
    {
      unsigned int sum = 0u;
      for (int w = 0; w < TWK_ADAPTIVE_TILE_WAVES; ++w) sum += wavePop[w];
      tileCounts[tile] = sum;
    }
    __syncthreads(); // wavePop is written again by the next tile
  }
}

// One block. tileOffsets[t] = sum of tileCounts[0 .. t-1]; *total = the sum of all.
__global__ void __launch_bounds__(TWK_ADAPTIVE_TILE)
adaptiveScanKernel(const unsigned int* __restrict__ tileCounts, size_t numTiles, unsigned int* __restrict__ tileOffsets, unsigned int* __restrict__ total)
{
  __shared__ unsigned int waveSum[TWK_ADAPTIVE_TILE_WAVES];
  const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  unsigned int carry = 0u; // the same in every lane
  for (size_t base = 0; base < numTiles; base += TWK_ADAPTIVE_TILE)
  {
    const size_t t = base + threadIdx.x;
    const unsigned int own = (t < numTiles) ? tileCounts[t] : 0u;
    unsigned int inclusive = own; // within the wave
#pragma unroll
    for (int offset = 1; offset < 64; offset <<= 1)
    {
      const unsigned int below = __shfl_up(inclusive, offset);
      if (lane >= (unsigned int) offset) inclusive += below;
    }
    if (lane == 63u) waveSum[wave] = inclusive;
    __syncthreads();
    unsigned int before = 0u, chunk = 0u;
    for (int w = 0; w < TWK_ADAPTIVE_TILE_WAVES; ++w)
    {
      const unsigned int s = waveSum[w];
      if ((unsigned int) w < wave) before += s;
      chunk += s;
    }
    if (t < numTiles) tileOffsets[t] = carry + before + (inclusive - own);
    carry += chunk;
    __syncthreads(); // waveSum is written again by the next chunk
  }
  if (threadIdx.x == 0u) *total = carry;
}

__global__ void __launch_bounds__(TWK_ADAPTIVE_TILE)
adaptiveScatterKernel(const unsigned long long* __restrict__ ballots, const unsigned int* __restrict__ tileOffsets, size_t numTiles, unsigned int* __restrict__ active)
{
  __shared__ unsigned long long words[TWK_ADAPTIVE_TILE_WAVES];
  const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (size_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x)
  {
    if (threadIdx.x < TWK_ADAPTIVE_TILE_WAVES) words[threadIdx.x] = ballots[tile * TWK_ADAPTIVE_TILE_WAVES + threadIdx.x];
    __syncthreads();
    const unsigned long long word = words[wave];
    if ((word >> lane) & 1ull)
    {
      unsigned int rank = (unsigned int) __popcll(word & ((1ull << lane) - 1ull));
      for (unsigned int w = 0; w < wave; ++w) rank += (unsigned int) __popcll(words[w]);
      active[(size_t) tileOffsets[tile] + rank] = (unsigned int) (tile * TWK_ADAPTIVE_TILE + threadIdx.x);
    }
    __syncthreads(); // words is written again by the next tile
  }
}

// `scratch`: adaptiveScratchBytes(numElements) bytes, aligned to 8. Returns where the total lies in it (one word, device memory).
unsigned int* launchAdaptiveSelect(const float4* moments, const unsigned int* counts, size_t numElements, unsigned int* active, void* scratch,
                                   const AdaptiveConstants& k, int numCUs, hipStream_t stream)
{
  const size_t tiles = adaptiveTiles(numElements);
  unsigned long long* ballots = static_cast<unsigned long long*>(scratch);
  unsigned int* tileCounts = reinterpret_cast<unsigned int*>(ballots + tiles * TWK_ADAPTIVE_TILE_WAVES);
  unsigned int* tileOffsets = tileCounts + tiles;
  unsigned int* total = tileOffsets + tiles;
  size_t grid = tiles;
  const size_t most = (size_t) (numCUs > 0 ? numCUs : 1) * 2; // two blocks of 1024 lanes fill a CU's 32 wave slots
  if (grid > most) grid = most;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(adaptiveBallotKernel, dim3((unsigned int) grid), dim3(TWK_ADAPTIVE_TILE), 0, stream, moments, counts, numElements, tiles, ballots, tileCounts, k);
  hipLaunchKernelGGL(adaptiveScanKernel, dim3(1), dim3(TWK_ADAPTIVE_TILE), 0, stream, tileCounts, tiles, tileOffsets, total);
  hipLaunchKernelGGL(adaptiveScatterKernel, dim3((unsigned int) grid), dim3(TWK_ADAPTIVE_TILE), 0, stream, ballots, tileOffsets, tiles, active);
  return total;
}

} // namespace twk
