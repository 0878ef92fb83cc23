// Kernels of twk_adaptive_plan: the budget of adaptive_plan_device.h over a stream of luminance moments and sample counts, the
// compaction of the elements with a budget into an ascending list, and the exclusive prefix sum of their budgets.
//
// The shape is adaptive_kernels.hip's: three launches on one stream, and no block ever waits for another (no look-back, no flag
// anybody spins on: the order of the launches is the only dependency):
//   1. planBudgetKernel   grid-stride over tiles of 1024 elements, a block of 1024 lanes per tile at a time. A lane reads its
//                         16-byte moments element and its count word (coalesced) and stores its budget as a byte (at most 64), every
//                         wave ballots `budget > 0` and stores the 64-bit word, the tile's population count and budget sum go
//                         through LDS into one word each.
//   2. planScanKernel     ONE block scans both tile arrays exclusively, 1024 tiles at a time with running carries, the budget sums
//                         in 64 bits (a tile's sum is at most 65 536, the total below 2^37), and stores the two totals.
//   3. planScatterKernel  reads the ballot words, the budget bytes and the tile offsets: an element with a budget writes its index at
//                         the tile's offset + the population count of the lower waves' words + that of the lower lanes' bits, and
//                         at the same place the tile's path offset + the sum of the lower elements' budgets: a shuffle scan within
//                         the wave, LDS across the 16 waves. One lane writes the closing pathOffset[numActive] = numPaths.
// Offsets, ranks and sums are over ascending indices, so the plan is ascending and does not depend on the grid. The list is written
// below numActive <= numElements and the offsets below numActive + 1 only. pathOffset holds 32-bit words: a plan whose numPaths does
// not fit them is refused by the caller, which reads the 64-bit total (device_adaptive.hip).
#include "adaptive_plan_device.h"

namespace twk {

__global__ void __launch_bounds__(TWK_ADAPTIVE_TILE)
adaptivePlanBudgetKernel(const float4* __restrict__ moments, const unsigned int* __restrict__ counts, size_t numElements, size_t numTiles,
                         unsigned long long* __restrict__ ballots, unsigned int* __restrict__ tileCounts, unsigned int* __restrict__ tileSums,
                         unsigned char* __restrict__ budgets, AdaptiveConstants k, AdaptivePlanConstants plan)
{
  __shared__ unsigned int wavePop[TWK_ADAPTIVE_TILE_WAVES];
  __shared__ unsigned int waveSum[TWK_ADAPTIVE_TILE_WAVES];
  const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  // `tile` is the same in every lane of the block: no lane leaves the loop before the others (barriers, ballots and shuffles see whole blocks)
  for (size_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x)
  {
    const size_t i = tile * TWK_ADAPTIVE_TILE + threadIdx.x;
    unsigned int b = 0u;
    if (i < numElements)
    {
      b = adaptiveBudget(k, plan, moments[i], counts[i]);
      budgets[i] = (unsigned char) b;
    }
    const unsigned long long word = __ballot(b != 0u);
    unsigned int sum = b; // the wave's budget sum, in every lane
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) sum += __shfl_xor(sum, offset);
    if (lane == 0u)
    {
      ballots[tile * TWK_ADAPTIVE_TILE_WAVES + wave] = word;
      wavePop[wave] = (unsigned int) __popcll(word);
      waveSum[wave] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0u)
    {
      unsigned int pop = 0u, total = 0u;
      for (int w = 0; w < TWK_ADAPTIVE_TILE_WAVES; ++w) { pop += wavePop[w]; total += waveSum[w]; }
      tileCounts[tile] = pop;
      tileSums[tile] = total;
    }
    __syncthreads(); // wavePop and waveSum are written again by the next tile
  }
}

// One block. tileOffsets[t] = sum of tileCounts[0 .. t-1], tilePathOffsets[t] = sum of tileSums[0 .. t-1]; totals = (sum of all
// budgets, sum of all counts).
__global__ void __launch_bounds__(TWK_ADAPTIVE_TILE)
adaptivePlanScanKernel(const unsigned int* __restrict__ tileCounts, const unsigned int* __restrict__ tileSums, size_t numTiles,
                       unsigned int* __restrict__ tileOffsets, unsigned long long* __restrict__ tilePathOffsets, unsigned long long* __restrict__ totals)
{
  __shared__ unsigned int waveCount[TWK_ADAPTIVE_TILE_WAVES];
  __shared__ unsigned long long wavePaths[TWK_ADAPTIVE_TILE_WAVES];
  const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  unsigned int carryCount = 0u; // the same in every lane
  unsigned long long carryPaths = 0ull;
  for (size_t base = 0; base < numTiles; base += TWK_ADAPTIVE_TILE)
  {
    const size_t t = base + threadIdx.x;
    const unsigned int ownCount = (t < numTiles) ? tileCounts[t] : 0u;
    const unsigned long long ownPaths = (t < numTiles) ? (unsigned long long) tileSums[t] : 0ull;
    unsigned int count = ownCount; // inclusive within the wave
    unsigned long long paths = ownPaths;
#pragma unroll
    for (int offset = 1; offset < 64; offset <<= 1)
    {
      const unsigned int countBelow = __shfl_up(count, offset);
      const unsigned long long pathsBelow = __shfl_up(paths, offset);
      if (lane >= (unsigned int) offset) { count += countBelow; paths += pathsBelow; }
    }
    if (lane == 63u) { waveCount[wave] = count; wavePaths[wave] = paths; }
    __syncthreads();
    unsigned int countBefore = 0u, countChunk = 0u;
    unsigned long long pathsBefore = 0ull, pathsChunk = 0ull;
    for (int w = 0; w < TWK_ADAPTIVE_TILE_WAVES; ++w)
    {
      const unsigned int c = waveCount[w];
      const unsigned long long s = wavePaths[w];
      if ((unsigned int) w < wave) { countBefore += c; pathsBefore += s; }
      countChunk += c; pathsChunk += s;
    }
    if (t < numTiles)
    {
      tileOffsets[t] = carryCount + countBefore + (count - ownCount);
      tilePathOffsets[t] = carryPaths + pathsBefore + (paths - ownPaths);
    }
    carryCount += countChunk; carryPaths += pathsChunk;
    __syncthreads(); // waveCount and wavePaths are written again by the next chunk
  }
  if (threadIdx.x == 0u) { totals[0] = carryPaths; totals[1] = (unsigned long long) carryCount; }
}

__global__ void __launch_bounds__(TWK_ADAPTIVE_TILE)
adaptivePlanScatterKernel(const unsigned long long* __restrict__ ballots, const unsigned char* __restrict__ budgets, const unsigned int* __restrict__ tileOffsets,
                          const unsigned long long* __restrict__ tilePathOffsets, const unsigned long long* __restrict__ totals, size_t numElements, size_t numTiles,
                          unsigned int* __restrict__ active, unsigned int* __restrict__ pathOffset)
{
  __shared__ unsigned long long words[TWK_ADAPTIVE_TILE_WAVES];
  __shared__ unsigned int waveSum[TWK_ADAPTIVE_TILE_WAVES];
  const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (blockIdx.x == 0u && threadIdx.x == 0u) pathOffset[totals[1]] = (unsigned int) totals[0]; // totals[1] <= numElements: the buffer's last word at most
  for (size_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x)
  {
    const size_t i = tile * TWK_ADAPTIVE_TILE + threadIdx.x;
    if (threadIdx.x < TWK_ADAPTIVE_TILE_WAVES) words[threadIdx.x] = ballots[tile * TWK_ADAPTIVE_TILE_WAVES + threadIdx.x];
    const unsigned int own = (i < numElements) ? (unsigned int) budgets[i] : 0u;
    unsigned int inclusive = own; // within the wave
#pragma unroll
    for (int offset = 1; offset < 64; offset <<= 1)
    {
      const unsigned int below = __shfl_up(inclusive, offset);
      if (lane >= (unsigned int) offset) inclusive += below;
    }
    if (lane == 63u) waveSum[wave] = inclusive;
    __syncthreads();
    if (own != 0u)
    {
      const unsigned long long word = words[wave];
      unsigned int rank = (unsigned int) __popcll(word & ((1ull << lane) - 1ull));
      unsigned int before = inclusive - own;
      for (unsigned int w = 0; w < wave; ++w) { rank += (unsigned int) __popcll(words[w]); before += waveSum[w]; }
      const size_t at = (size_t) tileOffsets[tile] + rank;
      active[at] = (unsigned int) i;
      pathOffset[at] = (unsigned int) (tilePathOffsets[tile] + before);
    }
    __syncthreads(); // words and waveSum are written again by the next tile
  }
}

// `scratch`: adaptivePlanScratchBytes(numElements) bytes, aligned to 8. active: numElements words at most, pathOffset: numElements
// + 1. Returns where the two totals lie in the scratch (numPaths, numActive: two 64-bit words, device memory).
unsigned long long* launchAdaptivePlan(const float4* moments, const unsigned int* counts, size_t numElements, unsigned int* active, unsigned int* pathOffset,
                                       void* scratch, const AdaptiveConstants& k, const AdaptivePlanConstants& plan, int numCUs, hipStream_t stream)
{
  const size_t tiles = adaptiveTiles(numElements);
  unsigned long long* ballots = static_cast<unsigned long long*>(scratch);
  unsigned long long* tilePathOffsets = ballots + tiles * TWK_ADAPTIVE_TILE_WAVES;
  unsigned long long* totals = tilePathOffsets + tiles;
  unsigned int* tileCounts = reinterpret_cast<unsigned int*>(totals + 2);
  unsigned int* tileOffsets = tileCounts + tiles;
  unsigned int* tileSums = tileOffsets + tiles;
  unsigned char* budgets = reinterpret_cast<unsigned char*>(tileCounts + ((tiles * 3 + 1) & ~(size_t) 1));
  size_t grid = tiles;
  const size_t most = (size_t) (numCUs > 0 ? numCUs : 1) * 2; // two blocks of 1024 lanes fill a CU's 32 wave slots
  if (grid > most) grid = most;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(adaptivePlanBudgetKernel, dim3((unsigned int) grid), dim3(TWK_ADAPTIVE_TILE), 0, stream, moments, counts, numElements, tiles, ballots, tileCounts, tileSums, budgets, k, plan);
  hipLaunchKernelGGL(adaptivePlanScanKernel, dim3(1), dim3(TWK_ADAPTIVE_TILE), 0, stream, tileCounts, tileSums, tiles, tileOffsets, tilePathOffsets, totals);
  hipLaunchKernelGGL(adaptivePlanScatterKernel, dim3((unsigned int) grid), dim3(TWK_ADAPTIVE_TILE), 0, stream, ballots, budgets, tileOffsets, tilePathOffsets, totals, numElements, tiles, active, pathOffset);
  return totals;
}

} // namespace twk
