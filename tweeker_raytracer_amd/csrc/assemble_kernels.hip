// The kernel of twk_assemble: one launch moves every requested plane and layer of every source device from its packed
// launchWidth x H rows to the W x H rows of the assembled frame (assemble_device.h: the map, the groups). A pure stream: nothing is
// computed, every in-picture element is read once and written once, padding is neither read nor written.
//   blockIdx.z  the entry of the table: one (plane, layer, device)
//   blockIdx.y  TWK_ASSEMBLE_ROWS consecutive rows
//   blockIdx.x  256 groups of a launch row; a lane moves its group in each of the block's rows, all loads issued before the first
//               store so that TWK_ASSEMBLE_ROWS x 16 B per lane are in flight
// A group is 16 bytes (1 float4, 2 RGBA16F pixels, 4 counts) on the 16-byte path and one element otherwise; which one is the entry's
// groupShift, chosen per plane on the host (assembleGroupShift), uniform over the block. The grid's x extent is that of the entry
// with the most groups per row; the blocks past an entry's own row end return at once.
#include "assemble_device.h"

namespace twk {

#define TWK_ASSEMBLE_ROWS 4

// One row of a lane's group: where it goes and, when it is inside the picture, its bytes. False: padding, or a row past the frame.
template<typename T>
TWK_D bool assembleLoad(const AssembleShape& s, const AssembleEntry& e, const T* __restrict__ source, unsigned int xLaunch, unsigned int y, T& value, size_t& to)
{
  if (y >= (unsigned int) s.height) return false;
  const unsigned int x = assembleColumn(s, e.device, xLaunch, y);
  if (x >= (unsigned int) s.width) return false; // the first element of a group decides for all of it (assemble_device.h THE GROUPS)
  to    = ((size_t) y * (size_t) s.width + x) >> e.groupShift;
  value = source[((size_t) y * (size_t) s.launchWidth + xLaunch) >> e.groupShift];
  return true;
}

// The block's TWK_ASSEMBLE_ROWS rows of one group, in named registers (an indexed array of them would be placed in LDS)
template<typename T>
TWK_D void assembleMove(const AssembleShape& s, const AssembleEntry& e, unsigned int group, unsigned int yFirst)
{
  static_assert(TWK_ASSEMBLE_ROWS == 4, "one named register per row");
  const unsigned int xLaunch = group << e.groupShift;
  const T* __restrict__ source      = static_cast<const T*>(e.source);
  T* __restrict__       destination = static_cast<T*>(e.destination);
  T value0, value1, value2, value3;
  size_t to0 = 0, to1 = 0, to2 = 0, to3 = 0;
  const bool inside0 = assembleLoad(s, e, source, xLaunch, yFirst + 0, value0, to0);
  const bool inside1 = assembleLoad(s, e, source, xLaunch, yFirst + 1, value1, to1);
  const bool inside2 = assembleLoad(s, e, source, xLaunch, yFirst + 2, value2, to2);
  const bool inside3 = assembleLoad(s, e, source, xLaunch, yFirst + 3, value3, to3);
  if (inside0) destination[to0] = value0;
  if (inside1) destination[to1] = value1;
  if (inside2) destination[to2] = value2;
  if (inside3) destination[to3] = value3;
}

__global__ void __launch_bounds__(256) assembleKernel(AssembleShape s, AssembleTable table)
{
  const AssembleEntry& e = table.entry[blockIdx.z];
  const unsigned int group = blockIdx.x * 256 + threadIdx.x;
  if (group >= ((unsigned int) s.launchWidth >> e.groupShift)) return;
  const unsigned int yFirst = blockIdx.y * TWK_ASSEMBLE_ROWS;
  switch (e.elementShift + e.groupShift) // log2 of the bytes a lane moves per row
  {
    case 2:  assembleMove<unsigned int>(s, e, group, yFirst); break;
    case 3:  assembleMove<uint2>(s, e, group, yFirst); break;
    default: assembleMove<uint4>(s, e, group, yFirst); break;
  }
}

// `count` entries of the table, 1 <= count <= TWK_ASSEMBLE_MAX_ENTRIES
void launchAssemble(const AssembleShape& s, const AssembleTable& table, int count, hipStream_t stream)
{
  unsigned int groups = 1;
  for (int i = 0; i < count; ++i) groups = max(groups, (unsigned int) s.launchWidth >> table.entry[i].groupShift);
  const dim3 grid((groups + 255) / 256, ((unsigned int) s.height + TWK_ASSEMBLE_ROWS - 1) / TWK_ASSEMBLE_ROWS, (unsigned int) count);
  hipLaunchKernelGGL(assembleKernel, grid, dim3(256), 0, stream, s, table);
}

} // namespace twk
