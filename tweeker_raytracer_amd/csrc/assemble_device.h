// Assembling a tiled frame (twk_assemble, twk_assemble_devices): with distribution 1 and N devices every device renders its
// checkerboard share of a W x H picture into packed launchWidth x H buffers, one per plane (beauty, AOVs, moments, sample counts, the
// cascade's layers); this is how they become W x H buffers on one device. The definition below is complete and is compiled once for
// the kernel (assemble_kernels.hip) and once for the host (twk_assemble_host, device_assemble.hip); tests/assemble_restate.py
// restates it in numpy. Nothing is computed: every element is moved as the bytes it is.
//
// THE MAP  launch index (xLaunch, y) of device d of N, tiles of tileSizeX x tileSizeY (powers of two):
//   xBlock = xLaunch >> log2(tileSizeX);  yBlock = y >> log2(tileSizeY)
//   xTile  = xBlock * N + (d + yBlock) % N                                   (the rotation that makes the checkerboard)
//   x      = xTile * tileSizeX + (xLaunch & (tileSizeX - 1))
//   x < W:  destination[y * W + x] = source d [y * launchWidth + xLaunch];  else the launch index is padding: not read, not written
// which is distribute() (shade_device.h), compositorKernel and twk_tile_column. launchWidth = ceil(W / N) rounded up to a multiple of
// tileSizeX (twk_launch_width). N == 1: launchWidth == W and the map is the identity. Every picture element has exactly one launch
// index, so no element is written twice and none is left out.
//
// THE PLANES  an element is 4 B (sample counts), 8 B (an RGBA16F pixel) or 16 B (a float4: RGBA32F pixel, moments, a cascade layer).
// A plane of K layers is K planes: source [K][H][launchWidth], destination [K][H][W].
//
// THE GROUPS  a lane moves 16 bytes where the shape allows: G = 16 / elementBytes consecutive launch indices starting at a multiple
// of G. They lie in one tile and map to G consecutive picture columns starting at a multiple of G when tileSizeX >= G, and source and
// destination are 16-byte aligned in every row when W * elementBytes is a multiple of 16 and both base pointers are (launchWidth is
// a multiple of tileSizeX, or W itself when N == 1). Then x < W for the first element of a group means the whole group is inside
// the picture (W is a multiple of G): no group is cut. Where a condition fails (assembleGroupShift: an odd width with counts or
// half pixels, a tile 1 or 2 wide, a base pointer that is not aligned) the plane is moved element by element, G = 1.
#pragma once
#include "device_types.h"

namespace twk {

// The frame's geometry as the map needs it
struct AssembleShape
{
  int width, height, launchWidth, deviceCount, tileSizeX, tileShiftX, tileShiftY;
};

// One (plane, layer, device) of a launch: where its packed rows are, where its picture rows go, and how it is moved
struct AssembleEntry
{
  const void*  source;       // [height][launchWidth] elements
  void*        destination;  // [height][width] elements
  unsigned int device;       // d of the map
  unsigned int elementShift; // log2(elementBytes): 2, 3 or 4
  unsigned int groupShift;   // log2(G): 0 = element by element; elementShift + groupShift == 4 on the 16-byte path
  unsigned int reserved;
};

// The table of a launch, a kernel argument: 13 planes and layers (5 planes + 8 layers) of 9 devices fit; more are launched in pieces
#define TWK_ASSEMBLE_MAX_ENTRIES 120
struct AssembleTable
{
  AssembleEntry entry[TWK_ASSEMBLE_MAX_ENTRIES];
};

TWK_HD int assembleLaunchWidth(int width, int tileSizeX, int deviceCount)
{
  if (deviceCount <= 1) return width;
  const int w = (width + deviceCount - 1) / deviceCount, mask = tileSizeX - 1;
  return (w + mask) & ~mask;
}

TWK_HD unsigned int assembleColumn(const AssembleShape& s, unsigned int device, unsigned int xLaunch, unsigned int y)
{
  const unsigned int xBlock = xLaunch >> s.tileShiftX;
  const unsigned int yBlock = y >> s.tileShiftY;
  const unsigned int xTile  = xBlock * (unsigned int) s.deviceCount + ((device + yBlock) % (unsigned int) s.deviceCount);
  return xTile * (unsigned int) s.tileSizeX + (xLaunch & (unsigned int) (s.tileSizeX - 1));
}

// log2 of the elements a lane moves at once: 4 - elementShift on the 16-byte path, 0 element by element
inline unsigned int assembleGroupShift(const AssembleShape& s, unsigned int elementShift, const void* source, const void* destination)
{
  const size_t elementBytes = (size_t) 1 << elementShift;
  const bool tile    = (size_t) s.tileSizeX * elementBytes >= 16;
  const bool rows    = ((size_t) s.width * elementBytes) % 16 == 0 && ((size_t) s.launchWidth * elementBytes) % 16 == 0;
  const bool aligned = ((uintptr_t) source % 16 == 0) && ((uintptr_t) destination % 16 == 0);
  return (tile && rows && aligned) ? 4u - elementShift : 0u;
}

} // namespace twk
