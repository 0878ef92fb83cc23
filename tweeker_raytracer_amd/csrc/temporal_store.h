// The store of the three outputs of a temporal merge at one pixel (temporal_device.h: colourOut, historyOut, momentsOut), for the
// kernels of the plain and of the rectified merge. Kernel side only: the host forms write float arrays of their own.
#pragma once
#include "pixel_formats.h"

namespace twk {

// A pixel that merged history: colourOut = narrow(colour) (RGBA16F: round to nearest even, once), historyOut = colour in f32,
// momentsOut = moments. An output that is nullptr is not written.
template<typename Pixel>
__device__ inline void temporalStoreMerged(size_t p, const float4& colour, const float4& moments, Pixel* colourOut, float4* historyOut, float4* momentsOut)
{
  if (colourOut) colourOut[p] = pixelOf<Pixel>(colour);
  if (historyOut) historyOut[p] = colour;
  if (momentsOut) momentsOut[p] = moments;
}

// A pixel that passes through: colourOut = the frame's pixel raw, its bits; historyOut = cur = widen(raw); momentsOut = mc
template<typename Pixel>
__device__ inline void temporalStorePassThrough(size_t p, const Pixel& raw, const float4& cur, const float4& mc, Pixel* colourOut, float4* historyOut, float4* momentsOut)
{
  if (colourOut) colourOut[p] = raw;
  if (historyOut) historyOut[p] = cur;
  if (momentsOut) momentsOut[p] = mc;
}

} // namespace twk
