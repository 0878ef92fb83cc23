// The kernels of a device-pointer vertex source (vertex_source_device.h is the definition; device_vertex_source.hip the caller): one
// thread per vertex, every thread writes its own record and nothing else, so no launch has a race and none needs an atomic but the check's.
//   vertexSourceCheckKernel   read-only: atomicMin of the index of every vertex whose position is not finite into one word
//   ingestAttributesKernel    a record as three 16-byte loads and three 16-byte stores
//   ingestPositionsKernel     three strided floats; with RECOMPUTE the frames: a gather of the adjacent triangles' positions from the
//                             source (the new positions of the neighbours, which no thread writes), in the table's order
// Compulsory bytes per vertex: attributes 48 read + 48 written; positions 12 read + 16 read + 16 written, with the frames 48 read + 48
// written, 8 of offsets, and per adjacent triangle 4 of table + 12 of indices + 36 of positions (cached: ~6 triangles share a vertex).
// Keeping the previous positions adds 16 written (and in attributes mode 16 read).
#include "vertex_source_device.h"

namespace twk {

__global__ void __launch_bounds__(256) vertexSourceCheckKernel(const void* __restrict__ positions, size_t stride, unsigned int numVertices, unsigned int* lowest)
{
  const unsigned int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= numVertices) return;
  if (!finitePosition(sourcePosition(positions, stride, v))) atomicMin(lowest, v);
}

__global__ void __launch_bounds__(256) ingestAttributesKernel(const float4* __restrict__ source, float4* __restrict__ slice, float4* __restrict__ kept, unsigned int numVertices)
{
  const unsigned int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= numVertices) return;
  const size_t r = 3 * (size_t) v;
  const float4 a = source[r], b = source[r + 1], c = source[r + 2];
  if (kept) { const float4 old = slice[r]; kept[v] = make_float4(old.x, old.y, old.z, 0.0f); }
  slice[r] = a; slice[r + 1] = b; slice[r + 2] = c;
}

template<bool RECOMPUTE>
__global__ void __launch_bounds__(256) ingestPositionsKernel(const void* __restrict__ positions, size_t stride, const unsigned int* __restrict__ indices,
                                                             const unsigned int* __restrict__ offsets, const unsigned int* __restrict__ triangles,
                                                             float4* __restrict__ slice, float4* __restrict__ kept, unsigned int numVertices)
{
  const unsigned int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= numVertices) return;
  const size_t r = 3 * (size_t) v;
  const V3 p = sourcePosition(positions, stride, v);
  const float4 a = slice[r]; // vertex.xyz, tangent.x
  if (kept) kept[v] = make_float4(a.x, a.y, a.z, 0.0f);
  if (!RECOMPUTE) { slice[r] = make_float4(p.x, p.y, p.z, a.w); return; }
  const float4 b = slice[r + 1]; // tangent.yz, normal.xy
  V3 tangent = v3(a.w, b.x, b.y), normal = v3(b.z, b.w, slice[r + 2].x);
  vertexFrame(positions, stride, indices, offsets, triangles, v, tangent, normal);
  slice[r] = make_float4(p.x, p.y, p.z, tangent.x);
  slice[r + 1] = make_float4(tangent.y, tangent.z, normal.x, normal.y);
  reinterpret_cast<float*>(slice + r + 2)[0] = normal.z; // the texture coordinates stay
}

static dim3 perVertex(unsigned int numVertices) { return dim3((numVertices + 255u) / 256u); }

void launchVertexSourceCheck(const void* positions, size_t stride, unsigned int numVertices, unsigned int* lowest, hipStream_t stream)
{
  hipLaunchKernelGGL(vertexSourceCheckKernel, perVertex(numVertices), dim3(256), 0, stream, positions, stride, numVertices, lowest);
}

void launchIngestAttributes(const float4* source, float4* slice, float4* kept, unsigned int numVertices, hipStream_t stream)
{
  hipLaunchKernelGGL(ingestAttributesKernel, perVertex(numVertices), dim3(256), 0, stream, source, slice, kept, numVertices);
}

void launchIngestPositions(const void* positions, size_t stride, bool recompute, const unsigned int* indices, const unsigned int* offsets, const unsigned int* triangles,
                           float4* slice, float4* kept, unsigned int numVertices, hipStream_t stream)
{
  if (recompute) hipLaunchKernelGGL(ingestPositionsKernel<true>, perVertex(numVertices), dim3(256), 0, stream, positions, stride, indices, offsets, triangles, slice, kept, numVertices);
  else hipLaunchKernelGGL(ingestPositionsKernel<false>, perVertex(numVertices), dim3(256), 0, stream, positions, stride, indices, offsets, triangles, slice, kept, numVertices);
}

} // namespace twk
