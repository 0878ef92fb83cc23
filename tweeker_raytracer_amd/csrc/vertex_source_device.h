// Vertices that already live on the device (include/tweeker_hip.h "A device-pointer source"): the complete definition of what
// twk_update_geometry_vertices_device and twk_refit_geometry_vertices_device write into the geometry's slice of the attribute array,
// shared by the kernels (vertex_source_kernels.hip) and the host form (twk_vertex_frames_host). tests/vertex_source_restate.py
// restates the frames in numpy, operation by operation in float32.
//
// A record is TwkTriangleAttributes, 12 floats: vertex[3], tangent[3], normal[3], texcoord[3]. A source is one of
//   attributes   numVertices records; the slice becomes the source, byte for byte
//   positions    x, y, z floats per vertex, `stride` bytes apart (>= 12, a multiple of 4); vertex[] of every record is replaced,
//                texcoord[] stays, and tangent[] / normal[] stay (recomputeFrames 0) or follow the new positions (1):
//
// FRAMES. adjacency: a CSR table, offsets[numVertices + 1] and triangles[offsets[numVertices]], that lists for every vertex the
// triangles whose indices name it, ascending by triangle, each triangle once (vertexAdjacency below builds it). For vertex v
//       s      = (+0, +0, +0);  for every adjacent triangle, in table order:  s = s + cross(p[i1] - p[i0], p[i2] - p[i0])
//                (i0, i1, i2) the triangle's own index order, p the NEW positions: emitTriangle's geometric normal, area-weighted
//       n'     = s * (1 / sqrtf(dot(s, s)))       unless no triangle names v, or dot(s, s) is zero or not finite: n' = n
//       t*     = t - n' * dot(n', t)
//       t'     = t* * (1 / sqrtf(dot(t*, t*)))    unless dot(t*, t*) is zero or not finite: t' = t
// with n, t the record's old normal and tangent, dot and cross as device_math.h writes them, every operation in float32 as written
// (-ffp-contract=off), sqrtf and the division correctly rounded. No float atomics: the order of every sum is the table's.
// What it is not: no welding (the two copies of a seam vertex each see their own triangles), not angle-weighted, no creases, no
// skinning (no bones, no weights).
//
// PREVIOUS POSITIONS. With a temporal history, and unless an earlier update since the history's frame has kept them, the thread that
// writes vertex v first writes the OLD vertex[] as a float4 (x, y, z, 0) into the geometry's kept array: keepPreviousPositions' rule.
#pragma once
#include "device_math.h"

#include <stddef.h>
#include <vector>

namespace twk {

// Position v of a strided source
TWK_HD V3 sourcePosition(const void* positions, size_t stride, size_t v)
{
  const float* p = reinterpret_cast<const float*>(static_cast<const char*>(positions) + stride * v);
  return v3(p[0], p[1], p[2]);
}

// Neither an infinity nor a NaN, by the exponent bits (the same answer on the host and on the device)
TWK_HD bool finiteBits(float x) { return (asUint(x) & 0x7f800000u) != 0x7f800000u; }
TWK_HD bool finitePosition(const V3& p) { return finiteBits(p.x) && finiteBits(p.y) && finiteBits(p.z); }
// A squared length a direction can be normalised by
TWK_HD bool usableLength(float squared) { return squared > 0.0f && finiteBits(squared); }

// FRAMES (above) of vertex v: tangent and normal in, the new ones out
TWK_HD void vertexFrame(const void* positions, size_t stride, const unsigned int* indices, const unsigned int* offsets, const unsigned int* triangles, size_t v,
                        V3& tangent, V3& normal)
{
  V3 s = v3(0.0f);
  const unsigned int first = offsets[v], end = offsets[v + 1];
  for (unsigned int k = first; k < end; ++k)
  {
    const unsigned int* triple = indices + 3 * (size_t) triangles[k];
    const V3 p0 = sourcePosition(positions, stride, triple[0]), p1 = sourcePosition(positions, stride, triple[1]), p2 = sourcePosition(positions, stride, triple[2]);
    s = s + cross(p1 - p0, p2 - p0);
  }
  const float ss = dot(s, s);
  if (first < end && usableLength(ss)) normal = s * (1.0f / sqrtf(ss));
  const V3 t = tangent - normal * dot(normal, tangent);
  const float tt = dot(t, t);
  if (usableLength(tt)) tangent = t * (1.0f / sqrtf(tt));
}

// The adjacency table of numVertices vertices under indices[numIndices] (every index below numVertices: the caller's check)
inline void vertexAdjacency(const unsigned int* indices, size_t numIndices, size_t numVertices, std::vector<unsigned int>& offsets, std::vector<unsigned int>& triangles)
{
  const auto named = [indices](size_t t, int j) { return j == 0 || (indices[3 * t + j] != indices[3 * t] && (j == 1 || indices[3 * t + 2] != indices[3 * t + 1])); };
  offsets.assign(numVertices + 1, 0u);
  for (size_t t = 0; t < numIndices / 3; ++t)
    for (int j = 0; j < 3; ++j) if (named(t, j)) offsets[indices[3 * t + j] + 1] += 1u; // a triangle that names a vertex twice is listed once
  for (size_t v = 0; v < numVertices; ++v) offsets[v + 1] += offsets[v];
  triangles.assign(offsets[numVertices], 0u);
  std::vector<unsigned int> next(offsets.begin(), offsets.end() - 1);
  for (size_t t = 0; t < numIndices / 3; ++t)
    for (int j = 0; j < 3; ++j) if (named(t, j)) triangles[next[indices[3 * t + j]]++] = (unsigned int) t;
}

// The records of a positions-mode source on the host: `before` with vertex[] from positions (stride 12) and, with recompute, the frames
inline void vertexFramesHost(const float* positions, size_t numVertices, const unsigned int* indices, size_t numIndices, const float* before, float* after, bool recompute = true)
{
  std::vector<unsigned int> offsets, triangles;
  if (recompute) vertexAdjacency(indices, numIndices, numVertices, offsets, triangles);
  for (size_t v = 0; v < numVertices; ++v)
  {
    const float* b = before + 12 * v;
    float* a = after + 12 * v;
    V3 tangent = v3(b[3], b[4], b[5]), normal = v3(b[6], b[7], b[8]);
    if (recompute) vertexFrame(positions, 12, indices, offsets.data(), triangles.data(), v, tangent, normal);
    a[0] = positions[3 * v]; a[1] = positions[3 * v + 1]; a[2] = positions[3 * v + 2];
    a[3] = tangent.x; a[4] = tangent.y; a[5] = tangent.z; a[6] = normal.x; a[7] = normal.y; a[8] = normal.z;
    a[9] = b[9]; a[10] = b[10]; a[11] = b[11];
  }
}

// vertex_source_kernels.hip. `slice`: the geometry's records in the attribute array (16-byte aligned); kept: its kept array, or
// nullptr when nothing is to be kept; lowest: one word, 0xffffffff before the check, the lowest vertex whose position is not finite after it
void launchVertexSourceCheck(const void* positions, size_t stride, unsigned int numVertices, unsigned int* lowest, hipStream_t stream);
void launchIngestAttributes(const float4* source, float4* slice, float4* kept, unsigned int numVertices, hipStream_t stream);
void launchIngestPositions(const void* positions, size_t stride, bool recompute, const unsigned int* indices, const unsigned int* offsets, const unsigned int* triangles,
                           float4* slice, float4* kept, unsigned int numVertices, hipStream_t stream);

} // namespace twk
