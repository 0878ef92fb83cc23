// Per-vertex motion for the temporal history (twk_update_geometry_vertices, twk_render_geometry_motion): where the surface point a
// pixel sees was when the history was taken, as one float4 per pixel beside the geometry AOV — the previous-position plane.
// twk_update_geometry_vertices replaces the vertices of a geometry and keeps the temporal history; the first update since the
// history's frame keeps the geometry's positions as they were then (one float4 per vertex: x, y, z, 0 — a lane's fetch is one load),
// and the geometry is DEFORMED until a merge swaps the history. One matrix per instance (temporal_motion_device.h) cannot say where a
// point of a deformed mesh was; the hit's triangle and barycentrics can: the same barycentrics on the triangle's previous vertices,
// through the instance's object-to-world matrix as of the history's frame. This header is the complete definition, shared by the
// kernel (temporal_carry_kernels.hip geometryMotionKernel) and the host form (twk_previous_positions_host), and the step by which the
// temporal merges read the plane (temporalCarry, below);
// tests/temporal_carry_restate.py restates it statement for statement. Built with -ffp-contract=off (csrc/Makefile): every
// operation rounds once, as written.
//
// ---- the records, indexed by instance ------------------------------------------------------------------------------------------
//   TwkInstanceMotion (64 bytes)  X = M_prev . M_cur^-1 and `moved`, exactly the table of temporal_motion_device.h
//   TwkInstanceCarry  (64 bytes)  previousObjectToWorld[12]  Mp, the instance's object-to-world matrix as of the history's frame
//                                 deformed      0: nothing below is read
//                                 positionBase  first previous position of the instance's geometry in the array of previous positions
//                                 indexBase     first index of the instance's geometry in the index array
//                                 reserved      0
//
// ---- one pixel (previousPosition) ----------------------------------------------------------------------------------------------
//   miss (instance < 0):       (0, 0, 0, bits 0)
//   hit of instance i, primitive q (local to the geometry, for flattened and entered instances alike), barycentrics beta, gamma —
//   what traverse<false> returns and shading uses — and g as the geometry AOV writes it:
//     i < numCarry and carry[i].deformed:
//       (i0, i1, i2) = indices[indexBase + 3 q + 0 .. 2];     v_j = previousPositions[positionBase + i_j]
//       a    = (1 - beta) - gamma
//       o.k  = (a * v0.k + beta * v1.k) + gamma * v2.k                              k = x, y, z   (f32)
//       g'.k = ((Mp[k][0] o.x + Mp[k][1] o.y) + Mp[k][2] o.z) + Mp[k][3]
//     else: g' = temporalMove(motion, numMotion, g) — X g when instance i has moved (the same function, the same bits), else g's bits
//   written: (g'.xyz, bits of g.w)
// A g' that is not finite is written as it is: a merge that reads the plane finds no history there.
//
// ---- the step of a Carried build (temporalCarry), after temporalCandidate has passed on g ------------------------------------------
// The third way the merges obtain g' (temporal_device.h temporalGather, temporal_cascade_device.h temporalCascadePixel), beside "g
// itself" and temporalMove:
//   gp = plane[p];      no history unless bits(gp.w) == bits(g.w) and gp.xyz is finite
// Everything after it is the existing merge: the projection of gp, the taps' position test against gp, the cap, the blend, the trust.
// The extra compulsory stream of a Carried build is one coalesced 16-byte read per pixel; no table is read (the plane holds X g of a
// moved instance already).
//
// What it is not. No topology change (the indices stay), no motion blur, no emitting geometry (an instance that carries a light
// refuses the update), pinhole only, picture-shaped handles only (a packed tile buffer is refused). Whether the two records are
// staged in LDS as TWK_MOTION_STAGED_RECORDS stages the table: not measured; they are read from global memory, once per hit pixel.
#pragma once
#include "temporal_motion_device.h"

#include <vector>

namespace twk {

static_assert(sizeof(TwkInstanceCarry) == 64, "a carry record is 64 bytes");

// The step of a Carried build: gp = the plane's element of the pixel. False: no history.
TWK_HD bool temporalCarry(const float4& planeElement, const float4& g, float4& gp)
{
  gp = planeElement;
  return asUint(gp.w) == asUint(g.w) && finite3(gp);
}

// One carry record: its three rows and its four words
TWK_HD void carryRecord(const TwkInstanceCarry* carry, unsigned int i, float4& r0, float4& r1, float4& r2, uint4& words)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const float4* rows = reinterpret_cast<const float4*>(carry + i); // (a table on the device is 16-byte aligned)
  r0 = rows[0]; r1 = rows[1]; r2 = rows[2];
  words = *reinterpret_cast<const uint4*>(rows + 3);
#else
  const float* M = carry[i].previousObjectToWorld;
  r0 = make_float4(M[0], M[1], M[2], M[3]); r1 = make_float4(M[4], M[5], M[6], M[7]); r2 = make_float4(M[8], M[9], M[10], M[11]);
  words = make_uint4(carry[i].deformed, carry[i].positionBase, carry[i].indexBase, carry[i].reserved);
#endif
}

// The plane's element of a hit (above). previousPositions: four floats per vertex.
TWK_HD float4 previousPosition(const TwkInstanceMotion* motion, unsigned int numMotion, const TwkInstanceCarry* carry, unsigned int numCarry,
                               const unsigned int* indices, const float4* previousPositions, int instance, int primitive, float beta, float gamma, const float4& g)
{
  const unsigned int i = (unsigned int) instance;
  if (i < numCarry)
  {
    float4 r0, r1, r2;
    uint4 words;
    carryRecord(carry, i, r0, r1, r2, words);
    if (words.x != 0u)
    {
      const unsigned int* triple = indices + (size_t) words.z + 3u * (size_t) (unsigned int) primitive;
      const float4 v0 = previousPositions[(size_t) words.y + triple[0]], v1 = previousPositions[(size_t) words.y + triple[1]], v2 = previousPositions[(size_t) words.y + triple[2]];
      const float a = (1.0f - beta) - gamma;
      const float ox = (a * v0.x + beta * v1.x) + gamma * v2.x;
      const float oy = (a * v0.y + beta * v1.y) + gamma * v2.y;
      const float oz = (a * v0.z + beta * v1.z) + gamma * v2.z;
      return make_float4(((r0.x * ox + r0.y * oy) + r0.z * oz) + r0.w, ((r1.x * ox + r1.y * oy) + r1.z * oz) + r1.w, ((r2.x * ox + r2.y * oy) + r2.z * oz) + r2.w, g.w);
    }
  }
  float4 gp;
  temporalMove(motion, numMotion, g, gp); // gp.w = g.w; a gp that is not finite is written as it is
  return gp;
}

// twk_previous_positions_host: the plane of numPixels pixels from host arrays. hits: (t, beta, gamma) per pixel; instance < 0: a miss.
inline void previousPositionsHost(const float* hits, const int* instance, const int* primitive, const float* geometry, size_t numPixels, const unsigned int* indices,
                                  const float* previousPositions, size_t numPositions, const TwkInstanceMotion* motion, unsigned int numMotion, const TwkInstanceCarry* carry,
                                  unsigned int numCarry, float* plane)
{
  std::vector<float4> positions(numPositions); // (a caller's array of floats need not be 16-byte aligned)
  if (numPositions > 0) memcpy(positions.data(), previousPositions, numPositions * sizeof(float4));
  for (size_t p = 0; p < numPixels; ++p)
  {
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (instance[p] >= 0)
    {
      float4 g;
      memcpy(&g, geometry + 4 * p, sizeof(float4));
      out = previousPosition(motion, numMotion, carry, numCarry, indices, positions.data(), instance[p], primitive[p], hits[3 * p + 1], hits[3 * p + 2], g);
    }
    memcpy(plane + 4 * p, &out, sizeof(float4));
  }
}

} // namespace twk
