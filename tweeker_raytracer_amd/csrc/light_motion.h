// The light an emitting instance carries, moved with it (twk_enable_emitter_motion; include/tweeker_hip.h "Moving a light"). Host
// only, plain C++, no HIP: included by the entry points (device_scene.hip, device_api.hip) and by the stand-alone program
// tests/light_motion_host.cpp. The definition below is complete; tests/light_motion_restate.py restates it statement for statement.
// Built with -ffp-contract=off (csrc/Makefile): every operation rounds once, as written.
//
// ---- the anchor ---------------------------------------------------------------------------------------------------------------
// A light's anchor is the pair (its definition, its instance's object-to-world matrix), taken when an emitter of that light is first
// moved. A moved definition is always derived from the anchor, never from the one derived before it, so roundings do not pile up and
// A -> B -> A is exact. twk_update_light drops the light's anchor (the next move anchors on the new definition and the matrix of that
// moment); twk_init_lights, twk_build and twk_clear_scene drop every anchor.
//
// ---- the derivation (lightMoved = twk_light_moved_host): anchor definition L0, anchor matrix A, new matrix N, all float ---------
//   N has A's 48 bytes: the result is L0's 80 bytes. Otherwise, in DOUBLE from the float inputs:
//   the cofactor inverse of temporal_motion_device.h instanceMotion, unrounded (a = A's 3 x 3, t its last column):
//     c00 = a11 a22 - a12 a21;  c01 = a12 a20 - a10 a22;  c02 = a10 a21 - a11 a20;  det = (a00 c00 + a01 c01) + a02 c02;  r = 1 / det
//     i00 = c00 r;  i01 = (a02 a21 - a01 a22) r;  i02 = (a01 a12 - a02 a11) r
//     i10 = c01 r;  i11 = (a00 a22 - a02 a20) r;  i12 = (a02 a10 - a00 a12) r
//     i20 = c02 r;  i21 = (a01 a20 - a00 a21) r;  i22 = (a00 a11 - a01 a10) r;   ik3 = -((ik0 t0 + ik1 t1) + ik2 t2)
//   D = N . A^-1, row by row, left to right, KEPT in double:
//     D[k][j] = (n[k][0] i0j + n[k][1] i1j) + n[k][2] i2j     j = 0, 1, 2;     D[k][3] = ((n[k][0] i03 + n[k][1] i13) + n[k][2] i23) + n[k][3]
//   position.k = (float) (((D[k][0] p.x + D[k][1] p.y) + D[k][2] p.z) + D[k][3])       p = L0.position
//   vecU.k     = (float) ((D[k][0] u.x + D[k][1] u.y) + D[k][2] u.z)                   u = L0.vecU; vecV likewise
//   on the rounded floats, in float (≙ createLights, reference Application.cpp:616-618 with vector_math.h's cross, length and
//   division by a scalar; host/application.cpp createLights):
//     n = (U.y V.z - U.z V.y, U.z V.x - U.x V.z, U.x V.y - U.y V.x);  area = sqrtf((n.x n.x + n.y n.y) + n.z n.z);  inv = 1 / area
//     normal = n inv
//   the mirror: dD = (D00 e00 + D01 e01) + D02 e02 with e00 = D11 D22 - D12 D21, e01 = D12 D20 - D10 D22, e02 = D10 D21 - D11 D20
//   (double); dD < 0: normal = -normal. The emitter's lit side is decided by normalize(transformNormal(worldToObject, ng))
//   (shade_device.h), an inverse transpose, which a mirror does not flip — cross(vecU, vecV) does.
//   type, emission and the three unused words are L0's.
// Refused (the text returned; nullptr: done): a light that is no parallelogram; a matrix that is not finite, or an anchor matrix whose
// det is zero or not finite; a derived area that is zero or not finite, or a derived component that is not finite.
//
// What it is not. It moves whatever definition it was given: nothing checks that the definition matched the instance's quad in the
// first place. One instance per light, parallelograms only, no deformation (the vertex calls keep refusing an emitting geometry), no
// environment light.
#pragma once
#include "../../include/tweeker_hip.h"

#include <math.h>
#include <string.h>

namespace twk {

inline bool lightFinite(double v) { return v - v == 0.0; }

// The anchor of one light (TwkDevice_t::lightAnchors, indexed by light)
struct LightAnchor
{
  bool valid = false;
  TwkLightDefinition definition;
  float transform[12];
};

static const char* const lightNotParallelogram = "the light is not a TWK_LIGHT_PARALLELOGRAM: only a parallelogram moves with its instance";
static const char* const lightBadTransform = "a transform is not finite, or the anchor transform's 3 x 3 determinant is zero or not finite";
static const char* const lightDegenerate = "the moved light is degenerate: its area is zero or not finite, or a component of it is not finite";

// twk_light_moved_host after its NULL checks; nullptr: `out` is the moved definition, else the refusal's text and `out` is untouched
inline const char* lightMoved(const TwkLightDefinition& anchor, const float anchorTransform[12], const float transform[12], TwkLightDefinition& out)
{
  if (anchor.type != TWK_LIGHT_PARALLELOGRAM) return lightNotParallelogram;
  for (int j = 0; j < 12; ++j) if (!lightFinite(anchorTransform[j]) || !lightFinite(transform[j])) return lightBadTransform;
  const double a00 = anchorTransform[0], a01 = anchorTransform[1], a02 = anchorTransform[2],  t0 = anchorTransform[3];
  const double a10 = anchorTransform[4], a11 = anchorTransform[5], a12 = anchorTransform[6],  t1 = anchorTransform[7];
  const double a20 = anchorTransform[8], a21 = anchorTransform[9], a22 = anchorTransform[10], t2 = anchorTransform[11];
  const double c00 = a11 * a22 - a12 * a21;
  const double c01 = a12 * a20 - a10 * a22;
  const double c02 = a10 * a21 - a11 * a20;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  if (!lightFinite(det) || det == 0.0) return lightBadTransform;
  if (memcmp(anchorTransform, transform, 12 * sizeof(float)) == 0) { memcpy(&out, &anchor, sizeof(out)); return nullptr; }
  const double r = 1.0 / det;
  double inv[3][4];
  inv[0][0] = c00 * r; inv[0][1] = (a02 * a21 - a01 * a22) * r; inv[0][2] = (a01 * a12 - a02 * a11) * r;
  inv[1][0] = c01 * r; inv[1][1] = (a00 * a22 - a02 * a20) * r; inv[1][2] = (a02 * a10 - a00 * a12) * r;
  inv[2][0] = c02 * r; inv[2][1] = (a01 * a20 - a00 * a21) * r; inv[2][2] = (a00 * a11 - a01 * a10) * r;
  for (int k = 0; k < 3; ++k) inv[k][3] = -((inv[k][0] * t0 + inv[k][1] * t1) + inv[k][2] * t2);
  double D[3][4];
  for (int k = 0; k < 3; ++k)
  {
    const double n0 = transform[4 * k], n1 = transform[4 * k + 1], n2 = transform[4 * k + 2], n3 = transform[4 * k + 3];
    for (int j = 0; j < 3; ++j) D[k][j] = (n0 * inv[0][j] + n1 * inv[1][j]) + n2 * inv[2][j];
    D[k][3] = ((n0 * inv[0][3] + n1 * inv[1][3]) + n2 * inv[2][3]) + n3;
  }
  TwkLightDefinition l;
  memcpy(&l, &anchor, sizeof(l)); // type, emission and the unused words
  const double px = anchor.position[0], py = anchor.position[1], pz = anchor.position[2];
  const double ux = anchor.vecU[0], uy = anchor.vecU[1], uz = anchor.vecU[2];
  const double vx = anchor.vecV[0], vy = anchor.vecV[1], vz = anchor.vecV[2];
  for (int k = 0; k < 3; ++k)
  {
    l.position[k] = (float) (((D[k][0] * px + D[k][1] * py) + D[k][2] * pz) + D[k][3]);
    l.vecU[k] = (float) ((D[k][0] * ux + D[k][1] * uy) + D[k][2] * uz);
    l.vecV[k] = (float) ((D[k][0] * vx + D[k][1] * vy) + D[k][2] * vz);
  }
  const float nx = l.vecU[1] * l.vecV[2] - l.vecU[2] * l.vecV[1];
  const float ny = l.vecU[2] * l.vecV[0] - l.vecU[0] * l.vecV[2];
  const float nz = l.vecU[0] * l.vecV[1] - l.vecU[1] * l.vecV[0];
  l.area = sqrtf((nx * nx + ny * ny) + nz * nz);
  if (!lightFinite(l.area) || l.area == 0.0f) return lightDegenerate;
  const float inverse = 1.0f / l.area;
  l.normal[0] = nx * inverse; l.normal[1] = ny * inverse; l.normal[2] = nz * inverse;
  const double e00 = D[1][1] * D[2][2] - D[1][2] * D[2][1];
  const double e01 = D[1][2] * D[2][0] - D[1][0] * D[2][2];
  const double e02 = D[1][0] * D[2][1] - D[1][1] * D[2][0];
  const double mirror = (D[0][0] * e00 + D[0][1] * e01) + D[0][2] * e02;
  if (mirror < 0.0) { l.normal[0] = -l.normal[0]; l.normal[1] = -l.normal[1]; l.normal[2] = -l.normal[2]; }
  for (int k = 0; k < 3; ++k)
    if (!lightFinite(l.position[k]) || !lightFinite(l.vecU[k]) || !lightFinite(l.vecV[k]) || !lightFinite(l.normal[k])) return lightDegenerate;
  memcpy(&out, &l, sizeof(out));
  return nullptr;
}

} // namespace twk
