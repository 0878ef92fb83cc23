// Motion of instances in the temporal merges (twk_update_instance_transform, twk_temporal_accumulate_moving): one matrix per
// instance that carries a surface point of THIS frame to where the same point of the object was when the history was taken.
// twk_update_instance_transform replaces an instance's object-to-world matrix M and keeps the temporal history; a point of instance
// i now at world g was at g' = M_prev,i . M_cur,i^-1 . g in the history's frame, so the history is looked up at the projection of
// g' and a tap belongs to the surface when the history's geometry lies near g'. Everything else of the three merges
// (temporal_device.h, temporal_rectify_device.h, temporal_cascade_device.h) is unchanged: this header adds the record, the host
// function that fills it and the one step temporalGather and temporalCascadePixel take in their `Moving` builds. The definition
// below is complete; tests/temporal_motion_restate.py restates it statement for statement. Built with -ffp-contract=off
// (csrc/Makefile): every operation rounds once, as written.
//
// ---- the record (TwkInstanceMotion, 64 bytes; a table has one per instance, indexed by instance) -----------------------------
//   previousFromCurrent[12]   X, row-major 3 x 4       moved   0: X is not read, the instance is where it was       reserved[3]
//
// ---- the host function (instanceMotion = twk_instance_motion) -----------------------------------------------------------------
// previous, current: row-major 3 x 4 object-to-world matrices (p, c below). moved = 0 when their 24 words are bit-equal; X is then
// written as the identity. Otherwise X = previous . current^-1, in DOUBLE from the float inputs, each element rounded to float once:
//   the cofactor inverse of the scene build's invertAffine, unrounded:
//     c00 = a11 a22 - a12 a21;  c01 = a12 a20 - a10 a22;  c02 = a10 a21 - a11 a20;  det = (a00 c00 + a01 c01) + a02 c02;  r = 1 / det
//     i00 = c00 r;  i01 = (a02 a21 - a01 a22) r;  i02 = (a01 a12 - a02 a11) r
//     i10 = c01 r;  i11 = (a00 a22 - a02 a20) r;  i12 = (a02 a10 - a00 a12) r
//     i20 = c02 r;  i21 = (a01 a20 - a00 a21) r;  i22 = (a00 a11 - a01 a10) r
//     ik3 = -((ik0 t0 + ik1 t1) + ik2 t2)                                                  (a = current's 3 x 3, t its last column)
//   the product, row by row, left to right:
//     X[k][j] = (p[k][0] i0j + p[k][1] i1j) + p[k][2] i2j      j = 0, 1, 2;       X[k][3] = ((p[k][0] i03 + p[k][1] i13) + p[k][2] i23) + p[k][3]
// Refused: an input that is not finite, and a current whose det is zero or not finite.
//
// ---- the step of a Moving build (temporalMove), after temporalCandidate has passed on g ----------------------------------------
//   i = bits(g.w) - 1
//   if i < numMotion and motion[i].moved:
//     g'.k = ((X[k][0] g.x + X[k][1] g.y) + X[k][2] g.z) + X[k][3]      k = 0, 1, 2 (f32);     no history unless g'.xyz is finite
//   else g' = g (its bits);       g'.w = g.w in both cases
//   (fx, fy, vv) = temporalProject(g'):  vv = |g' - P'|^2;  a tap belongs when temporalTapGeometry(g', hg, vv):
//   bits(hg.w) == bits(g.w) and distance2(hg, g') <= tol2 vv
// The record is read once per pixel, before the projection, as three 16-byte loads and one word. The table is small and nearly
// wave-uniform (a wave's 64 pixels see one or two instances), so the loads of a wave fall into one or two cache lines — or, for a
// table of at most TWK_MOTION_STAGED_RECORDS records, into the block's LDS copy of it (below: measured, the faster of the two).
//
// What it is not. One rigid or affine matrix per INSTANCE: no deforming geometry and no per-vertex motion here (temporal_carry_device.h:
// the previous-position plane of a deformed mesh and the Carried builds that read it), no motion blur. The light
// an emitting instance carries moves with it only under twk_enable_emitter_motion (light_motion.h; else the instance is refused). Shadows and
// inter-reflections the move changes elsewhere in the picture are stale history like any light edit: the rectified merge discounts
// them, the plain merge fades them at the cap. A miss never has history, and the lens is the pinhole.
#pragma once
#include "denoise_device.h"            // finite1, finite3
#include "../../include/tweeker_hip.h" // TwkInstanceMotion

#include <string.h>

namespace twk {

static_assert(sizeof(TwkInstanceMotion) == 64, "a motion record is 64 bytes");

TWK_HD bool motionFinite(double v) { return v - v == 0.0; }

// twk_instance_motion; false: refused (an input that is not finite, a singular current)
inline bool instanceMotion(const float previous[12], const float current[12], TwkInstanceMotion& out)
{
  for (int j = 0; j < 12; ++j) if (!finite1(previous[j]) || !finite1(current[j])) return false;
  memset(&out, 0, sizeof(out));
  const double a00 = current[0], a01 = current[1], a02 = current[2],  t0 = current[3];
  const double a10 = current[4], a11 = current[5], a12 = current[6],  t1 = current[7];
  const double a20 = current[8], a21 = current[9], a22 = current[10], t2 = current[11];
  const double c00 = a11 * a22 - a12 * a21;
  const double c01 = a12 * a20 - a10 * a22;
  const double c02 = a10 * a21 - a11 * a20;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  if (!motionFinite(det) || det == 0.0) return false;
  if (memcmp(previous, current, 12 * sizeof(float)) == 0)
  {
    out.previousFromCurrent[0] = 1.0f; out.previousFromCurrent[5] = 1.0f; out.previousFromCurrent[10] = 1.0f;
    return true;
  }
  const double r = 1.0 / det;
  double inv[3][4];
  inv[0][0] = c00 * r; inv[0][1] = (a02 * a21 - a01 * a22) * r; inv[0][2] = (a01 * a12 - a02 * a11) * r;
  inv[1][0] = c01 * r; inv[1][1] = (a00 * a22 - a02 * a20) * r; inv[1][2] = (a02 * a10 - a00 * a12) * r;
  inv[2][0] = c02 * r; inv[2][1] = (a01 * a20 - a00 * a21) * r; inv[2][2] = (a00 * a11 - a01 * a10) * r;
  for (int k = 0; k < 3; ++k) inv[k][3] = -((inv[k][0] * t0 + inv[k][1] * t1) + inv[k][2] * t2);
  for (int k = 0; k < 3; ++k)
  {
    const double p0 = previous[4 * k], p1 = previous[4 * k + 1], p2 = previous[4 * k + 2], p3 = previous[4 * k + 3];
    for (int j = 0; j < 3; ++j) out.previousFromCurrent[4 * k + j] = (float) ((p0 * inv[0][j] + p1 * inv[1][j]) + p2 * inv[2][j]);
    out.previousFromCurrent[4 * k + 3] = (float) (((p0 * inv[0][3] + p1 * inv[1][3]) + p2 * inv[2][3]) + p3);
  }
  out.moved = 1u;
  return true;
}

// Whether a 3 x 4 object-to-world matrix can be an instance's: finite, with a 3 x 3 determinant (in double, as above) that is
// finite and not zero
inline bool instanceTransformUsable(const float m[12])
{
  TwkInstanceMotion unused;
  return instanceMotion(m, m, unused);
}

// One record of the table: its three rows and its `moved` word. The kernel reads 16-byte words (a table on the device is 16-byte
// aligned: the entry points refuse another); a host array of records need not be, and is read by floats.
TWK_HD void motionRecord(const TwkInstanceMotion* motion, unsigned int i, float4& r0, float4& r1, float4& r2, unsigned int& moved)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const float4* rows = reinterpret_cast<const float4*>(motion + i);
  r0 = rows[0]; r1 = rows[1]; r2 = rows[2];
  moved = motion[i].moved;
#else
  const float* X = motion[i].previousFromCurrent;
  r0 = make_float4(X[0], X[1], X[2], X[3]); r1 = make_float4(X[4], X[5], X[6], X[7]); r2 = make_float4(X[8], X[9], X[10], X[11]);
  moved = motion[i].moved;
#endif
}

// The step of a Moving build: gp = g' (above). False: no history (g' is not finite).
TWK_HD bool temporalMove(const TwkInstanceMotion* motion, unsigned int numMotion, const float4& g, float4& gp)
{
  gp = g;
  const unsigned int i = asUint(g.w) - 1u; // (a candidate: bits(g.w) != 0)
  if (!(i < numMotion)) return true;
  float4 r0, r1, r2;
  unsigned int moved;
  motionRecord(motion, i, r0, r1, r2, moved);
  if (moved == 0u) return true;
  gp.x = ((r0.x * g.x + r0.y * g.y) + r0.z * g.z) + r0.w;
  gp.y = ((r1.x * g.x + r1.y * g.y) + r1.z * g.z) + r1.w;
  gp.z = ((r2.x * g.x + r2.y * g.y) + r2.z * g.z) + r2.w;
  return finite3(gp);
}

// Where the kernels of the Moving builds read the table from. A table of at most TWK_MOTION_STAGED_RECORDS records is copied into
// LDS by every block (256 threads, 16 bytes each per round; 4 KiB at 64 records) and read from there; a larger one, and every table
// when the macro is 0, is read from global memory by each pixel. Both compute the same bits. Decided by an A/B on the MI355X
// (tools/temporal_motion_time.py on builds of tools/ab_variant.sh with -DTWK_MOTION_STAGED_RECORDS=0 and =64;
// profiles/r23_temporal_motion.md): at 1080p with half of the hit pixels on moved instances the staged build costs -0.2 / +0.3 /
// +1.0 us over its parent build (plain / rectified / cascade) where the global one costs +0.5 / +1.3 / +1.8 us — 1 % of the call,
// the same sign in every run and in both output formats. Tables above 64 records are not measured and stay in global memory.
#ifndef TWK_MOTION_STAGED_RECORDS
#define TWK_MOTION_STAGED_RECORDS 64
#endif
#define TWK_MOTION_LDS_RECORDS (TWK_MOTION_STAGED_RECORDS > 0 ? TWK_MOTION_STAGED_RECORDS : 1)

#if defined(__HIPCC__)
// Staged = true: the block's copy of the table (numMotion <= TWK_MOTION_STAGED_RECORDS: the launcher's choice), every thread of the
// block calls it before any leaves; Staged = false: the table where it is
template<bool Staged>
__device__ __forceinline__ const TwkInstanceMotion* motionTable(const TwkInstanceMotion* motion, unsigned int numMotion, TwkInstanceMotion* lds, unsigned int blockThreads)
{
  if (!Staged) return motion;
  const float4* from = reinterpret_cast<const float4*>(motion);
  float4* to = reinterpret_cast<float4*>(lds);
  for (unsigned int i = threadIdx.x; i < 4u * numMotion; i += blockThreads) to[i] = from[i];
  __syncthreads();
  return lds;
}
#endif

} // namespace twk
