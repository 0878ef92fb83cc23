// The records of a wavefront pass: what every word of a queued ray, a shadow ray and a hit record means, and the ONE place that
// reads and writes them. traceKernel, traceOverflowKernel, shadeKernel, generateKernel and the host build of the kernels
// (oracle/host_kernels.cpp) go through the functions below; the streams themselves are declared, listed and carved in
// device_types.h (LaunchParams, TWK_PATH_STREAMS).
//
// Indices. A queue is TWK_QUEUE_SEGMENTS regions of the same arrays (device_types.h "queue segments"): a consumer's VIRTUAL slot v
// is RECORD physicalSlot(v) of the queue streams; the hit record it writes / reads stays indexed by v. Queue 0 is the identity.
//
// A record has three forms.
//
// FULL — every stream is written and read:
//   queued ray   rayOrg[q] = origin.xyz, tmin      rayDir[q] = direction.xyz, tmax (< 0: an inactive launch index)
//                rayPixel[q] = launch index        raySeedFlags[q] = LCG state, path word      rayThroughput[q] = throughput.xyz, pdf
//   shadow ray   shadowOrg = origin.xyz, tmin      shadowDir = direction.xyz, tmax
//                shadowPixel = launch index        shadowPending = pending contribution.xyz, the seed the cutout test draws from
//   hit          hitRecord = t, beta, gamma, triangle slot (-1: a miss)      hitInstance = instance (-1: a miss)
//
// PACKED (LaunchParams::packedQueue; the queues shadeKernel writes, every depth >= 1) — the tmin / tmax of a continuation ray are
// the constants sceneEpsilon / RT_DEFAULT_MAX, so the record's two .w words carry the path instead:
//   rayOrg[q].w = launch index (TWK_PACKED_PIXEL_BITS bits) | FLAG_DIFFUSE << 27 | FLAG_ALBEDO << 28 | (volume stack index + 1) << 29
//   rayDir[q].w = the LCG state
// and rayPixel / raySeedFlags are neither written nor read: 12 bytes less per path and bounce on both sides (the big shade launches
// sit at the HBM rate). Scenes without cutout opacity only — its candidate loop keeps a per-ray tmin in the record —
// and passes of fewer than 2^27 paths. Queue 0 is computed (PRIMARY) or written by generateKernel: always full.
//
// SLIM (LaunchParams::slimSlotBits != 0: the bits a triangle slot takes; scenes whose instances are all flattened and that have no
// cutout opacity, decided per pass by renderPass; TWK_SLIM_STREAMS=0 keeps the full form):
//   hit          the slot word is slot | instance << slimSlotBits (a miss: -1, both halves) — a world-space slot belongs to one
//                instance, and traversal holds it (triangles[3 * slot + 1].w) — and hitInstance is neither written nor read;
//   shadow ray   shadowPending.w, the seed only the cutout test draws from, is the launch index; shadowPixel is neither written nor
//                read: the result write of a visible shadow ray needs ONE record before it adds to pathRadiance.
// 8 bytes less per path and bounce. shadePath never sees the packed or the slim form: the kernels around it pack and unpack here.
//
// PRIMARY launches (depth 0 of a pass without generateKernel) COMPUTE the ray and path state of queue 0 (shade_device.h
// primaryRay) instead of reading it: the launch index is the slot itself. A scene with cutout opacity keeps one word of the
// queue, the seed (storePrimarySeed), and hands the tmin of an overflowed ray on through its hit record (storeOverflowTmin).
#pragma once
#include "device_types.h"

namespace twk {

// ---- the path word --------------------------------------------------------------------------------------------------------------
// Packed records: the path word (device_types.h TWK_PATH_*_SHIFT) <-> the five bits next to the launch index.
TWK_HD unsigned int packPathWord(unsigned int pixel, unsigned int word)
{
  return pixel | (((word >> 2) & 1u) << 27) | (((word >> 28) & 1u) << 28) | (((word >> TWK_PATH_STACK_SHIFT) & 7u) << 29);
}
TWK_HD unsigned int unpackPathWord(unsigned int packed)
{
  return (((packed >> 27) & 1u) << 2) | (((packed >> 28) & 1u) << 28) | ((packed >> 29) << TWK_PATH_STACK_SHIFT);
}
static_assert(TWK_FLAG_DIFFUSE == (1u << 2) && TWK_FLAG_ALBEDO == (1u << 28) && TWK_PACKED_PIXEL_BITS == 27, "packPathWord's bit positions");

// Slim records: the hit record's slot word <-> (triangle slot, instance). A miss is -1 on both sides.
TWK_HD int packSlotWord(int slotBits, int triangleSlot, int instance) { return triangleSlot | (int) ((unsigned int) instance << slotBits); }
TWK_HD int slotWordInstance(int slotBits, int word) { return word >> slotBits; } // arithmetic shift: -1 stays -1
TWK_HD int slotWordSlot(int slotBits, int word) { return (word < 0) ? word : (word & ((1 << slotBits) - 1)); }

// ---- the form of a launch's records ---------------------------------------------------------------------------------------------
// shadeKernel(depth): the queue it reads and the queue it writes.
TWK_HD bool packedInput(const LaunchParams& p, int depth) { return p.packedQueue != 0 && depth > 0; }
TWK_HD bool packedOutput(const LaunchParams& p) { return p.packedQueue != 0; }
// The trace launch of bounce `depth`: its closest-hit rays' .w words are not tmin / tmax; its results go out in the slim form
// (set for flattened scenes only). cutout, primary: the build's.
TWK_HD bool tracePacked(const LaunchParams& p, int depth, bool cutout, bool primary) { return !cutout && !primary && packedInput(p, depth); }
TWK_HD bool traceSlim(const LaunchParams& p, bool cutout) { return !cutout && p.slimSlotBits != 0; }

// ---- readers --------------------------------------------------------------------------------------------------------------------
// What traversal finds for one ray (trace_device.h traverse, traceKernel), and what a hit record and the firstHit capture hold of it.
struct TraceResult
{
  float t, beta, gamma;
  int   instance, primitive;
  int   triangleSlot; // slot of the hit triangle in the leaf-ordered arrays (what shading indexes)
};

// A ray as traversal takes it: o.w = tmin, d.w = tmax, whatever the record's form. word: origin.w as stored — a packed record's
// launch index | path bits (closestLaunchIndex reads it again where a kernel has not kept it).
struct QueuedRay { float4 o, d; unsigned int word; };

// The ONE decode of a packed record's two .w words: the launch index in the low bits of origin.w, and the tmin / tmax a
// continuation ray's record holds there otherwise, put back.
TWK_HD unsigned int packedLaunchIndex(unsigned int word) { return word & TWK_PACKED_PIXEL_MASK; }
TWK_D void restoreContinuationBounds(const LaunchParams& p, float4& o, float4& d) { o.w = p.sceneEpsilon; d.w = RT_DEFAULT_MAX; }

TWK_D QueuedRay loadClosestRay(const LaunchParams& p, int q, unsigned int record, bool packed)
{
  QueuedRay r;
  r.o = p.rayOrg[q][record]; r.d = p.rayDir[q][record];
  r.word = __float_as_uint(r.o.w);
  if (packed) restoreContinuationBounds(p, r.o, r.d);
  return r;
}
TWK_D QueuedRay loadShadowRay(const LaunchParams& p, unsigned int record)
{
  QueuedRay r;
  r.o = p.shadowOrg[record]; r.d = p.shadowDir[record]; r.word = 0u;
  return r;
}

// Launch index of the closest-hit ray at `record` of queue q. primary: queue 0 is the identity and was never written.
TWK_D unsigned int closestLaunchIndex(const LaunchParams& p, int q, unsigned int record, bool primary, bool packed)
{
  return primary ? record : (packed ? packedLaunchIndex(__float_as_uint(p.rayOrg[q][record].w)) : p.rayPixel[q][record]);
}
TWK_D unsigned int shadowLaunchIndex(const LaunchParams& p, unsigned int record, bool slim)
{
  return slim ? __float_as_uint(p.shadowPending[record].w) : p.shadowPixel[record];
}

// The path that travels with a closest-hit ray, as shadePath takes it: the ray with tmin / tmax restored, launch index, LCG state
// and path word, throughput and pdf. The host build of the kernels calls it; shadeKernel's loadShadeInput restates it as written
// (so does its shadow append storeShadowRay): through the calls its sorted builds came out in another register allocation and
// measured 1 % slower (profiles/r26_path_queue_records.md).
TWK_D void loadQueuedPath(const LaunchParams& p, int q, unsigned int record, bool packed, float4& ro, float4& rd, float4& throughputPdf, uint2& seedFlags, unsigned int& pixel)
{
  ro = p.rayOrg[q][record];
  rd = p.rayDir[q][record];
  throughputPdf = p.rayThroughput[q][record];
  if (packed)
  {
    const unsigned int word = __float_as_uint(ro.w);
    pixel = packedLaunchIndex(word);
    seedFlags = make_uint2(__float_as_uint(rd.w), unpackPathWord(word));
    restoreContinuationBounds(p, ro, rd);
  }
  else
  {
    pixel = p.rayPixel[q][record];
    seedFlags = p.raySeedFlags[q][record];
  }
}

// The hit of virtual slot `slot`. Slim: `instance` is left alone — the slot word holds both and is taken apart where the record is
// first used (unpackSlimHit): done here, the wave would wait for the record it has just requested.
TWK_D void loadHit(const LaunchParams& p, unsigned int slot, bool slim, float4& hit, int& instance)
{
  hit = p.hitRecord[slot];
  if (!slim) instance = p.hitInstance[slot];
}
TWK_D int slimHitInstance(int slotBits, const float4& hit) { return slotWordInstance(slotBits, __float_as_int(hit.w)); }
// Slim hit record -> the instance shadePath is given and the triangle slot it finds in the record.
TWK_D void unpackSlimHit(int slotBits, float4& hit, int& instanceIndex)
{
  const int word = __float_as_int(hit.w);
  int instance = slotWordInstance(slotBits, word), slot = slotWordSlot(slotBits, word);
#if defined(__HIP_DEVICE_COMPILE__)
  // Pinned: left alone, hipcc keeps the word alive next to the two and derives them again where they are used — one register
  // more through the whole of shadePath, and the five-wave builds, which sit exactly at their 96, spill 8 bytes.
  asm volatile("" : "+v"(instance), "+v"(slot));
#endif
  instanceIndex = instance;
  hit.w = __int_as_float(slot);
}

// ---- writers --------------------------------------------------------------------------------------------------------------------
// Record `index` of queue 0, as generateKernel writes it (always full). Inactive launch indices (tile columns beyond the image)
// still own a slot so that queue 0 is the identity mapping; they carry tmax < tmin and never hit anything, and shade drops them.
TWK_D void storePrimaryRecord(const LaunchParams& p, unsigned int index, const V3& origin, const V3& direction, bool active, unsigned int seed)
{
  p.rayThroughput[0][index] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
  p.raySeedFlags[0][index]  = make_uint2(seed, 0u);
  p.rayOrg[0][index]   = make_float4(origin.x, origin.y, origin.z, p.sceneEpsilon);
  p.rayDir[0][index]   = make_float4(direction.x, direction.y, direction.z, active ? RT_DEFAULT_MAX : -1.0f);
  p.rayPixel[0][index] = index;
}
// PRIMARY launches of a scene with cutout opacity: the first traversal stores the seed in queue 0, its opacity tests draw from it
// (drawFromRaySeed), and shade(0) takes it from there.
TWK_D void storePrimarySeed(const LaunchParams& p, unsigned int slot, unsigned int seed) { p.raySeedFlags[0][slot] = make_uint2(seed, 0u); }
TWK_D uint2 loadPrimarySeedFlags(const LaunchParams& p, unsigned int slot) { return p.raySeedFlags[0][slot]; }
// ... and where the re-trace of an overflowed ray continues (behind the candidates ignored so far) rides in its hit record, which
// the re-trace overwrites.
TWK_D void storeOverflowTmin(const LaunchParams& p, unsigned int slot, float tmin) { p.hitRecord[slot] = make_float4(tmin, 0.0f, 0.0f, 0.0f); }
TWK_D float loadOverflowTmin(const LaunchParams& p, unsigned int slot) { return p.hitRecord[slot].x; }

// The continuation ray of a path, record n of queue qn.
TWK_D void storeContinuation(const LaunchParams& p, int qn, unsigned int n, bool packed, const V3& pos, const V3& dir, unsigned int pixel, const uint2 seedFlags, const float4 throughputPdf)
{
  if (packed)
  {
    p.rayOrg[qn][n] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(packPathWord(pixel, seedFlags.y)));
    p.rayDir[qn][n] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(seedFlags.x));
  }
  else
  {
    p.rayOrg[qn][n]   = make_float4(pos.x, pos.y, pos.z, p.sceneEpsilon);
    p.rayDir[qn][n]   = make_float4(dir.x, dir.y, dir.z, RT_DEFAULT_MAX);
    p.rayPixel[qn][n] = pixel;
    p.raySeedFlags[qn][n]  = seedFlags;
  }
  p.rayThroughput[qn][n] = throughputPdf;
}
// The shadow ray of a path and the contribution that waits for it, record s of the shadow queue. Slim: no cutout test draws from
// the seed; the launch index rides there.
TWK_D void storeShadowRay(const LaunchParams& p, unsigned int s, bool slim, const V3& pos, const V3& dir, float tmax, const V3& pending, unsigned int pixel, unsigned int seed)
{
  p.shadowOrg[s]     = make_float4(pos.x, pos.y, pos.z, p.sceneEpsilon);
  p.shadowDir[s]     = make_float4(dir.x, dir.y, dir.z, tmax);
  if (!slim) p.shadowPixel[s] = pixel;
  p.shadowPending[s] = make_float4(pending.x, pending.y, pending.z, __uint_as_float(slim ? pixel : seed));
}

TWK_D void storeHit(const LaunchParams& p, unsigned int slot, bool slim, const TraceResult& res)
{
  if (slim) p.hitRecord[slot] = make_float4(res.t, res.beta, res.gamma, __int_as_float(packSlotWord(p.slimSlotBits, res.triangleSlot, res.instance)));
  else
  {
    p.hitRecord[slot]   = make_float4(res.t, res.beta, res.gamma, __int_as_float(res.triangleSlot));
    p.hitInstance[slot] = res.instance;
  }
}
// debug capture of the primary hits, by launch index
TWK_D void storeFirstHit(const LaunchParams& p, unsigned int pixel, const TraceResult& res)
{
  p.firstHit[pixel] = make_float4(res.t, res.beta, res.gamma, __int_as_float(res.primitive));
  p.firstHitInstance[pixel] = res.instance;
}
// A visible shadow ray: add the pending next-event contribution (closesthit.cu:288-299, raygeneration.cu:100)
TWK_D void addVisibleShadow(const LaunchParams& p, unsigned int record, bool slim)
{
  const float4 c = p.shadowPending[record];
  const unsigned int pixel = slim ? __float_as_uint(c.w) : p.shadowPixel[record]; // slim: the launch index rides in the pending record
  float4 r = p.pathRadiance[pixel];
  r.x += c.x; r.y += c.y; r.z += c.z;
  p.pathRadiance[pixel] = r;
}

// The cutout test of one candidate (trace_persistent.h cutoutIgnoresCandidate) draws from the seed IN the record — a radiance ray's
// from the path's, a shadow ray's from the stream forked when the ray was emitted — and writes the advanced seed back.
// draw(seed): advances the seed, returns the number.
template<typename Draw>
TWK_D float drawFromRaySeed(const LaunchParams& p, bool isShadow, int q, unsigned int record, Draw draw)
{
  float x;
  if (isShadow)
  {
    float4 pend = p.shadowPending[record];
    unsigned int seed = __float_as_uint(pend.w);
    x = draw(seed);
    pend.w = __uint_as_float(seed);
    p.shadowPending[record] = pend;
  }
  else
  {
    uint2 sf = p.raySeedFlags[q][record];
    x = draw(sf.x);
    p.raySeedFlags[q][record] = sf;
  }
  return x;
}
// ... and an ignored candidate's distance becomes the record's tmin, so that a re-trace by traceOverflowKernel continues behind
// the same candidate.
TWK_D void storeRayTmin(const LaunchParams& p, bool isShadow, int q, unsigned int record, float tmin)
{
  if (isShadow) p.shadowOrg[record].w = tmin; else p.rayOrg[q][record].w = tmin;
}

// ---- the result of one finished ray -----------------------------------------------------------------------------------------------
// What a trace kernel leaves behind for the ray of virtual slot `slot`: a closest-hit ray's hit record (and the debug capture of
// the primary hits), a visible shadow ray's contribution to its path's radiance; COUNT builds with the time view on add the
// ray's cycles to its path's time word. primary / packed / slim: the form of the launch (above) — three plain arguments: handed
// over as one struct, the PRIMARY builds of traceKernel came out with another register allocation through the whole node loop.
// record(): the ray's physical record in its queue — a callable, evaluated only on the branches that read the queue again.
template<bool COUNT, typename Record>
TWK_D void storeRayResult(const LaunchParams& p, int depth, bool primary, bool packed, bool slim, unsigned int slot, bool isShadow,
                          const TraceResult& res, unsigned int rayCycles, Record record)
{
  const int q = depth & 1;
  if (!isShadow)
  {
    storeHit(p, slot, slim, res);
    if (COUNT && p.pathTime != nullptr) atomicAdd(&p.pathTime[closestLaunchIndex(p, q, record(), primary, packed)], float(rayCycles));
    if (p.firstHit != nullptr && depth == 0) storeFirstHit(p, closestLaunchIndex(p, q, record(), primary, false), res); // queue 0 is never packed
  }
  else
  {
    if (COUNT && p.pathTime != nullptr) atomicAdd(&p.pathTime[shadowLaunchIndex(p, record(), slim)], float(rayCycles));
    if (res.instance < 0) addVisibleShadow(p, record(), slim);
  }
}

} // namespace twk
