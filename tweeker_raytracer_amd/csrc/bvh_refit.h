// The refit of one tree (twk_refit_geometry_vertices): new vertices, the topology kept. This header is the complete per-slot and
// per-node definition, shared by the kernels (bvh_refit.hip) and the host form (twk_refit_tree_host), and it holds what the build
// (bvh_build.hip) and the refit write with one text: padBox, the binary and the wide node, the triangle slot and its shading
// record. Built with -ffp-contract=off (csrc/Makefile): every operation rounds once, as written, so the host form has the device's bits.
//
// ---- what a refit keeps, and what it writes ---------------------------------------------------------------------------------------
// Kept: the child references of every binary node (so: which slots a leaf covers, which nodes a range leaves unused), the primitive
// word of every slot (and the instance word of a world-space slot), the pair flags, and the CUT of every wide node — which of a node's
// two children gives way to its own children, read from the references the wide node holds.
// Written: every slot and its shading record (emitTriangle, as the build emits them), every leaf's box, every inner box as the
// fminf / fmaxf union of its children's, every full-precision wide node with the cut it had, and nodeCost by refitKernel's formula for
// that cut. The refit of a tree whose INSTANCE moved (twk_refit_instance_transform, kind 2 of refit_scene_plan.h) writes the same, except that
// it leaves the shading records alone: moveTriangle instead of emitTriangle.
//
// ---- a leaf's box (refitLeafBox) ------------------------------------------------------------------------------------------------
// The build's rule: a leaf covers `count` consecutive slots; pairFlags groups them into build primitives (a pair is ONE primitive
// with the box of both triangles); each primitive's tight box, from the slots' own vertices in triangleBoxesKernel's order, is grown
// by padBox ONCE; the leaf's box is the union of its primitives' padded boxes. A refit with the vertices the tree was built from
// therefore changes no bit (tests/test_gpu_refit.py).
//
// ---- a node (refitNode), once both child boxes stand in its binary node ------------------------------------------------------------
//   the one node of a one-primitive tree keeps its never-hit second child (+inf box, reference ~0) and costs 1
//   else: child k was opened in the wide node iff the wide node's entry at its place is not the child's own reference; the entries are
//   rebuilt with expandChild / emptyEntry / writeWideNode; nodeCost = 1 + sum over the inner entries of min(area(e) / area(node), 1)
//   nodeCost(e), evaluated in refitKernel's order.
// An all-zero node (a tree over pairs has fewer nodes than its triangles reserve) reads as two references to node 0: it takes no part
// and stays all-zero. A node INSIDE a collapsed subtree is written by the build although its parent references the whole subtree as
// one leaf: nothing references it and both its children are leaves (every part of a collapsed range is collapsed too). It is refit
// like any other node, so that a refit back restores it, hands its box to nobody, and is no part of the SAH terms.
//
// ---- SAH terms (refitNodeTerms) ---------------------------------------------------------------------------------------------------
// BvhBuilder::lastSahInner / lastSahLeaf as sahCostKernel (bvh_sah.hip) adds them up: per node half-area(union of its child boxes) /
// half-area(root) in float; per leaf child the same quotient of its box — the UNPADDED box of a leaf of one build primitive, the
// (padded) node box of a collapsed subtree — times its triangles. Summed in double.
//
// What it is not: no new topology, no restructuring, no new cuts (the costs follow the boxes, the cuts stay), and a refit of a tree
// whose references leave its ranges is refused by the host form and never launched by the device form (the build made them).
#pragma once
#include "device_types.h"

#include <cmath>
#include <vector>

namespace twk {

// Soup descriptor of one flattened triangle: x = instance, y = first vertex of its geometry in the shared attribute
// array, z = first index of the TRIANGLE in the shared index array, w = primitive index inside the geometry.
// Vertex c of a soup triangle, in world space: the geometry's object-space position through the instance's
// object-to-world matrix — m0*x + m1*y + m2*z + m3 in fp32, the expression transformPoint (closesthit.cu:88-98) and
// the oracle evaluate.
TWK_HD void soupVertices(const int4& d, const float* __restrict__ attributes, const unsigned int* __restrict__ indices,
                         const DevInstance* __restrict__ instances, const float*& a, const float*& b, const float*& c, V3& wa, V3& wb, V3& wc)
{
  const unsigned int i0 = indices[d.z], i1 = indices[d.z + 1], i2 = indices[d.z + 2];
  a = attributes + 12 * ((size_t) d.y + i0);
  b = attributes + 12 * ((size_t) d.y + i1);
  c = attributes + 12 * ((size_t) d.y + i2);
  const float* m = instances[d.x].objectToWorld;
  wa = transformPoint(m, v3(a[0], a[1], a[2]));
  wb = transformPoint(m, v3(b[0], b[1], b[2]));
  wc = transformPoint(m, v3(c[0], c[1], c[2]));
}

TWK_HD void padBox(float4& lo, float4& hi)
{
  // The watertight triangle test reports t with an ABSOLUTE error that scales with the triangle's size and with the
  // magnitude of its coordinates (the edge functions are differences of products of vertex-minus-origin terms), not
  // with t: a ray that starts 2e-4 above a 16-unit floor triangle gets a t that is off by 3e-7, 1e-3 of its value —
  // measured: with axis-tight boxes (a flat floor: pad 1e-30 in y) the slab interval [3.52942e-4, 3.52942e-4] was
  // culled against a current best of 3.52938e-4 although the triangle test would have returned 3.5266e-4. Every
  // primitive box therefore grows on ALL axes by 2^-17 (128 ulp) of (largest coordinate magnitude + box diagonal):
  // two orders of magnitude above the observed error, 0.03 % of a 0.03-unit triangle. Errors that scale with the
  // distance travelled are covered by the relative widening of the slab test itself (trace_device.h).
  const float k = 7.6293945e-6f; // 2^-17
  const float m = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(hi.x)), fmaxf(fabsf(lo.y), fabsf(hi.y))), fmaxf(fabsf(lo.z), fabsf(hi.z)));
  const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
  const float e = k * (m + sqrtf(dx * dx + dy * dy + dz * dz)) + 1.0e-30f;
  lo.x -= e; lo.y -= e; lo.z -= e;
  hi.x += e; hi.y += e; hi.z += e;
}

TWK_HD void writeNode(BvhNode* node, const float4& lo0, const float4& hi0, const float4& lo1, const float4& hi1, int c0, int c1)
{
  float4* p = reinterpret_cast<float4*>(node);
  p[0] = make_float4(lo0.x, lo0.y, lo0.z, hi0.x);
  p[1] = make_float4(hi0.y, hi0.z, lo1.x, lo1.y);
  p[2] = make_float4(lo1.z, hi1.x, hi1.y, hi1.z);
  p[3] = make_float4(asFloat((uint32_t) c0), asFloat((uint32_t) c1), 0.0f, 0.0f);
}

// Wide (4-ary) node of inner node i = the children of its children, 128 bytes (layout at writeWideNode): a traversal step over a wide node crosses two levels of the binary tree
// with one round of loads instead of two dependent ones. A child that is a leaf occupies one entry; unused entries
// get an empty box. Wide nodes share the index space of the binary nodes (every inner node has one; only those at
// even depth below the root are ever visited).
struct WideEntry { float4 lo, hi; int ref; };
// (Round 3, measured and not kept: opening twice the inner entry with the largest surface area instead of taking the four
// grandchildren — node visits per ray 7.64 -> 7.43 on C2, triangle tests 3.07 -> 3.28, C2 -7 %: profiles/r03y_wide_collapse_greedy.txt.)
TWK_HD float wideHalfArea(const float4& lo, const float4& hi)
{
  const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
  return dx * dy + dy * dz + dz * dx;
}

TWK_HD void emptyEntry(WideEntry& e)
{
  const float inf = asFloat(0x7f800000u);
  // lo = hi = +inf: every plane distance is +inf or -inf on both sides, so the slab interval is empty for any ray.
  // (An inverted box lo > hi does NOT work: the slab test orders the two plane distances itself.)
  e.lo = make_float4(inf, inf, inf, 0.0f); e.hi = make_float4(inf, inf, inf, 0.0f); e.ref = ~0;
}

// Expands child `ref` (box lo/hi) into one entry (leaf) or the two entries of its own children (inner node).
TWK_HD void expandChild(const BvhNode* outNodes, int nodeBase, int ref, const float4& lo, const float4& hi, WideEntry* e, int& n)
{
  if (ref < 0) { e[n].lo = lo; e[n].hi = hi; e[n].ref = ref; ++n; return; }
  const float4* c = reinterpret_cast<const float4*>(outNodes + (ref - nodeBase));
  const float4 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
  e[n].lo = make_float4(c0.x, c0.y, c0.z, 0.0f); e[n].hi = make_float4(c0.w, c1.x, c1.y, 0.0f); e[n].ref = (int) asUint(c3.x); ++n;
  e[n].lo = make_float4(c1.z, c1.w, c2.x, 0.0f); e[n].hi = make_float4(c2.y, c2.z, c2.w, 0.0f); e[n].ref = (int) asUint(c3.y); ++n;
}

// Wide node layout, 8 float4: (lo_k.xyz, ref_k) and (hi_k.xyz, unused) for k = 0..3, with the four references in
// the .w of the FIRST four float4 — (lo0,ref0) (hi0,ref1) (lo1,ref2) (hi1,ref3) (lo2,-) (hi2,-) (lo3,-) (hi3,-) —
// so that they arrive with the box data the first slab tests need. (With the references in a float4 of their own
// the compiler sank those loads behind the box tests: two extra dependent L2 round trips per traversal step.)
TWK_HD void writeWideNode(BvhNode* wide, const WideEntry* e)
{
  float4* p = reinterpret_cast<float4*>(wide);
  p[0] = make_float4(e[0].lo.x, e[0].lo.y, e[0].lo.z, asFloat((uint32_t) e[0].ref));
  p[1] = make_float4(e[0].hi.x, e[0].hi.y, e[0].hi.z, asFloat((uint32_t) e[1].ref));
  p[2] = make_float4(e[1].lo.x, e[1].lo.y, e[1].lo.z, asFloat((uint32_t) e[2].ref));
  p[3] = make_float4(e[1].hi.x, e[1].hi.y, e[1].hi.z, asFloat((uint32_t) e[3].ref));
  p[4] = make_float4(e[2].lo.x, e[2].lo.y, e[2].lo.z, 0.0f);
  p[5] = make_float4(e[2].hi.x, e[2].hi.y, e[2].hi.z, 0.0f);
  p[6] = make_float4(e[3].lo.x, e[3].lo.y, e[3].lo.z, 0.0f);
  p[7] = make_float4(e[3].hi.x, e[3].hi.y, e[3].hi.z, 0.0f);
}

// Triangle slots in leaf order: three float4 per slot, w of the first = primitive index. The same pass writes the
// 128-byte shading record of the slot (one cache line, eight float4), ordered by who needs what, so that shading does
// not chase indices → three 48-byte vertex records and fetches only the part its material uses — every fetch here is
// one divergent lane address, and a CU takes one of those per clock (tools/gather_probe.hip):
//   [0..2]  geometric normal cross(v1 - v0, v2 - v0) as closesthit.cu:150 computes it (same float operations, done
//           once here), then the three vertex normals                                   — every hit
//   [3..5.x] the three vertex tangents                                                  — GGX materials (TBN) only
//   [5.y..7.y] the three vertex texture coordinates                                     — textured materials only
TWK_HD void emitTriangle(const float* __restrict__ attributes, const unsigned int* __restrict__ indices,
                         const int4* __restrict__ soup, const DevInstance* __restrict__ instances,
                         unsigned int prim, int slot, float4* __restrict__ triangles, float4* __restrict__ shadeTriangles)
{
  const float *a, *b, *c;
  if (soup != nullptr)
  {
    // world-space positions for traversal, tagged with primitive and instance; the shading record below stays in
    // object space (shading transforms normals / tangents with the instance matrices as for any other hit)
    const int4 d = soup[prim];
    V3 wa, wb, wc;
    soupVertices(d, attributes, indices, instances, a, b, c, wa, wb, wc);
    triangles[3 * (size_t) slot + 0] = make_float4(wa.x, wa.y, wa.z, asFloat((uint32_t) d.w));
    triangles[3 * (size_t) slot + 1] = make_float4(wb.x, wb.y, wb.z, asFloat((uint32_t) d.x));
    triangles[3 * (size_t) slot + 2] = make_float4(wc.x, wc.y, wc.z, 0.0f);
  }
  else
  {
    const unsigned int i0 = indices[3 * prim], i1 = indices[3 * prim + 1], i2 = indices[3 * prim + 2];
    a = attributes + 12 * (size_t) i0;
    b = attributes + 12 * (size_t) i1;
    c = attributes + 12 * (size_t) i2;
    triangles[3 * (size_t) slot + 0] = make_float4(a[0], a[1], a[2], asFloat(prim));
    triangles[3 * (size_t) slot + 1] = make_float4(b[0], b[1], b[2], 0.0f);
    triangles[3 * (size_t) slot + 2] = make_float4(c[0], c[1], c[2], 0.0f);
  }
  const V3 v0 = v3(a[0], a[1], a[2]), v1 = v3(b[0], b[1], b[2]), v2 = v3(c[0], c[1], c[2]);
  const V3 ng = cross(v1 - v0, v2 - v0);
  float4* out = shadeTriangles + TWK_SHADE_RECORD * (size_t) slot;
  out[0] = make_float4(ng.x, ng.y, ng.z, a[6]);
  out[1] = make_float4(a[7], a[8], b[6], b[7]);
  out[2] = make_float4(b[8], c[6], c[7], c[8]);
  out[3] = make_float4(a[3], a[4], a[5], b[3]);
  out[4] = make_float4(b[4], b[5], c[3], c[4]);
  out[5] = make_float4(c[5], a[9], a[10], a[11]);
  out[6] = make_float4(b[9], b[10], b[11], c[9]);
  out[7] = make_float4(c[10], c[11], 0.0f, 0.0f);
}

// The slot of a world-space tree whose INSTANCE moved (twk_refit_instance_transform, kind 2 of refit_scene_plan.h): emitTriangle's three
// world-space float4 through the matrix the instance record holds now, and nothing else. The shading record is built from the
// object-space a, b, c alone (above: the geometric normal of the untransformed triangle, the vertices' normals, tangents and texture
// coordinates as the geometry holds them) — a transform changes none of its 128 bytes, so it is neither read nor written.
TWK_HD void moveTriangle(const float* __restrict__ attributes, const unsigned int* __restrict__ indices, const int4* __restrict__ soup,
                         const DevInstance* __restrict__ instances, unsigned int prim, int slot, float4* __restrict__ triangles)
{
  const float *a, *b, *c;
  const int4 d = soup[prim];
  V3 wa, wb, wc;
  soupVertices(d, attributes, indices, instances, a, b, c, wa, wb, wc);
  triangles[3 * (size_t) slot + 0] = make_float4(wa.x, wa.y, wa.z, asFloat((uint32_t) d.w));
  triangles[3 * (size_t) slot + 1] = make_float4(wb.x, wb.y, wb.z, asFloat((uint32_t) d.x));
  triangles[3 * (size_t) slot + 2] = make_float4(wc.x, wc.y, wc.z, 0.0f);
}

// ---- the refit -------------------------------------------------------------------------------------------------------------------

// One tree as a refit sees it. Every array is the TREE's: node nodeBase + i stands at nodes[i] (its wide node at wide[2 * i], its
// cost at nodeCost[i]), slot slotBase + s at triangles[3 * s] and pairFlags[s]; the references in the nodes are absolute.
// nodeCost nullptr: the cuts were not costed (every wide node holds the four grandchildren); pairFlags nullptr: no pairs.
struct RefitTree
{
  BvhNode* nodes; BvhNode* wide; float* nodeCost;
  const float4* triangles; const int* pairFlags;
  int nodeBase, numNodes, slotBase, numSlots;
};
// One tree of a batched refit (bvh_refit.hip), as the device table holds it: the tree, and how many nodes (nodeOffset: where its
// parents and tickets stand) and slots (slotOffset) the trees before it have (refit_batch_plan.h). 64 bytes.
struct RefitBatchTree { RefitTree tree; int nodeOffset, slotOffset; };

TWK_HD void refitChildren(const BvhNode* node, int& c0, int& c1)
{
  const float4 w = reinterpret_cast<const float4*>(node)[3];
  c0 = (int) asUint(w.x); c1 = (int) asUint(w.y);
}
// A node the leaf collapse left unused is all-zero
TWK_HD bool refitUnused(int c0, int c1) { return c0 == 0 && c1 == 0; }
// The second child of the one node of a one-primitive tree (singleLeafKernel): never hit, never refit
TWK_HD bool refitNeverHit(const BvhNode* node)
{
  const float4* p = reinterpret_cast<const float4*>(node);
  const float inf = asFloat(0x7f800000u);
  return (int) asUint(p[3].y) == ~0 && p[1].z == inf && p[2].y == inf;
}
// The slots of leaf `ref`, tree-local; false when they leave the tree's slot range
TWK_HD bool refitLeafSlots(const RefitTree& t, int ref, int& first, int& count)
{
  const int payload = ~ref;
  first = (payload & 0x0fffffff) - t.slotBase; count = ((payload >> 28) & 3) + 1;
  return first >= 0 && first <= t.numSlots - count;
}

// The box of leaf `ref` (above: "a leaf's box"). tightLo / tightHi: the unpadded box of its last build primitive — of its only
// one when `single`.
TWK_HD void refitLeafBox(const RefitTree& t, int ref, float4& lo, float4& hi, float4& tightLo, float4& tightHi, int& triangles, bool& single)
{
  const float inf = asFloat(0x7f800000u);
  int first, count;
  lo = make_float4(inf, inf, inf, 0.0f); hi = make_float4(-inf, -inf, -inf, 0.0f);
  tightLo = lo; tightHi = hi; triangles = 0; single = false;
  if (!refitLeafSlots(t, ref, first, count)) return;
  int primitives = 0;
  for (int s = 0; s < count; ++primitives)
  {
    const int n = (t.pairFlags != nullptr && s + 1 < count && t.pairFlags[first + s] != 0) ? 2 : 1;
    float4 plo = make_float4(inf, inf, inf, 0.0f), phi = make_float4(-inf, -inf, -inf, 0.0f);
    for (int k = 0; k < n; ++k)
    {
      const float4* v = t.triangles + 3 * (size_t) (first + s + k);
      const float4 va = v[0], vb = v[1], vc = v[2];
      plo.x = fminf(plo.x, fminf(fminf(va.x, vb.x), vc.x)); plo.y = fminf(plo.y, fminf(fminf(va.y, vb.y), vc.y)); plo.z = fminf(plo.z, fminf(fminf(va.z, vb.z), vc.z));
      phi.x = fmaxf(phi.x, fmaxf(fmaxf(va.x, vb.x), vc.x)); phi.y = fmaxf(phi.y, fmaxf(fmaxf(va.y, vb.y), vc.y)); phi.z = fmaxf(phi.z, fmaxf(fmaxf(va.z, vb.z), vc.z));
    }
    tightLo = plo; tightHi = phi;
    padBox(plo, phi);
    lo = make_float4(fminf(lo.x, plo.x), fminf(lo.y, plo.y), fminf(lo.z, plo.z), 0.0f);
    hi = make_float4(fmaxf(hi.x, phi.x), fmaxf(hi.y, phi.y), fmaxf(hi.z, phi.z), 0.0f);
    s += n;
  }
  triangles = count; single = (primitives == 1);
}

// The two child boxes and references of node i as its binary node holds them
TWK_HD void refitChildBoxes(const BvhNode* node, float4& lo0, float4& hi0, float4& lo1, float4& hi1, int& c0, int& c1)
{
  const float4* p = reinterpret_cast<const float4*>(node);
  const float4 p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
  lo0 = make_float4(p0.x, p0.y, p0.z, 0.0f); hi0 = make_float4(p0.w, p1.x, p1.y, 0.0f);
  lo1 = make_float4(p1.z, p1.w, p2.x, 0.0f); hi1 = make_float4(p2.y, p2.z, p2.w, 0.0f);
  c0 = (int) asUint(p3.x); c1 = (int) asUint(p3.y);
}
// Child `side` of a node gets a new box; nothing else of the node is touched (another thread may be writing the other child's)
TWK_HD void refitStoreChildBox(BvhNode* node, int side, const float4& lo, const float4& hi)
{
  float* w = reinterpret_cast<float*>(node) + 6 * side;
  w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = hi.x; w[4] = hi.y; w[5] = hi.z;
}

// Node i (tree-local), whose binary node holds both child boxes and whose inner children are complete (above: "a node"). lo / hi:
// its own box, for its parent.
TWK_HD void refitNode(const RefitTree& t, int i, float4& lo, float4& hi)
{
  BvhNode* node = t.nodes + i;
  float4 lo0, hi0, lo1, hi1;
  int c0, c1;
  refitChildBoxes(node, lo0, hi0, lo1, hi1, c0, c1);
  WideEntry e[4];
  int n = 0;
  if (refitNeverHit(node))
  {
    writeNode(node, lo0, hi0, lo1, hi1, c0, c1);
    e[n].lo = lo0; e[n].hi = hi0; e[n].ref = c0; ++n;
    for (; n < 4; ++n) emptyEntry(e[n]);
    writeWideNode(t.wide + 2 * (size_t) i, e);
    if (t.nodeCost != nullptr) t.nodeCost[i] = 1.0f;
    lo = lo0; hi = hi0;
    return;
  }
  writeNode(node, lo0, hi0, lo1, hi1, c0, c1);
  // the cut the wide node had: child 0 stands at entry 0 or its two children at entries 0 and 1; child 1 follows
  const float4* w = reinterpret_cast<const float4*>(t.wide + 2 * (size_t) i);
  const int had[4] = { (int) asUint(w[0].w), (int) asUint(w[1].w), (int) asUint(w[2].w), (int) asUint(w[3].w) };
  const bool open0 = (c0 >= 0) && (had[0] != c0);
  const bool open1 = (c1 >= 0) && (had[open0 ? 2 : 1] != c1);
  lo = make_float4(fminf(lo0.x, lo1.x), fminf(lo0.y, lo1.y), fminf(lo0.z, lo1.z), 0.0f);
  hi = make_float4(fmaxf(hi0.x, hi1.x), fmaxf(hi0.y, hi1.y), fmaxf(hi0.z, hi1.z), 0.0f);
  const float areaNode = wideHalfArea(lo, hi);
  const float scale = (areaNode > 0.0f) ? 1.0f / areaNode : 0.0f;
  // what each child puts into the wide node — itself, or its two children — and the expected visits below it under that cut
  // (refitKernel's keep[k] / open[k]); every index is a constant, so that the entries stay in registers
  const bool open[2] = { open0, open1 };
  WideEntry child[2], grand[2][2], none;
  child[0].lo = lo0; child[0].hi = hi0; child[0].ref = c0;
  child[1].lo = lo1; child[1].hi = hi1; child[1].ref = c1;
  emptyEntry(none);
  float below[2] = { 0.0f, 0.0f };
  for (int k = 0; k < 2; ++k)
  {
    grand[k][0] = child[k]; grand[k][1] = none;
    if (open[k]) { int m = 0; expandChild(t.nodes, t.nodeBase, child[k].ref, child[k].lo, child[k].hi, grand[k], m); }
    if (t.nodeCost == nullptr) continue;
    for (int g = 0; g < 2; ++g)
      if (grand[k][g].ref >= 0) below[k] += fminf(wideHalfArea(grand[k][g].lo, grand[k][g].hi) * scale, 1.0f) * t.nodeCost[grand[k][g].ref - t.nodeBase];
  }
  e[0] = grand[0][0];
  e[1] = open0 ? grand[0][1] : grand[1][0];
  e[2] = open0 ? grand[1][0] : grand[1][1];
  e[3] = open0 ? grand[1][1] : none;
  writeWideNode(t.wide + 2 * (size_t) i, e);
  if (t.nodeCost != nullptr) t.nodeCost[i] = 1.0f + below[0] + below[1];
}

// The box of the whole tree from its root node (BvhBuilder::buildTriangles' rootBounds)
TWK_HD void refitRootBox(const BvhNode* root, float4& lo, float4& hi)
{
  float4 lo0, hi0, lo1, hi1;
  int c0, c1;
  refitChildBoxes(root, lo0, hi0, lo1, hi1, c0, c1);
  if (refitNeverHit(root)) { lo = lo0; hi = hi0; return; }
  lo = make_float4(fminf(lo0.x, lo1.x), fminf(lo0.y, lo1.y), fminf(lo0.z, lo1.z), 0.0f);
  hi = make_float4(fmaxf(hi0.x, hi1.x), fmaxf(hi0.y, hi1.y), fmaxf(hi0.z, hi1.z), 0.0f);
}

// What node i (tree-local) adds to the tree's SAH terms (above: "SAH terms"); an unused node and a one-primitive tree add nothing
TWK_HD void refitNodeTerms(const RefitTree& t, int i, double& inner, double& leaf)
{
  inner = 0.0; leaf = 0.0;
  float4 rlo, rhi, lo0, hi0, lo1, hi1;
  int c0, c1;
  if (refitNeverHit(t.nodes)) return;
  refitRootBox(t.nodes, rlo, rhi);
  const float rootArea = wideHalfArea(rlo, rhi);
  if (!(rootArea > 0.0f)) return;
  refitChildBoxes(t.nodes + i, lo0, hi0, lo1, hi1, c0, c1);
  if (refitUnused(c0, c1)) return;
  const float4 lo = make_float4(fminf(lo0.x, lo1.x), fminf(lo0.y, lo1.y), fminf(lo0.z, lo1.z), 0.0f);
  const float4 hi = make_float4(fmaxf(hi0.x, hi1.x), fmaxf(hi0.y, hi1.y), fmaxf(hi0.z, hi1.z), 0.0f);
  inner = (double) (wideHalfArea(lo, hi) / rootArea);
  const float4 clo[2] = { lo0, lo1 }, chi[2] = { hi0, hi1 };
  const int cref[2] = { c0, c1 };
  for (int k = 0; k < 2; ++k)
  {
    if (cref[k] >= 0) continue;
    float4 blo, bhi, tlo, thi;
    int triangles; bool single;
    refitLeafBox(t, cref[k], blo, bhi, tlo, thi, triangles, single);
    leaf += (double) ((single ? wideHalfArea(tlo, thi) : wideHalfArea(clo[k], chi[k])) / rootArea) * triangles;
  }
}

// ---- the host form (twk_refit_tree_host after its refusals; tests/refit_host.cpp) ---------------------------------------------------
// Why a tree cannot be refit, or nullptr: no node is referenced twice, every inner reference stays in the node range and names a used
// node, every leaf in the slot range, a node nothing references is all-zero or holds two leaves, every primitive word names a
// triangle of the indices. parents: per node its parent, -1 for the root and for what the root does not reach.
inline const char* refitTreeRefusal(const RefitTree& t, size_t numTriangles, std::vector<int>& parents)
{
  parents.assign((size_t) t.numNodes, -1);
  std::vector<char> reached((size_t) t.numNodes, 0);
  std::vector<int> stack(1, 0);
  reached[0] = 1;
  int c0, c1;
  refitChildren(t.nodes, c0, c1);
  if (refitUnused(c0, c1)) return "the root node is unused";
  while (!stack.empty())
  {
    const int i = stack.back();
    stack.pop_back();
    int c[2], first, count;
    refitChildren(t.nodes + i, c[0], c[1]);
    for (int k = 0; k < 2; ++k)
    {
      if (c[k] < 0)
      {
        if (k == 1 && refitNeverHit(t.nodes + i)) continue;
        if (!refitLeafSlots(t, c[k], first, count)) return "a leaf reference leaves the slot range";
        continue;
      }
      const long long local = (long long) c[k] - t.nodeBase;
      if (local < 0 || local >= t.numNodes) return "an inner reference leaves the node range";
      if (reached[(size_t) local]) return "a node is referenced twice";
      int g0, g1;
      refitChildren(t.nodes + local, g0, g1);
      if (refitUnused(g0, g1)) return "an inner reference names an unused node";
      reached[(size_t) local] = 1; parents[(size_t) local] = i;
      stack.push_back((int) local);
    }
  }
  // what the walk did not reach: all-zero, or a node inside a collapsed subtree (two leaves)
  for (int i = 0; i < t.numNodes; ++i)
  {
    if (reached[(size_t) i]) continue;
    int c[2], first, count;
    refitChildren(t.nodes + i, c[0], c[1]);
    if (refitUnused(c[0], c[1])) continue;
    for (int k = 0; k < 2; ++k)
    {
      if (c[k] >= 0) return "a node that nothing references holds an inner reference";
      if (!refitLeafSlots(t, c[k], first, count)) return "a leaf reference leaves the slot range";
    }
  }
  for (int s = 0; s < t.numSlots; ++s)
    if ((size_t) asUint(t.triangles[3 * (size_t) s].w) >= numTriangles) return "a slot's primitive word is beyond the indices";
  return nullptr;
}

// What emitTriangle reads for the world-space tree of instance idInstance under `transform`, as buildFlattenedTree makes it: one soup
// descriptor per triangle of the geometry (whose attributes and indices are given as they are: both bases 0) and the instance's record
inline void refitSoupHost(int numTriangles, int idInstance, const float transform[12], std::vector<int4>& soup, std::vector<DevInstance>& instances)
{
  soup.resize((size_t) numTriangles);
  for (int k = 0; k < numTriangles; ++k) soup[(size_t) k] = make_int4(idInstance, 0, 3 * k, k);
  instances.assign((size_t) idInstance + 1, DevInstance());
  for (int k = 0; k < 12; ++k) instances[(size_t) idInstance].objectToWorld[k] = transform[k];
}

// The refit of a tree that refitTreeRefusal has passed (parents: its). triangles is t.triangles, writable; soup / instances as for
// emitTriangle, nullptr for an object-space tree. terms: the SAH terms (inner, leaf); rootBounds: the tree's box.
inline void refitTreeHost(const RefitTree& t, const std::vector<int>& parents, const float* attributes, const unsigned int* indices, const int4* soup,
                          const DevInstance* instances, float4* triangles, float4* shadeTriangles, double terms[2], float rootBounds[6])
{
  for (int s = 0; s < t.numSlots; ++s) emitTriangle(attributes, indices, soup, instances, asUint(triangles[3 * (size_t) s].w), s, triangles, shadeTriangles);
  // children before parents: the nodes in the order a walk from the root reaches them, backwards
  std::vector<int> order(1, 0);
  for (size_t at = 0; at < order.size(); ++at)
  {
    int c[2];
    refitChildren(t.nodes + order[at], c[0], c[1]);
    for (int k = 0; k < 2; ++k) if (c[k] >= 0) order.push_back(c[k] - t.nodeBase);
  }
  for (size_t at = order.size(); at-- > 0; )
  {
    const int i = order[at];
    int c0, c1, triangleCount; bool single;
    float4 lo, hi, tlo, thi;
    refitChildren(t.nodes + i, c0, c1);
    if (c0 < 0) { refitLeafBox(t, c0, lo, hi, tlo, thi, triangleCount, single); refitStoreChildBox(t.nodes + i, 0, lo, hi); }
    if (c1 < 0 && !refitNeverHit(t.nodes + i)) { refitLeafBox(t, c1, lo, hi, tlo, thi, triangleCount, single); refitStoreChildBox(t.nodes + i, 1, lo, hi); }
    refitNode(t, i, lo, hi);
    if (i == 0) continue;
    int p0, p1;
    refitChildren(t.nodes + parents[(size_t) i], p0, p1);
    refitStoreChildBox(t.nodes + parents[(size_t) i], (p0 == t.nodeBase + i) ? 0 : 1, lo, hi);
  }
  // the nodes inside collapsed subtrees: two leaves each, nobody's children
  for (int i = 1; i < t.numNodes; ++i)
  {
    int c0, c1, triangleCount; bool single;
    float4 lo, hi, tlo, thi;
    refitChildren(t.nodes + i, c0, c1);
    if (parents[(size_t) i] >= 0 || refitUnused(c0, c1)) continue;
    refitLeafBox(t, c0, lo, hi, tlo, thi, triangleCount, single); refitStoreChildBox(t.nodes + i, 0, lo, hi);
    refitLeafBox(t, c1, lo, hi, tlo, thi, triangleCount, single); refitStoreChildBox(t.nodes + i, 1, lo, hi);
    refitNode(t, i, lo, hi);
  }
  terms[0] = 0.0; terms[1] = 0.0;
  for (int i = 0; i < t.numNodes; ++i)
  {
    double inner, leaf;
    if (i > 0 && parents[(size_t) i] < 0) continue;
    refitNodeTerms(t, i, inner, leaf);
    terms[0] += inner; terms[1] += leaf;
  }
  float4 lo, hi;
  refitRootBox(t.nodes, lo, hi);
  rootBounds[0] = lo.x; rootBounds[1] = lo.y; rootBounds[2] = lo.z; rootBounds[3] = hi.x; rootBounds[4] = hi.y; rootBounds[5] = hi.z;
}

} // namespace twk
