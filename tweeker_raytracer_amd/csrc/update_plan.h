// Where everything of a scene stands, and what an update of some instances' transforms has to touch: the one place that decides
// which instances are flattened, which node and slot ranges the trees take, which trees a selective update rebuilds and which node
// ranges its ranged tail (bvh_build.hip rangedTailKernel) covers. Plain C++, no HIP: buildScene (device_scene.hip) lays its scene
// out with sceneLayout, the selective update plans with updatePlan, and twk_update_plan_host hands both out without a device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace twk {

// Binary nodes a tree over n triangles (or instances) reserves: n - 1, and one for a single primitive (singleLeafKernel)
inline int treeNodes(int primitives) { return (primitives > 1) ? primitives - 1 : 1; }

// The layout of a scene's node and slot arrays, in build order: one bottom-level tree per geometry that some instance still enters,
// one world-space tree per flattened instance, the top level. A transform moves none of it: whether an instance is flattened depends
// on triangle counts and reference counts only (include/tweeker_hip.h twk_set_flatten_policy).
struct SceneLayout
{
  std::vector<char> flattened;                              // per instance
  std::vector<char> directLeaf;                             // per instance: flattened and a leaf of the top level itself
  std::vector<char> needsBlas;                              // per geometry: some instance enters it
  std::vector<int>  geometryNodeBase, geometryTriangleBase; // per geometry (meaningful where needsBlas)
  std::vector<int>  flatNodeBase, flatTriangleBase;         // per instance, -1 for an entered one
  int    numEntered = 0, maxFlatTriangles = 0, tlasBase = 0;
  size_t numNodes = 0, numTriangles = 0;                    // binary nodes (the top level's included) and triangle slots
  bool   single = false;                                    // one flattened instance and nothing else: its tree IS the scene, no top level is built
};

// maxLeaf: triangles a leaf holds (BvhBuilder::maxLeaf); directSmallLeaves: a flattened instance of no more triangles than that
// (and than 4) is referenced by the top level as a leaf. Its one-node tree is built all the same.
inline void sceneLayout(const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries,
                        int flattenMaxTriangles, int flattenMaxReferences, int maxLeaf, bool directSmallLeaves, SceneLayout& s)
{
  s = SceneLayout();
  std::vector<int> references((size_t) numGeometries, 0);
  for (int i = 0; i < numInstances; ++i) references[(size_t) instanceGeometry[i]]++;
  s.flattened.assign((size_t) numInstances, 0); s.directLeaf.assign((size_t) numInstances, 0); s.needsBlas.assign((size_t) numGeometries, 0);
  for (int i = 0; i < numInstances; ++i)
  {
    const int g = instanceGeometry[i], n = geometryTriangles[g];
    s.flattened[i] = (n <= flattenMaxTriangles) || (references[g] <= flattenMaxReferences);
    if (s.flattened[i]) { s.maxFlatTriangles = std::max(s.maxFlatTriangles, n); s.directLeaf[i] = directSmallLeaves && n <= maxLeaf && n <= 4; }
    else { s.needsBlas[g] = 1; ++s.numEntered; }
  }
  s.geometryNodeBase.assign((size_t) numGeometries, 0); s.geometryTriangleBase.assign((size_t) numGeometries, 0);
  for (int k = 0; k < numGeometries; ++k)
  {
    s.geometryTriangleBase[k] = (int) s.numTriangles; s.geometryNodeBase[k] = (int) s.numNodes;
    if (s.needsBlas[k]) { s.numTriangles += (size_t) geometryTriangles[k]; s.numNodes += (size_t) treeNodes(geometryTriangles[k]); }
  }
  s.flatNodeBase.assign((size_t) numInstances, -1); s.flatTriangleBase.assign((size_t) numInstances, -1);
  for (int i = 0; i < numInstances; ++i)
  {
    if (!s.flattened[i]) continue;
    const int n = geometryTriangles[instanceGeometry[i]];
    s.flatTriangleBase[i] = (int) s.numTriangles; s.flatNodeBase[i] = (int) s.numNodes;
    s.numTriangles += (size_t) n; s.numNodes += (size_t) treeNodes(n);
  }
  s.tlasBase = (int) s.numNodes;
  s.numNodes += (size_t) treeNodes(numInstances);
  s.single = (numInstances == 1 && s.flattened[0]);
}

// A run of wide nodes the ranged tail quantises: `count` nodes from `first`
struct NodeRange { int first, count; };

// What a selective update of the instances `moved` (distinct, in range) touches. No bottom-level tree is in it: an entered instance
// changes its world box and nothing else. ranges: every rebuilt tree's node range in ascending order, then the top level's (it is
// rebuilt whenever there is one), then the two root slots behind the last node (bvh_build.hip wideRootKernel) — disjoint and
// ascending, because a flattened instance's range grows with its index and the top level follows them all.
// A vertex update (updatePlanWith: `updated` geometries, distinct, in range) adds what new vertices change: the bottom-level tree of
// an updated geometry that some instance enters, the world box of every entered instance of it, and the world-space tree of every
// flattened instance of it. A bottom-level range lies before every flattened one (sceneLayout), so the ranges stay ascending.
struct UpdatePlan
{
  std::vector<int>       geometries; // the entered geometries among `updated`, ascending: their bottom-level trees are rebuilt
  std::vector<int>       boxes;      // the entered instances of `updated` geometries, ascending: their world boxes change
  std::vector<int>       trees;  // the flattened instances among `moved` and of `updated` geometries, ascending: their world-space trees are rebuilt
  std::vector<NodeRange> ranges;
  bool   topLevel = false;
  size_t totalNodes = 0, totalSlots = 0; // nodes the ranged tail quantises, triangle slots the rebuilt trees rewrite
};

inline void updatePlanWith(const SceneLayout& s, const int* instanceGeometry, const int* geometryTriangles, const int* moved, int numMoved,
                           const int* updated, int numUpdated, UpdatePlan& p)
{
  p = UpdatePlan();
  const int numInstances = (int) s.flattened.size();
  std::vector<char> changed(s.needsBlas.size(), 0); // per geometry: its vertices are new
  for (int k = 0; k < numUpdated; ++k) changed[(size_t) updated[k]] = 1;
  for (size_t g = 0; g < changed.size(); ++g) if (changed[g] && s.needsBlas[g]) p.geometries.push_back((int) g);
  for (int k = 0; k < numMoved; ++k) if (s.flattened[(size_t) moved[k]]) p.trees.push_back(moved[k]);
  for (int i = 0; i < numInstances && numUpdated > 0; ++i)
  {
    if (!changed[(size_t) instanceGeometry[i]]) continue;
    if (!s.flattened[(size_t) i]) p.boxes.push_back(i);
    else if (std::find(p.trees.begin(), p.trees.end(), i) == p.trees.end()) p.trees.push_back(i);
  }
  std::sort(p.trees.begin(), p.trees.end());
  for (int g : p.geometries)
  {
    p.ranges.push_back({s.geometryNodeBase[(size_t) g], treeNodes(geometryTriangles[g])});
    p.totalSlots += (size_t) geometryTriangles[g];
  }
  for (int i : p.trees)
  {
    const int n = geometryTriangles[instanceGeometry[i]];
    p.ranges.push_back({s.flatNodeBase[(size_t) i], treeNodes(n)});
    p.totalSlots += (size_t) n;
  }
  p.topLevel = !s.single;
  if (p.topLevel) p.ranges.push_back({s.tlasBase, (int) (s.numNodes - (size_t) s.tlasBase)});
  p.ranges.push_back({(int) s.numNodes, 2});
  for (const NodeRange& r : p.ranges) p.totalNodes += (size_t) r.count;
}

inline void updatePlan(const SceneLayout& s, const int* instanceGeometry, const int* geometryTriangles, const int* moved, int numMoved, UpdatePlan& p)
{
  updatePlanWith(s, instanceGeometry, geometryTriangles, moved, numMoved, nullptr, 0, p);
}

} // namespace twk
