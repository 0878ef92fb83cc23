// The trees of one refit call — a vertex refit, an instance refit or twk_refit_scene (bvh_refit.hip launchRefitSceneTrees;
// device_scene.hip refitTrees is the caller): the one place that turns an UpdatePlan (update_plan.h) and the scene's layout into the
// list of trees the call's ONE batch refits, and says what kind each is. A vertex refit gives kinds 0 and 1, an instance refit kind 2 only. Plain C++, no HIP: the call plans with refitScenePlan, and twk_scene_refit_plan_host hands the plan out
// without a device.
//
// The order: the bottom-level trees of the edited geometries that some instance enters, ascending by geometry, then the plan's
// flattened instances that have a tree of their own (not a direct leaf of the top level: that one takes the rebuild's path),
// ascending by instance. A tree's KIND says what its slot writer is (bvh_refit.h) and what it writes per slot:
//   0  bottom-level tree of an edited geometry               emitTriangle, object space, no descriptor      48 + 128 = 176 B
//   1  world-space tree of an instance of an edited geometry emitTriangle through the instance's record     48 + 128 = 176 B
//      (moved in the same call or not: the record holds the matrix the instance has now)
//   2  world-space tree of a moved instance of a geometry    moveTriangle: the shading record is            48 B
//      that was not edited                                   object-space and stays
// The blocks of the launches are refit_batch_plan.h's, unchanged: a block is one tree's, so a block's kind is uniform.
#pragma once
#include "refit_batch_plan.h"
#include "update_plan.h"

namespace twk {

constexpr int REFIT_SCENE_GEOMETRY = 0, REFIT_SCENE_EDITED = 1, REFIT_SCENE_MOVED = 2;
constexpr int REFIT_SCENE_SLOT_BYTES[3] = {176, 176, 48};

// What the slot kernel reads per tree beside its RefitBatchTree (which stays 64 bytes): the kind, the instance whose record holds the
// matrix (-1 for kind 0), and where the geometry's vertices and indices begin in the shared arrays. 16 bytes.
struct RefitSceneKind { int kind, instance, attributeBase, indexBase; };

struct RefitScenePlan
{
  std::vector<int> tree;                                // per tree: ~geometry (negative) for a bottom-level tree, else the instance
  std::vector<int> kind, geometry;                      // per tree: REFIT_SCENE_*, the geometry its triangles are of
  std::vector<int> nodeBase, nodes, slotBase, slots;    // per tree: its node and slot range in the scene's arrays
  std::vector<int> directLeaves;                        // the plan's direct-leaf instances, ascending: rebuilt, in front of the batch
  std::vector<int> boxes;                               // the entered instances whose world box the call writes, ascending: moved, or of an edited geometry
  size_t slotBytes = 0;                                 // bytes the slot kernel writes: the sum of slots x REFIT_SCENE_SLOT_BYTES[kind]
  RefitBatchPlan batch;                                 // empty when there is no tree
};

// Why the trees cannot be planned (refitBatchPlan's reasons), or nullptr. u: updatePlanWith's answer for the same layout, moved
// instances and updated geometries; moved / numMoved and updated / numUpdated: those instances and geometries (distinct, in range).
inline const char* refitScenePlan(const SceneLayout& s, const int* instanceGeometry, const int* geometryTriangles, const UpdatePlan& u,
                                  const int* moved, int numMoved, const int* updated, int numUpdated, RefitScenePlan& p)
{
  p = RefitScenePlan();
  std::vector<char> edited(s.needsBlas.size(), 0);
  for (int k = 0; k < numUpdated; ++k) edited[(size_t) updated[k]] = 1;
  const auto add = [&p](int tree, int kind, int geometry, int nodeBase, int slotBase, int triangles)
  {
    p.tree.push_back(tree); p.kind.push_back(kind); p.geometry.push_back(geometry);
    p.nodeBase.push_back(nodeBase); p.nodes.push_back(treeNodes(triangles)); p.slotBase.push_back(slotBase); p.slots.push_back(triangles);
    p.slotBytes += (size_t) triangles * (size_t) REFIT_SCENE_SLOT_BYTES[kind];
  };
  for (int g : u.geometries) add(~g, REFIT_SCENE_GEOMETRY, g, s.geometryNodeBase[(size_t) g], s.geometryTriangleBase[(size_t) g], geometryTriangles[g]);
  for (int i : u.trees)
  {
    const int g = instanceGeometry[i];
    if (s.directLeaf[(size_t) i]) { p.directLeaves.push_back(i); continue; }
    add(i, edited[(size_t) g] ? REFIT_SCENE_EDITED : REFIT_SCENE_MOVED, g, s.flatNodeBase[(size_t) i], s.flatTriangleBase[(size_t) i], geometryTriangles[g]);
  }
  p.boxes = u.boxes;
  for (int k = 0; k < numMoved; ++k)
    if (!s.flattened[(size_t) moved[k]] && !edited[(size_t) instanceGeometry[moved[k]]]) p.boxes.push_back(moved[k]);
  std::sort(p.boxes.begin(), p.boxes.end());
  if (p.tree.empty()) return nullptr;
  return refitBatchPlan(p.nodes.data(), p.slots.data(), (int) p.tree.size(), p.batch);
}

} // namespace twk
