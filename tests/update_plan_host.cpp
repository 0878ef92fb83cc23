// Stand-alone program for the address and undefined-behaviour sanitizers: csrc/update_plan.h on the scenes of
// tests/selective_scenes.py and on a few degenerate ones, printing "scene moved trees topLevel total ranges..." per plan
// (tests/test_update_plan_host.py compares the lines with twk_update_plan_host's answers). No HIP, no library.
#include "update_plan.h"

#include <cstdio>
#include <vector>

using namespace twk;

static void plan(const char* name, const std::vector<int>& instanceGeometry, const std::vector<int>& triangles, int maxTriangles, int maxReferences,
                 const std::vector<int>& moved)
{
  SceneLayout layout;
  sceneLayout(instanceGeometry.data(), (int) instanceGeometry.size(), triangles.data(), (int) triangles.size(), maxTriangles, maxReferences, 2, true, layout);
  UpdatePlan p;
  updatePlan(layout, instanceGeometry.data(), triangles.data(), moved.data(), (int) moved.size(), p);
  std::printf("%s nodes %zu slots %zu tlas %d trees %zu top %d total %zu rewritten %zu :", name, layout.numNodes, layout.numTriangles, layout.tlasBase, p.trees.size(),
              p.topLevel ? 1 : 0, p.totalNodes, p.totalSlots);
  for (const NodeRange& r : p.ranges) std::printf(" %d+%d", r.first, r.count);
  std::printf("\n");
}

int main()
{
  const std::vector<int> triangles = {2, 2, 2, 2, 12, 48};
  plan("flat", {0, 1, 2, 3, 4, 5}, triangles, 4, 2, {5, 4});
  plan("two-level", {0, 1, 2, 3, 5, 5, 5}, triangles, 0, 0, {5});
  plan("mixed", {0, 1, 2, 3, 5, 5, 5, 4}, triangles, 0, 1, {0, 1, 2, 3, 4, 5, 6, 7});
  plan("single", {5}, triangles, 4, 2, {0});
  std::vector<int> many = {0, 1, 2, 3};
  for (int k = 0; k < 12; ++k) many.push_back(4);
  plan("many", many, triangles, 12, 0, {15, 4});
  plan("one-triangle", {0}, {1}, 4, 2, {0});
  plan("nothing-moved", {0, 1}, {1, 3}, 0, 0, {});
  return 0;
}
