// Stand-alone program for the address and undefined-behaviour sanitizers: csrc/update_plan.h's updatePlanWith on the scenes of
// tests/selective_scenes.py, printing "scene geometries g.. boxes i.. trees i.. top total rewritten : ranges" per plan
// (tests/test_vertex_update_plan_host.py compares the lines with twk_vertex_update_plan_host's answers and with hand-written
// boxes, which the C struct does not carry). No HIP, no library.
#include "update_plan.h"

#include <cstdio>
#include <vector>

using namespace twk;

static void plan(const char* name, const std::vector<int>& instanceGeometry, const std::vector<int>& triangles, int maxTriangles, int maxReferences,
                 const std::vector<int>& moved, const std::vector<int>& updated)
{
  SceneLayout layout;
  sceneLayout(instanceGeometry.data(), (int) instanceGeometry.size(), triangles.data(), (int) triangles.size(), maxTriangles, maxReferences, 2, true, layout);
  UpdatePlan p;
  updatePlanWith(layout, instanceGeometry.data(), triangles.data(), moved.data(), (int) moved.size(), updated.data(), (int) updated.size(), p);
  std::printf("%s geometries", name);
  for (int g : p.geometries) std::printf(" %d", g);
  std::printf(" boxes");
  for (int i : p.boxes) std::printf(" %d", i);
  std::printf(" trees");
  for (int i : p.trees) std::printf(" %d", i);
  std::printf(" top %d total %zu rewritten %zu :", p.topLevel ? 1 : 0, p.totalNodes, p.totalSlots);
  for (const NodeRange& r : p.ranges) std::printf(" %d+%d", r.first, r.count);
  std::printf("\n");
}

int main()
{
  const std::vector<int> triangles = {2, 2, 2, 2, 12, 48};
  plan("flat", {0, 1, 2, 3, 4, 5}, triangles, 4, 2, {}, {5});
  plan("two-level", {0, 1, 2, 3, 5, 5, 5}, triangles, 0, 0, {}, {5});
  plan("mixed", {0, 1, 2, 3, 5, 5, 5, 4}, triangles, 0, 1, {}, {4, 5});
  plan("mixed-moved", {0, 1, 2, 3, 5, 5, 5, 4}, triangles, 0, 1, {7, 4}, {5});
  plan("single", {5}, triangles, 4, 2, {}, {5});
  std::vector<int> many = {0, 1, 2, 3};
  for (int k = 0; k < 12; ++k) many.push_back(4);
  plan("many", many, triangles, 12, 0, {}, {4});
  plan("unreferenced", {0, 1, 2, 3, 5, 5, 5}, triangles, 0, 0, {}, {4});
  plan("one-triangle", {0}, {1}, 4, 2, {}, {0});
  plan("nothing", {0, 1}, {1, 3}, 0, 0, {}, {});
  return 0;
}
