// Stand-alone driver of csrc/refit_scene_plan.h for tests/test_scene_refit_host.py, built with -fsanitize=address,undefined: reads
// cases from a text file, plans each with sceneLayout, updatePlanWith and refitScenePlan — the calls twk_refit_scene and
// twk_scene_refit_plan_host make — and prints every table, one line each, as the library's host call must return them.
// A case: numInstances numGeometries maxTriangles maxReferences maxLeaf numMoved numUpdated, then the instance geometries, the
// geometry triangles, the moved instances, the updated geometries.
#include "refit_scene_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace twk;

static bool readInts(FILE* f, std::vector<int>& out, int count)
{
  out.resize((size_t) count);
  for (int k = 0; k < count; ++k) if (fscanf(f, "%d", &out[(size_t) k]) != 1) return false;
  return true;
}

static void line(const char* name, const std::vector<int>& values)
{
  printf("%s", name);
  for (int v : values) printf(" %d", v);
  printf("\n");
}

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: scene_refit_plan_host cases.txt\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int head[7], cases = 0;
  while (fscanf(f, "%d %d %d %d %d %d %d", &head[0], &head[1], &head[2], &head[3], &head[4], &head[5], &head[6]) == 7)
  {
    std::vector<int> instanceGeometry, geometryTriangles, moved, updated;
    if (!readInts(f, instanceGeometry, head[0]) || !readInts(f, geometryTriangles, head[1]) || !readInts(f, moved, head[5]) || !readInts(f, updated, head[6]))
    { fprintf(stderr, "case %d is cut short\n", cases); return 2; }
    SceneLayout layout;
    sceneLayout(instanceGeometry.data(), head[0], geometryTriangles.data(), head[1], head[2], head[3], head[4], true, layout);
    UpdatePlan u;
    updatePlanWith(layout, instanceGeometry.data(), geometryTriangles.data(), moved.data(), head[5], updated.data(), head[6], u);
    RefitScenePlan p;
    if (const char* why = refitScenePlan(layout, instanceGeometry.data(), geometryTriangles.data(), u, moved.data(), head[5], updated.data(), head[6], p)) { fprintf(stderr, "case %d: %s\n", cases, why); return 1; }
    printf("case %d\n", cases);
    printf("totals %d %d %d %d %d %d %llu %llu %llu %llu\n", (int) p.tree.size(), p.batch.totalNodeBlocks, p.batch.totalSlotBlocks, REFIT_BATCH_BLOCK, (int) p.directLeaves.size(),
           u.topLevel ? 1 : 0, (unsigned long long) p.batch.totalNodes, (unsigned long long) p.batch.totalSlots, (unsigned long long) u.totalSlots, (unsigned long long) p.slotBytes);
    line("trees", p.tree); line("kinds", p.kind); line("nodeBases", p.nodeBase); line("nodeCounts", p.nodes); line("slotBases", p.slotBase); line("slotCounts", p.slots);
    line("nodeOffsets", p.batch.nodeOffset); line("slotOffsets", p.batch.slotOffset); line("nodeBlockFirst", p.batch.nodeBlockFirst); line("slotBlockFirst", p.batch.slotBlockFirst);
    std::vector<int> table;
    for (const RefitBatchBlock& b : p.batch.nodeBlocks) { table.push_back(b.tree); table.push_back(b.first); }
    line("nodeBlockTable", table);
    table.clear();
    for (const RefitBatchBlock& b : p.batch.slotBlocks) { table.push_back(b.tree); table.push_back(b.first); }
    line("slotBlockTable", table);
    line("directLeafInstances", p.directLeaves);
    line("boxInstances", p.boxes);
    ++cases;
  }
  fclose(f);
  printf("cases %d\n", cases);
  return 0;
}
