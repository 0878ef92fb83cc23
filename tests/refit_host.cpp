// A stand-alone program for tests/test_refit_host.py: the host form of a tree's refit (csrc/bvh_refit.h refitTreeRefusal and
// refitTreeHost — the code twk_refit_tree_host runs after the refusals of its arguments), compiled by the test with
// -fsanitize=address,undefined and run on the cases it writes to a file. Nothing of it is loaded into Python.
//   refit_host <case file> <result file>
// case:   int32 numNodes, numSlots, numAttributes, nodeBase, slotBase, leafFlag, idInstance, hasCost, hasFlags; nodes [numNodes x 16
//         float32]; wide nodes [numNodes x 32]; node costs [numNodes] (hasCost); slots [numSlots x 12]; pair flags [numSlots int32]
//         (hasFlags); attributes [numAttributes x 12 float32]; indices [3 numSlots uint32]; transform [12 float32]
// result: nodes, wide nodes, node costs (hasCost), slots, shading records [numSlots x 32 float32], terms [2 float64], root box [6 float32]
#include "bvh_refit.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace twk;

template<typename T> static std::vector<T> take(FILE* f, size_t count)
{
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "refit_host: the case file is short\n"); exit(2); }
  return v;
}

template<typename T> static void give(FILE* f, const std::vector<T>& v)
{
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "refit_host: cannot write the result\n"); exit(2); }
}

int main(int argc, char** argv)
{
  if (argc != 3) { fprintf(stderr, "usage: refit_host <case> <result>\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "refit_host: cannot open %s\n", argv[1]); return 2; }
  const std::vector<int> head = take<int>(in, 9);
  const size_t numNodes = (size_t) head[0], numSlots = (size_t) head[1], numAttributes = (size_t) head[2];
  const int nodeBase = head[3], slotBase = head[4], leafFlag = head[5], idInstance = head[6];
  const bool hasCost = head[7] != 0, hasFlags = head[8] != 0;
  std::vector<BvhNode> nodes = take<BvhNode>(in, numNodes), wide = take<BvhNode>(in, 2 * numNodes);
  std::vector<float> cost = take<float>(in, hasCost ? numNodes : 0);
  std::vector<float4> slots = take<float4>(in, 3 * numSlots);
  const std::vector<int> flags = take<int>(in, hasFlags ? numSlots : 0);
  const std::vector<float> attributes = take<float>(in, 12 * numAttributes);
  const std::vector<unsigned int> indices = take<unsigned int>(in, 3 * numSlots);
  const std::vector<float> transform = take<float>(in, 12);
  fclose(in);

  RefitTree tree;
  tree.nodes = nodes.data(); tree.wide = wide.data(); tree.nodeCost = hasCost ? cost.data() : nullptr;
  tree.triangles = slots.data(); tree.pairFlags = hasFlags ? flags.data() : nullptr;
  tree.nodeBase = nodeBase; tree.numNodes = (int) numNodes; tree.slotBase = slotBase; tree.numSlots = (int) numSlots;
  std::vector<int> parents;
  if (const char* why = refitTreeRefusal(tree, numSlots, parents)) { fprintf(stderr, "refit_host: %s\n", why); return 3; }
  std::vector<int4> soup;
  std::vector<DevInstance> instances;
  if (leafFlag != 0) refitSoupHost((int) numSlots, idInstance, transform.data(), soup, instances);
  std::vector<float4> shade(TWK_SHADE_RECORD * numSlots);
  std::vector<double> terms(2);
  std::vector<float> bounds(6);
  refitTreeHost(tree, parents, attributes.data(), indices.data(), leafFlag ? soup.data() : nullptr, leafFlag ? instances.data() : nullptr, slots.data(), shade.data(), terms.data(), bounds.data());

  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "refit_host: cannot write %s\n", argv[2]); return 2; }
  give(out, nodes); give(out, wide); give(out, cost); give(out, slots); give(out, shade); give(out, terms); give(out, bounds);
  fclose(out);
  return 0;
}
