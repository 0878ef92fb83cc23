// The refit of every tree a frame's edits touch (twk_refit_scene; device_scene.hip refitScene is the caller): the launches of
// bvh_refit_batch.hip for a batch of MIXED trees — the bottom-level trees of edited geometries, the world-space trees of instances
// of edited geometries, the world-space trees of moved instances — one upload, one slots launch, one memset, three launches, one
// read-back, one wait. refit_scene_plan.h says which tree is of which kind, refit_batch_plan.h which block works on which tree;
// bvh_refit.h is the per-slot and per-node definition, unchanged.
//   refitSceneSlotsKernel   one thread per slot, one tree per block. The kind is the block's, so the branch is uniform:
//                             0  emitTriangle on the geometry's own vertices and indices (object space, no descriptor)
//                             1  emitTriangle through the instance's record: world-space slot + the 128-byte shading record
//                             2  moveTriangle: the world-space slot only, the shading record is object-space and stays
//                           The soup descriptor of kinds 1 and 2 — (instance, attributeBase, indexBase + 3 prim, prim) — is made in
//                           registers from the tree's 16-byte record and the primitive word the slot holds: no descriptor array is
//                           written by a launch of its own and none is read (16 B per slot less each way than the per-tree path).
//   parents, nodes, terms   refitBatchParentsKernel, refitBatchNodesKernel, refitBatchTermsKernel of bvh_refit_batch.hip as they are
// Compulsory bytes per slot: 12 of indices, three 48-byte vertex records, the 16-byte primitive word; written 176 (kinds 0, 1) or 48 (kind 2).
#include "bvh_refit_scene.h"
#include "bvh_build.h"

#include <cstring>

namespace twk {

static_assert(sizeof(RefitBatchTree) == 64 && sizeof(RefitBatchBlock) == 8 && sizeof(RefitSceneKind) == 16, "the upload's layout");

__global__ void __launch_bounds__(256) refitSceneSlotsKernel(const RefitBatchTree* __restrict__ trees, const RefitSceneKind* __restrict__ kinds,
                                                             const RefitBatchBlock* __restrict__ blocks, const float* __restrict__ attributes,
                                                             const unsigned int* __restrict__ indices, const DevInstance* __restrict__ instances,
                                                             float4* triangles, float4* shadeTriangles)
{
  const RefitBatchBlock block = blocks[blockIdx.x];
  const RefitBatchTree tree = trees[block.tree];
  const RefitSceneKind k = kinds[block.tree];
  const int s = block.first + (int) threadIdx.x;
  if (s >= tree.tree.numSlots) return;
  float4* slots = triangles + 3 * (size_t) tree.tree.slotBase;
  float4* shade = shadeTriangles + TWK_SHADE_RECORD * (size_t) tree.tree.slotBase;
  const unsigned int prim = asUint(slots[3 * (size_t) s].w);
  if (prim >= (unsigned int) tree.tree.numSlots) return; // the build wrote every primitive of the geometry once: never taken
  if (k.kind == REFIT_SCENE_GEOMETRY)
  {
    emitTriangle(attributes + 12 * (size_t) k.attributeBase, indices + k.indexBase, nullptr, nullptr, prim, s, slots, shade);
    return;
  }
  // BvhBuilder::soupDescriptors' descriptor of the primitive, as the one element of a soup
  const int4 d = make_int4(k.instance, k.attributeBase, k.indexBase + 3 * (int) prim, (int) prim);
  if (k.kind == REFIT_SCENE_EDITED) emitTriangle(attributes, indices, &d, instances, 0u, s, slots, shade);
  else moveTriangle(attributes, indices, &d, instances, 0u, s, slots);
}

#define REFIT_CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// The scratch of a call, in 4-byte words: what is uploaded — the tree table, the kind table, the two block tables — then parents and
// tickets at the running node offsets, then what is read back — two doubles per node block, six floats per tree.
namespace {
struct SceneLayoutWords { size_t trees, kinds, nodeBlocks, slotBlocks, uploaded, parents, tickets, partials, boxes, total; };
SceneLayoutWords sceneLayoutWords(const RefitBatchPlan& p)
{
  SceneLayoutWords l;
  const size_t numTrees = p.nodeOffset.size();
  l.trees = 0;
  l.kinds = l.trees + 16 * numTrees;
  l.nodeBlocks = l.kinds + 4 * numTrees;
  l.slotBlocks = l.nodeBlocks + 2 * (size_t) p.totalNodeBlocks;
  l.uploaded = l.slotBlocks + 2 * (size_t) p.totalSlotBlocks;
  l.parents = (l.uploaded + 3) & ~(size_t) 3;
  l.tickets = l.parents + p.totalNodes;
  l.partials = (l.tickets + p.totalNodes + 3) & ~(size_t) 3; // 16-byte aligned
  l.boxes = l.partials + 4 * (size_t) p.totalNodeBlocks;
  l.total = l.boxes + 6 * numTrees + 16;
  return l;
}
}

size_t refitSceneScratchWords(const RefitScenePlan& plan) { return sceneLayoutWords(plan.batch).total; }

hipError_t launchRefitSceneTrees(hipStream_t stream, const float* attributes, const unsigned int* indices, const DevInstance* instances, BvhNode* nodes, BvhNode* wide,
                                 float* nodeCost, float4* triangles, float4* shadeTriangles, const int* pairFlags, const RefitScenePlan& scene, const RefitSceneKind* kinds,
                                 unsigned int* scratch, float* rootBounds, double* terms)
{
  const RefitBatchPlan& plan = scene.batch;
  const size_t numTrees = scene.tree.size();
  if (numTrees == 0 || plan.nodeOffset.size() != numTrees) return hipErrorInvalidValue;
  const SceneLayoutWords l = sceneLayoutWords(plan);
  // the one upload: every tree's record and kind, then the block tables; it lives until the wait below
  std::vector<unsigned int> upload(l.uploaded);
  RefitBatchTree* records = reinterpret_cast<RefitBatchTree*>(upload.data() + l.trees);
  for (size_t k = 0; k < numTrees; ++k)
  {
    RefitTree& t = records[k].tree;
    const int nodeBase = scene.nodeBase[k], slotBase = scene.slotBase[k];
    t.nodes = nodes + nodeBase; t.wide = wide + 2 * (size_t) nodeBase; t.nodeCost = nodeCost ? nodeCost + nodeBase : nullptr;
    t.triangles = triangles + 3 * (size_t) slotBase; t.pairFlags = pairFlags ? pairFlags + slotBase : nullptr;
    t.nodeBase = nodeBase; t.numNodes = scene.nodes[k]; t.slotBase = slotBase; t.numSlots = scene.slots[k];
    records[k].nodeOffset = plan.nodeOffset[k]; records[k].slotOffset = plan.slotOffset[k];
  }
  memcpy(upload.data() + l.kinds, kinds, sizeof(RefitSceneKind) * numTrees);
  memcpy(upload.data() + l.nodeBlocks, plan.nodeBlocks.data(), sizeof(RefitBatchBlock) * plan.nodeBlocks.size());
  memcpy(upload.data() + l.slotBlocks, plan.slotBlocks.data(), sizeof(RefitBatchBlock) * plan.slotBlocks.size());
  REFIT_CHECK(hipMemcpyAsync(scratch, upload.data(), sizeof(unsigned int) * upload.size(), hipMemcpyHostToDevice, stream));
  const RefitBatchTree* d_trees = reinterpret_cast<const RefitBatchTree*>(scratch + l.trees);
  const RefitSceneKind* d_kinds = reinterpret_cast<const RefitSceneKind*>(scratch + l.kinds);
  const RefitBatchBlock* d_nodeBlocks = reinterpret_cast<const RefitBatchBlock*>(scratch + l.nodeBlocks);
  const RefitBatchBlock* d_slotBlocks = reinterpret_cast<const RefitBatchBlock*>(scratch + l.slotBlocks);
  int* parents = reinterpret_cast<int*>(scratch + l.parents);
  unsigned int* tickets = scratch + l.tickets;
  double* partials = reinterpret_cast<double*>(scratch + l.partials);
  float* boxes = reinterpret_cast<float*>(scratch + l.boxes);

  hipLaunchKernelGGL(refitSceneSlotsKernel, dim3(plan.totalSlotBlocks), dim3(256), 0, stream, d_trees, d_kinds, d_slotBlocks, attributes, indices, instances, triangles, shadeTriangles);
  REFIT_CHECK(hipMemsetAsync(parents, 0xff, sizeof(int) * plan.totalNodes, stream)); // -1: no parent
  hipLaunchKernelGGL(refitBatchParentsKernel, dim3(plan.totalNodeBlocks), dim3(256), 0, stream, d_trees, d_nodeBlocks, parents, tickets);
  hipLaunchKernelGGL(refitBatchNodesKernel, dim3(plan.totalNodeBlocks), dim3(256), 0, stream, d_trees, d_nodeBlocks, (const int*) parents, tickets);
  hipLaunchKernelGGL(refitBatchTermsKernel, dim3(plan.totalNodeBlocks), dim3(256), 0, stream, d_trees, d_nodeBlocks, (const int*) parents, partials, boxes);
  REFIT_CHECK(hipGetLastError());
  // the one read-back: the partial sums and, behind them, the root boxes
  std::vector<unsigned int> back(4 * (size_t) plan.totalNodeBlocks + 6 * numTrees);
  REFIT_CHECK(hipMemcpyAsync(back.data(), partials, sizeof(unsigned int) * back.size(), hipMemcpyDeviceToHost, stream));
  REFIT_CHECK(hipStreamSynchronize(stream));
  for (size_t k = 0; k < numTrees; ++k)
  {
    const int blocks = (scene.nodes[k] + REFIT_BATCH_BLOCK - 1) / REFIT_BATCH_BLOCK;
    double inner = 0.0, leaf = 0.0, sums[2];
    for (int b = 0; b < blocks; ++b) // a tree's blocks by index, as launchRefitTree and launchRefitTrees add them
    {
      memcpy(sums, back.data() + 4 * ((size_t) plan.nodeBlockFirst[k] + (size_t) b), sizeof(sums));
      inner += sums[0]; leaf += sums[1];
    }
    terms[2 * k] = inner; terms[2 * k + 1] = leaf;
    memcpy(rootBounds + 6 * k, back.data() + 4 * (size_t) plan.totalNodeBlocks + 6 * k, sizeof(float) * 6);
  }
  return hipSuccess;
}

} // namespace twk
