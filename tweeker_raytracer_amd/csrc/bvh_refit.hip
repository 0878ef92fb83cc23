// The refit of trees on the device (bvh_refit.h is the per-slot and per-node definition; device_scene.hip refitTrees is the caller):
// every tree a call touches — the bottom-level trees of edited geometries, the world-space trees of instances of edited geometries,
// the world-space trees of moved instances — in ONE batch: one upload, one slots launch, one memset, three launches, one read-back,
// one wait, whatever the number and the kinds of the trees. No sort, no topology, no scan. refit_scene_plan.h says which tree is of
// which kind, refit_batch_plan.h which block works on which tree.
//   refitSceneSlotsKernel   one thread per slot, one tree per block. The kind is the block's, so the branch is uniform:
//                             0  emitTriangle on the geometry's own vertices and indices (object space, no descriptor)
//                             1  emitTriangle through the instance's record: world-space slot + the 128-byte shading record
//                             2  moveTriangle: the world-space slot only, the shading record is object-space and stays
//                           The soup descriptor of kinds 1 and 2 — (instance, attributeBase, indexBase + 3 prim, prim) — is made in
//                           registers from the tree's 16-byte record and the primitive word the slot holds: no descriptor array is
//                           written and none is read.
//   refitBatchParentsKernel one thread per node: the parent of each inner child, from the child references (parents start at -1: the
//                           memset); zeroes the node's ticket
//   refitBatchNodesKernel   one thread per node: the boxes of its leaf children, then bottom-up with refitKernel's ticket scheme
//                           (bvh_build.hip), on the tree its block belongs to
//   refitBatchTermsKernel   one thread per node: the SAH terms, reduced per block in a fixed order; the host adds a tree's blocks by
//                           index. The block of a tree's root also writes the tree's box
// Every thread finds its tree through its block's table entry and reads the tree's record (RefitBatchTree) from a device table.
// Compulsory bytes per slot: 12 of indices, three 48-byte vertex records, the 16-byte primitive word; written 176 (kinds 0, 1) or 48
// (kind 2). Per used node: 64 + 128 written for the node and its wide node; the node kernel reads each slot once more for the boxes.
#include "bvh_refit.h"
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

__global__ void __launch_bounds__(256) refitBatchParentsKernel(const RefitBatchTree* __restrict__ trees, const RefitBatchBlock* __restrict__ blocks,
                                                               int* __restrict__ allParents, unsigned int* __restrict__ allTickets)
{
  const RefitBatchBlock block = blocks[blockIdx.x];
  const RefitBatchTree tree = trees[block.tree];
  const RefitTree t = tree.tree;
  const int i = block.first + (int) threadIdx.x;
  if (i >= t.numNodes) return;
  int* parents = allParents + tree.nodeOffset;
  allTickets[tree.nodeOffset + i] = 0u;
  int c0, c1;
  refitChildren(t.nodes + i, c0, c1);
  if (refitUnused(c0, c1)) return;
  if (c0 >= 0 && (unsigned int) (c0 - t.nodeBase) < (unsigned int) t.numNodes) parents[c0 - t.nodeBase] = i;
  if (c1 >= 0 && (unsigned int) (c1 - t.nodeBase) < (unsigned int) t.numNodes) parents[c1 - t.nodeBase] = i;
}

// Whether an inner reference stays in the tree (the build's always do; a stray one must not become an address)
TWK_D bool refitBatchInside(const RefitTree& t, int ref) { return (unsigned int) (ref - t.nodeBase) < (unsigned int) t.numNodes; }

// A node is complete once its own thread (the boxes of its leaf children) and the thread that finished each inner child (that child's
// box) have arrived: 1 + inner children arrivals, counted by a ticket. Every arrival is a release — the stores, __threadfence, the
// wait for it, the atomicAdd — and the last arrival an acquire: __threadfence, then plain vector loads of what the others stored
// (neither pointer is __restrict__: handed-off bytes stay off the scalar path). No thread waits for another; a thread that is not the
// last returns, so no block depends on another being resident. A path to the root stays inside the tree, so the level loop is bounded
// by the tree's own node count. The trees of a batch share no node, no slot and no ticket.
__global__ void __launch_bounds__(256) refitBatchNodesKernel(const RefitBatchTree* __restrict__ trees, const RefitBatchBlock* __restrict__ blocks,
                                                             const int* allParents, unsigned int* allTickets)
{
  const RefitBatchBlock block = blocks[blockIdx.x];
  const RefitBatchTree tree = trees[block.tree];
  const RefitTree t = tree.tree;
  const int i = block.first + (int) threadIdx.x;
  if (i >= t.numNodes) return;
  const int* parents = allParents + tree.nodeOffset;
  unsigned int* tickets = allTickets + tree.nodeOffset;
  int c0, c1;
  refitChildren(t.nodes + i, c0, c1);
  if (refitUnused(c0, c1)) return;
  if ((c0 >= 0 && !refitBatchInside(t, c0)) || (c1 >= 0 && !refitBatchInside(t, c1))) return;
  {
    float4 lo, hi, tlo, thi;
    int triangles; bool single;
    if (c0 < 0) { refitLeafBox(t, c0, lo, hi, tlo, thi, triangles, single); if (triangles > 0) refitStoreChildBox(t.nodes + i, 0, lo, hi); }
    if (c1 < 0 && !refitNeverHit(t.nodes + i)) { refitLeafBox(t, c1, lo, hi, tlo, thi, triangles, single); if (triangles > 0) refitStoreChildBox(t.nodes + i, 1, lo, hi); }
  }
  int node = i;
  for (int level = 0; level < t.numNodes; ++level) // a path to the root is shorter than the tree has nodes
  {
    int a0, a1;
    refitChildren(t.nodes + node, a0, a1);
    const unsigned int needed = 1u + (a0 >= 0 ? 1u : 0u) + (a1 >= 0 ? 1u : 0u);
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the fence's own wait may be dropped by the compiler; the ticket must not overtake the stores
    const unsigned int ticket = atomicAdd(&tickets[node], 1u);
    if (ticket + 1u != needed) return; // someone else will finish this node
    __threadfence();
    float4 lo, hi;
    refitNode(t, node, lo, hi);
    if (node == 0) return; // the root
    const int parent = parents[node];
    if ((unsigned int) parent >= (unsigned int) t.numNodes) return; // -1: a node inside a collapsed subtree, nobody's child (bvh_refit.h)
    int p0, p1;
    refitChildren(t.nodes + parent, p0, p1);
    refitStoreChildBox(t.nodes + parent, (p0 == t.nodeBase + node) ? 0 : 1, lo, hi);
    node = parent;
  }
}

__global__ void __launch_bounds__(256) refitBatchTermsKernel(const RefitBatchTree* __restrict__ trees, const RefitBatchBlock* __restrict__ blocks,
                                                             const int* __restrict__ allParents, double* __restrict__ partials, float* __restrict__ rootBoxes)
{
  __shared__ double sums[2][256];
  const RefitBatchBlock block = blocks[blockIdx.x];
  const RefitBatchTree tree = trees[block.tree];
  const RefitTree t = tree.tree;
  const int i = block.first + (int) threadIdx.x;
  double inner = 0.0, leaf = 0.0;
  if (i < t.numNodes && (i == 0 || allParents[tree.nodeOffset + i] >= 0)) refitNodeTerms(t, i, inner, leaf); // the nodes the root reaches
  sums[0][threadIdx.x] = inner; sums[1][threadIdx.x] = leaf;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) // the same pairs in the same order, whatever the scheduling
  {
    if ((int) threadIdx.x < step) { sums[0][threadIdx.x] += sums[0][threadIdx.x + step]; sums[1][threadIdx.x] += sums[1][threadIdx.x + step]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = sums[0][0]; partials[2 * blockIdx.x + 1] = sums[1][0]; }
  if (i == 0)
  {
    float4 lo, hi;
    refitRootBox(t.nodes, lo, hi);
    float* out = rootBoxes + 6 * (size_t) block.tree;
    out[0] = lo.x; out[1] = lo.y; out[2] = lo.z; out[3] = hi.x; out[4] = hi.y; out[5] = hi.z;
  }
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
    for (int b = 0; b < blocks; ++b) // a tree's blocks by index: the same sums in the same order, whatever else is in the batch
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
