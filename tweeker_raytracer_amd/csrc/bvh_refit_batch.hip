// The refit of all moved trees of one call (twk_refit_instance_transform[s]; device_scene.hip updateSelective is the caller): the
// launches of bvh_refit.hip once for T trees instead of once per tree — one memset, four launches, one read-back, one wait, whatever
// T is. refit_batch_plan.h says which block works on which tree; bvh_refit.h is the per-slot and per-node definition, unchanged.
//   refitMovedSlotsKernel   one thread per slot: the three world-space float4 again through the instance's new matrix (moveTriangle);
//                           the shading record is object-space and stays: 48 B written per slot where refitSlotsKernel writes 176
//   refitBatchParentsKernel one thread per node: the parent of each inner child (parents start at -1: the memset); zeroes the ticket
//   refitBatchNodesKernel   one thread per node: refitNodesKernel's body and ticket scheme, on the tree its block belongs to
//   refitBatchTermsKernel   one thread per node: refitTermsKernel's reduction per block — a block is one tree's, and covers the local
//                           range the tree's own launch would give it, so the sums are the same in the same order; the block of a
//                           tree's root also writes the tree's box
// Every thread finds its tree through its block's table entry and reads the tree's record (RefitBatchTree) from a device table.
#include "bvh_refit.h"
#include "bvh_build.h"
#include "refit_batch_plan.h"

#include <cstring>

namespace twk {

static_assert(sizeof(RefitBatchTree) == 64 && sizeof(RefitBatchBlock) == 8, "the upload's layout");

__global__ void __launch_bounds__(256) refitMovedSlotsKernel(const RefitBatchTree* __restrict__ trees, const RefitBatchBlock* __restrict__ blocks,
                                                             const float* __restrict__ attributes, const unsigned int* __restrict__ indices, const int4* __restrict__ soup,
                                                             const DevInstance* __restrict__ instances, float4* triangles)
{
  const RefitBatchBlock block = blocks[blockIdx.x];
  const RefitBatchTree tree = trees[block.tree];
  const int s = block.first + (int) threadIdx.x;
  if (s >= tree.tree.numSlots) return;
  float4* slots = triangles + 3 * (size_t) tree.tree.slotBase;
  const unsigned int prim = asUint(slots[3 * (size_t) s].w);
  if (prim >= (unsigned int) tree.tree.numSlots) return; // the build wrote every primitive of the geometry once: never taken
  moveTriangle(attributes, indices, soup + tree.slotOffset, instances, prim, s, slots);
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

// refitNodesKernel (bvh_refit.hip) on the tree of the block: the same arrivals — the stores, __threadfence, the wait for it, the
// atomicAdd — and the same acquire by the last arrival; no thread waits for another, and a path to the root stays inside the tree, so
// the level loop is bounded by the tree's own node count. The trees of a batch share no node, no slot and no ticket.
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

// The scratch of a batch, in 4-byte words: what is uploaded — the tree table, the two block tables — then parents and tickets at the
// running node offsets, then what is read back — two doubles per node block, six floats per tree.
namespace {
struct BatchLayout { size_t trees, nodeBlocks, slotBlocks, uploaded, parents, tickets, partials, boxes, total; };
BatchLayout batchLayout(const RefitBatchPlan& p)
{
  BatchLayout l;
  const size_t numTrees = p.nodeOffset.size();
  l.trees = 0;
  l.nodeBlocks = l.trees + 16 * numTrees;
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

size_t refitBatchScratchWords(const RefitBatchPlan& plan) { return batchLayout(plan).total; }

hipError_t launchRefitTrees(hipStream_t stream, const float* attributes, const unsigned int* indices, const int4* soup, const DevInstance* instances,
                            BvhNode* nodes, BvhNode* wide, float* nodeCost, float4* triangles, const int* pairFlags, const RefitBatchPlan& plan,
                            const int* nodeBase, const int* numNodes, const int* slotBase, const int* numSlots, unsigned int* scratch, float* rootBounds, double* terms)
{
  const size_t numTrees = plan.nodeOffset.size();
  const BatchLayout l = batchLayout(plan);
  // the one upload: every tree's record, then the block tables; it lives until the wait below
  std::vector<unsigned int> upload(l.uploaded);
  RefitBatchTree* records = reinterpret_cast<RefitBatchTree*>(upload.data() + l.trees);
  for (size_t k = 0; k < numTrees; ++k)
  {
    RefitTree& t = records[k].tree;
    t.nodes = nodes + nodeBase[k]; t.wide = wide + 2 * (size_t) nodeBase[k]; t.nodeCost = nodeCost ? nodeCost + nodeBase[k] : nullptr;
    t.triangles = triangles + 3 * (size_t) slotBase[k]; t.pairFlags = pairFlags ? pairFlags + slotBase[k] : nullptr;
    t.nodeBase = nodeBase[k]; t.numNodes = numNodes[k]; t.slotBase = slotBase[k]; t.numSlots = numSlots[k];
    records[k].nodeOffset = plan.nodeOffset[k]; records[k].slotOffset = plan.slotOffset[k];
  }
  memcpy(upload.data() + l.nodeBlocks, plan.nodeBlocks.data(), sizeof(RefitBatchBlock) * plan.nodeBlocks.size());
  memcpy(upload.data() + l.slotBlocks, plan.slotBlocks.data(), sizeof(RefitBatchBlock) * plan.slotBlocks.size());
  REFIT_CHECK(hipMemcpyAsync(scratch, upload.data(), sizeof(unsigned int) * upload.size(), hipMemcpyHostToDevice, stream));
  const RefitBatchTree* d_trees = reinterpret_cast<const RefitBatchTree*>(scratch + l.trees);
  const RefitBatchBlock* d_nodeBlocks = reinterpret_cast<const RefitBatchBlock*>(scratch + l.nodeBlocks);
  const RefitBatchBlock* d_slotBlocks = reinterpret_cast<const RefitBatchBlock*>(scratch + l.slotBlocks);
  int* parents = reinterpret_cast<int*>(scratch + l.parents);
  unsigned int* tickets = scratch + l.tickets;
  double* partials = reinterpret_cast<double*>(scratch + l.partials);
  float* boxes = reinterpret_cast<float*>(scratch + l.boxes);

  hipLaunchKernelGGL(refitMovedSlotsKernel, dim3(plan.totalSlotBlocks), dim3(256), 0, stream, d_trees, d_slotBlocks, attributes, indices, soup, instances, triangles);
  REFIT_CHECK(hipMemsetAsync(parents, 0xff, sizeof(int) * plan.totalNodes, stream)); // -1: no parent
  hipLaunchKernelGGL(refitBatchParentsKernel, dim3(plan.totalNodeBlocks), dim3(256), 0, stream, d_trees, d_nodeBlocks, parents, tickets);
  hipLaunchKernelGGL(refitBatchNodesKernel, dim3(plan.totalNodeBlocks), dim3(256), 0, stream, d_trees, d_nodeBlocks, parents, tickets);
  hipLaunchKernelGGL(refitBatchTermsKernel, dim3(plan.totalNodeBlocks), dim3(256), 0, stream, d_trees, d_nodeBlocks, parents, partials, boxes);
  REFIT_CHECK(hipGetLastError());
  // the one read-back: the partial sums and, behind them, the root boxes
  std::vector<unsigned int> back(4 * (size_t) plan.totalNodeBlocks + 6 * numTrees);
  REFIT_CHECK(hipMemcpyAsync(back.data(), partials, sizeof(unsigned int) * back.size(), hipMemcpyDeviceToHost, stream));
  REFIT_CHECK(hipStreamSynchronize(stream));
  for (size_t k = 0; k < numTrees; ++k)
  {
    const int blocks = (numNodes[k] + REFIT_BATCH_BLOCK - 1) / REFIT_BATCH_BLOCK;
    double inner = 0.0, leaf = 0.0, sums[2];
    for (int b = 0; b < blocks; ++b) // a tree's blocks by index, as launchRefitTree adds them
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
