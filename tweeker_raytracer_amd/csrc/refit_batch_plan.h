// How the trees of one batched refit (bvh_refit.hip launchRefitSceneTrees) share its launches: the one place that decides which
// block of a launch works on which tree, and where each tree's parents, tickets and per-block partial sums stand.
// Plain C++, no HIP: the launcher plans with refitBatchPlan, and twk_refit_batch_plan_host hands the plan out without a device.
//
// Tree k has n_k nodes and s_k slots. It occupies ceil(n_k / 256) consecutive NODE blocks of the parents, nodes and terms launches
// and ceil(s_k / 256) consecutive SLOT blocks of the slots launch, the trees in the order given. Per block, a table entry names the
// tree and the tree-local index of the block's first thread: thread j of the block works on local index first + j, or on nothing when
// that is beyond the tree — so a block never straddles two trees, and block b of tree k covers the local indices
// [256 b, 256 b + 256), the range block b of a launch for the tree alone would cover. The 256-thread reduction of the terms is
// therefore the same sums in the same order whatever else is in the batch, and the host adds a tree's blocks by index: a tree's terms
// are bit-equal in every batch. Parents and tickets (one word per node) stand at the running node offset, a tree's partial sums at
// its first node block; the running slot offset counts the slots of the trees before it.
#pragma once
#include <cstddef>
#include <vector>

namespace twk {

constexpr int REFIT_BATCH_BLOCK = 256;

struct RefitBatchBlock { int tree, first; }; // the block's tree, the tree-local index of its first thread

struct RefitBatchPlan
{
  std::vector<int> nodeOffset, slotOffset;           // per tree: nodes / slots of the trees before it
  std::vector<int> nodeBlockFirst, slotBlockFirst;   // per tree: its first node block / slot block
  std::vector<RefitBatchBlock> nodeBlocks, slotBlocks;
  size_t totalNodes = 0, totalSlots = 0;
  int    totalNodeBlocks = 0, totalSlotBlocks = 0;
};

// Why the trees cannot be planned, or nullptr. The totals, and the threads of either launch, stay below 2^31: every index is an int.
inline const char* refitBatchPlan(const int* treeNodes, const int* treeSlots, int numTrees, RefitBatchPlan& p)
{
  p = RefitBatchPlan();
  if (numTrees < 1) return "no tree";
  const size_t limit = (size_t) 1 << 31;
  size_t nodes = 0, slots = 0, nodeBlocks = 0, slotBlocks = 0;
  for (int k = 0; k < numTrees; ++k)
  {
    if (treeNodes[k] < 1 || treeSlots[k] < 1) return "a tree without a node or without a slot";
    nodes += (size_t) treeNodes[k]; slots += (size_t) treeSlots[k];
    nodeBlocks += ((size_t) treeNodes[k] + REFIT_BATCH_BLOCK - 1) / REFIT_BATCH_BLOCK;
    slotBlocks += ((size_t) treeSlots[k] + REFIT_BATCH_BLOCK - 1) / REFIT_BATCH_BLOCK;
    if (nodes >= limit || slots >= limit || nodeBlocks * REFIT_BATCH_BLOCK >= limit || slotBlocks * REFIT_BATCH_BLOCK >= limit)
      return "2^31 or more nodes, slots or threads in one batch";
  }
  p.nodeOffset.resize((size_t) numTrees); p.slotOffset.resize((size_t) numTrees);
  p.nodeBlockFirst.resize((size_t) numTrees); p.slotBlockFirst.resize((size_t) numTrees);
  p.nodeBlocks.reserve(nodeBlocks); p.slotBlocks.reserve(slotBlocks);
  for (int k = 0; k < numTrees; ++k)
  {
    p.nodeOffset[(size_t) k] = (int) p.totalNodes; p.slotOffset[(size_t) k] = (int) p.totalSlots;
    p.nodeBlockFirst[(size_t) k] = (int) p.nodeBlocks.size(); p.slotBlockFirst[(size_t) k] = (int) p.slotBlocks.size();
    for (int first = 0; first < treeNodes[k]; first += REFIT_BATCH_BLOCK) p.nodeBlocks.push_back({k, first});
    for (int first = 0; first < treeSlots[k]; first += REFIT_BATCH_BLOCK) p.slotBlocks.push_back({k, first});
    p.totalNodes += (size_t) treeNodes[k]; p.totalSlots += (size_t) treeSlots[k];
  }
  p.totalNodeBlocks = (int) p.nodeBlocks.size(); p.totalSlotBlocks = (int) p.slotBlocks.size();
  return nullptr;
}

} // namespace twk
