// The batch of a twk_refit_scene call (bvh_refit_scene.hip): trees of mixed kinds (refit_scene_plan.h) refit by one launch sequence
// and one host wait. The parents, nodes and terms kernels are bvh_refit_batch.hip's, declared here and launched as they are: they do
// not care what kind of tree they work on.
#pragma once
#include "bvh_refit.h"
#include "refit_scene_plan.h"

namespace twk {

// bvh_refit_batch.hip
__global__ void refitBatchParentsKernel(const RefitBatchTree* __restrict__ trees, const RefitBatchBlock* __restrict__ blocks, int* __restrict__ allParents,
                                        unsigned int* __restrict__ allTickets);
__global__ void refitBatchNodesKernel(const RefitBatchTree* __restrict__ trees, const RefitBatchBlock* __restrict__ blocks, const int* allParents, unsigned int* allTickets);
__global__ void refitBatchTermsKernel(const RefitBatchTree* __restrict__ trees, const RefitBatchBlock* __restrict__ blocks, const int* __restrict__ allParents,
                                      double* __restrict__ partials, float* __restrict__ rootBoxes);

// The refit of the plan's trees in place: ONE upload (tree table, kind table, block tables), the slots launch (refitSceneSlotsKernel:
// every slot again by its tree's kind, the descriptor made in registers — no soup array is read or written), one memset, the three
// launches above, one read-back and one wait, whatever the number and the kinds of the trees. kinds[k]: tree k's record, with the
// bases of ITS handle. All arrays are the scene's (absolute indices); nodeCost / pairFlags nullptr: the scene has none. scratch:
// refitSceneScratchWords(plan) words. rootBounds[6 k ..] receives tree k's box, terms[2 k ..] its SAH terms, bit-equal to what
// launchRefitTree returns for the tree alone.
size_t refitSceneScratchWords(const RefitScenePlan& plan);
hipError_t launchRefitSceneTrees(hipStream_t stream, const float* attributes, const unsigned int* indices, const DevInstance* instances, BvhNode* nodes, BvhNode* wide,
                                 float* nodeCost, float4* triangles, float4* shadeTriangles, const int* pairFlags, const RefitScenePlan& plan, const RefitSceneKind* kinds,
                                 unsigned int* scratch, float* rootBounds, double* terms);

} // namespace twk
