// The refit of one tree on the device (bvh_refit.h is the definition; twk_refit_geometry_vertices, device_scene.hip updateSelective,
// is the caller): four launches on the tree's node and slot ranges, no sort, no topology, no scan.
//   refitSlotsKernel    one thread per slot: the slot and its shading record again, through emitTriangle, from the primitive word it holds
//   refitParentsKernel  one thread per node: the parent of each inner child, from the child references (parents start at -1: a memset);
//                       zeroes the node's ticket
//   refitNodesKernel    one thread per node: the boxes of its leaf children, then bottom-up with refitKernel's ticket scheme
//   refitTermsKernel    one thread per node: the SAH terms, reduced per block in a fixed order; the host adds the blocks by index
// Compulsory bytes per tree of t slots and n used nodes: 3 x 48 t attribute bytes read (through 12 t index bytes), 48 t + 128 t
// written for slots and shading records, 64 n + 128 n for nodes and wide nodes; the node kernel reads each slot once more for the boxes.
#include "bvh_refit.h"
#include "bvh_build.h"

namespace twk {

__global__ void __launch_bounds__(256) refitSlotsKernel(const float* __restrict__ attributes, const unsigned int* __restrict__ indices, const int4* __restrict__ soup,
                                                        const DevInstance* __restrict__ instances, float4* triangles, float4* shadeTriangles, int numSlots)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numSlots) return;
  const unsigned int prim = asUint(triangles[3 * (size_t) s].w);
  if (prim >= (unsigned int) numSlots) return; // the build wrote every primitive of the geometry once: never taken
  emitTriangle(attributes, indices, soup, instances, prim, s, triangles, shadeTriangles);
}

__global__ void __launch_bounds__(256) refitParentsKernel(RefitTree t, int* __restrict__ parents, unsigned int* __restrict__ tickets)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.numNodes) return;
  tickets[i] = 0u;
  int c0, c1;
  refitChildren(t.nodes + i, c0, c1);
  if (refitUnused(c0, c1)) return;
  if (c0 >= 0 && (unsigned int) (c0 - t.nodeBase) < (unsigned int) t.numNodes) parents[c0 - t.nodeBase] = i;
  if (c1 >= 0 && (unsigned int) (c1 - t.nodeBase) < (unsigned int) t.numNodes) parents[c1 - t.nodeBase] = i;
}

// Whether an inner reference stays in the tree (the build's always do; a stray one must not become an address)
TWK_D bool refitInside(const RefitTree& t, int ref) { return (unsigned int) (ref - t.nodeBase) < (unsigned int) t.numNodes; }

// A node is complete once its own thread (the boxes of its leaf children) and the thread that finished each inner child (that child's
// box) have arrived: 1 + inner children arrivals, counted by a ticket. Every arrival is a release — the stores, __threadfence, the
// wait for it, the atomicAdd — and the last arrival an acquire: __threadfence, then plain vector loads of what the others stored
// (none of these pointers is __restrict__: handed-off bytes stay off the scalar path). No thread waits for another; a thread that is
// not the last returns, so no block depends on another being resident.
__global__ void __launch_bounds__(256) refitNodesKernel(RefitTree t, const int* parents, unsigned int* tickets)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.numNodes) return;
  int c0, c1;
  refitChildren(t.nodes + i, c0, c1);
  if (refitUnused(c0, c1)) return;
  if ((c0 >= 0 && !refitInside(t, c0)) || (c1 >= 0 && !refitInside(t, c1))) return;
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

__global__ void __launch_bounds__(256) refitTermsKernel(RefitTree t, const int* __restrict__ parents, double* __restrict__ partials)
{
  __shared__ double sums[2][256];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double inner = 0.0, leaf = 0.0;
  if (i < t.numNodes && (i == 0 || parents[i] >= 0)) refitNodeTerms(t, i, inner, leaf); // the nodes the root reaches
  sums[0][threadIdx.x] = inner; sums[1][threadIdx.x] = leaf;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) // the same pairs in the same order, whatever the scheduling
  {
    if ((int) threadIdx.x < step) { sums[0][threadIdx.x] += sums[0][threadIdx.x + step]; sums[1][threadIdx.x] += sums[1][threadIdx.x + step]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = sums[0][0]; partials[2 * blockIdx.x + 1] = sums[1][0]; }
}

#define REFIT_CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

size_t refitScratchWords(int numNodes) { return 2 * (size_t) numNodes + 4 * (size_t) ((numNodes + 255) / 256) + 16; }

hipError_t launchRefitTree(hipStream_t stream, const float* attributes, const unsigned int* indices, const int4* soup, const DevInstance* instances,
                           BvhNode* nodes, BvhNode* wide, float* nodeCost, float4* triangles, float4* shadeTriangles, const int* pairFlags,
                           int nodeBase, int numNodes, int slotBase, int numSlots, unsigned int* scratch, float rootBounds[6], double terms[2])
{
  RefitTree t;
  t.nodes = nodes + nodeBase; t.wide = wide + 2 * (size_t) nodeBase; t.nodeCost = nodeCost ? nodeCost + nodeBase : nullptr;
  t.triangles = triangles + 3 * (size_t) slotBase; t.pairFlags = pairFlags ? pairFlags + slotBase : nullptr;
  t.nodeBase = nodeBase; t.numNodes = numNodes; t.slotBase = slotBase; t.numSlots = numSlots;
  const int blocks = (numNodes + 255) / 256;
  int* parents = reinterpret_cast<int*>(scratch);
  unsigned int* tickets = scratch + numNodes;
  double* partials = reinterpret_cast<double*>(scratch + ((2 * (size_t) numNodes + 3) & ~(size_t) 3)); // 16-byte aligned
  hipLaunchKernelGGL(refitSlotsKernel, dim3((numSlots + 255) / 256), dim3(256), 0, stream, attributes, indices, soup, instances,
                     triangles + 3 * (size_t) slotBase, shadeTriangles + TWK_SHADE_RECORD * (size_t) slotBase, numSlots);
  REFIT_CHECK(hipMemsetAsync(parents, 0xff, sizeof(int) * (size_t) numNodes, stream)); // -1: no parent
  hipLaunchKernelGGL(refitParentsKernel, dim3(blocks), dim3(256), 0, stream, t, parents, tickets);
  hipLaunchKernelGGL(refitNodesKernel, dim3(blocks), dim3(256), 0, stream, t, parents, tickets);
  hipLaunchKernelGGL(refitTermsKernel, dim3(blocks), dim3(256), 0, stream, t, parents, partials);
  REFIT_CHECK(hipGetLastError());
  BvhNode root;
  std::vector<double> sums(2 * (size_t) blocks);
  REFIT_CHECK(hipMemcpyAsync(&root, t.nodes, sizeof(BvhNode), hipMemcpyDeviceToHost, stream));
  REFIT_CHECK(hipMemcpyAsync(sums.data(), partials, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, stream));
  REFIT_CHECK(hipStreamSynchronize(stream));
  float4 lo, hi;
  refitRootBox(&root, lo, hi);
  rootBounds[0] = lo.x; rootBounds[1] = lo.y; rootBounds[2] = lo.z; rootBounds[3] = hi.x; rootBounds[4] = hi.y; rootBounds[5] = hi.z;
  terms[0] = 0.0; terms[1] = 0.0;
  for (int b = 0; b < blocks; ++b) { terms[0] += sums[2 * (size_t) b]; terms[1] += sums[2 * (size_t) b + 1]; }
  return hipSuccess;
}

} // namespace twk
