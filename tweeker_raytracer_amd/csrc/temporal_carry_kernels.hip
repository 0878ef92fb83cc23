// Kernel of twk_render_geometry_motion: the geometry AOV and, beside it, the previous-position plane defined in temporal_carry_device.h.
#include "temporal_carry_device.h"
#include "temporal_device.h" // centreRay
#include "trace_device.h"

namespace twk {

// geometryKernel<false> (temporal_kernels.hip) with one more stream: the same ray through the centre of every pixel with the same
// single-ray traversal, the same element of the geometry AOV, and the plane's element from the hit's instance, primitive and
// barycentrics (previousPosition) — per hit pixel two 64-byte records, and on a deformed geometry three index words and three 16-byte
// previous positions. A kernel of its own, so that geometryKernel is the code it was.
__global__ void __launch_bounds__(TWK_TRACE_BLOCK)
geometryMotionKernel(LaunchParams p, float4* __restrict__ geometry, float4* __restrict__ plane, const TwkInstanceMotion* __restrict__ motion, unsigned int numMotion,
                     const TwkInstanceCarry* __restrict__ carry, unsigned int numCarry, const float4* __restrict__ previousPositions)
{
  __shared__ int stackStorage[TWK_TRACE_STACK_LDS * TWK_TRACE_BLOCK];
  int* ldsStack = stackStorage + threadIdx.x;
  int* spill = p.traceStackSpill + (size_t) (blockIdx.x * blockDim.x + threadIdx.x) * TWK_TRACE_STACK_SPILL;
  unsigned int n0 = 0, n1 = 0, n2 = 0;
  const unsigned int columns = (unsigned int) p.resolution[0];
  const unsigned int numPixels = columns * (unsigned int) p.resolution[1];
  const float* cam = p.camera;
  const V3 P = v3(cam[0], cam[1], cam[2]);
  for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < numPixels; i += gridDim.x * blockDim.x)
  {
    const int x = (int) (i % columns);
    const int y = (int) (i / columns);
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = g;
    const V3 d = centreRay(cam, x, y, p.resolution[0], p.resolution[1]);
    TraceResult res;
    traverse<false>(p, P, d, p.sceneEpsilon, RT_DEFAULT_MAX, false, ldsStack, spill, res, n0, n1, n2);
    if (res.instance >= 0)
    {
      g = make_float4(P.x + res.t * d.x, P.y + res.t * d.y, P.z + res.t * d.z, __uint_as_float((unsigned int) res.instance + 1u));
      gp = previousPosition(motion, numMotion, carry, numCarry, p.indices, previousPositions, res.instance, res.primitive, res.beta, res.gamma, g);
    }
    geometry[i] = g;
    plane[i] = gp;
  }
}

void launchGeometryMotion(const LaunchParams& p, float4* geometry, float4* plane, const TwkInstanceMotion* motion, unsigned int numMotion, const TwkInstanceCarry* carry,
                          unsigned int numCarry, const float4* previousPositions, int gridBlocks, hipStream_t stream)
{
  hipLaunchKernelGGL(geometryMotionKernel, dim3(gridBlocks), dim3(TWK_TRACE_BLOCK), 0, stream, p, geometry, plane, motion, numMotion, carry, numCarry, previousPositions);
}

} // namespace twk
