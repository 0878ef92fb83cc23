// Stand-alone program: what tests/selective_scenes.py says about LaunchParams' leading fields and the array sizes behind them, and
// the layouts of TwkUpdateInfo / TwkUpdatePlan, printed from the headers themselves ("name value" per line) for
// tests/test_update_plan_host.py to compare with the ctypes mirrors. Host only.
#include "device_types.h"

#include <cstddef>
#include <cstdio>

using namespace twk;

#define FIELD(type, field) std::printf(#type "." #field " %zu\n", offsetof(type, field))

int main()
{
  FIELD(LaunchParams, nodes); FIELD(LaunchParams, topNodes); FIELD(LaunchParams, topNodes7); FIELD(LaunchParams, topRoot); FIELD(LaunchParams, topRoot2);
  FIELD(LaunchParams, wideQ); FIELD(LaunchParams, triangles); FIELD(LaunchParams, shadeTriangles);
  std::printf("NODE_BYTES %zu\nSLOT_BYTES %zu\nSHADE_RECORD_BYTES %zu\nTOP_NODES %d\nTOP_NODES7 %d\nQUANTISED_NODE_BYTES %zu\n", sizeof(BvhNode), 3 * sizeof(float4),
              TWK_SHADE_RECORD * sizeof(float4), TWK_TOP_NODES, TWK_TOP_NODES7, 4 * sizeof(float4));
  std::printf("TwkUpdateInfo.size %zu\n", sizeof(TwkUpdateInfo));
  FIELD(TwkUpdateInfo, selective); FIELD(TwkUpdateInfo, instancesMoved); FIELD(TwkUpdateInfo, treesRebuilt); FIELD(TwkUpdateInfo, topLevelRebuilt);
  FIELD(TwkUpdateInfo, nodesRequantised); FIELD(TwkUpdateInfo, slotsRewritten); FIELD(TwkUpdateInfo, instanceRecordsUploaded); FIELD(TwkUpdateInfo, keptBytes);
  FIELD(TwkUpdateInfo, milliseconds);
  std::printf("TwkUpdatePlan.size %zu\n", sizeof(TwkUpdatePlan));
  FIELD(TwkUpdatePlan, instances); FIELD(TwkUpdatePlan, flattenedInstances); FIELD(TwkUpdatePlan, directLeafInstances); FIELD(TwkUpdatePlan, enteredGeometries);
  FIELD(TwkUpdatePlan, treesRebuilt); FIELD(TwkUpdatePlan, topLevelRebuilt); FIELD(TwkUpdatePlan, numRanges); FIELD(TwkUpdatePlan, tlasBase);
  FIELD(TwkUpdatePlan, nodes); FIELD(TwkUpdatePlan, triangleSlots); FIELD(TwkUpdatePlan, nodesRequantised); FIELD(TwkUpdatePlan, slotsRewritten);
  return 0;
}
