// Stand-alone program: the layouts of the structs a vertex update and the previous-position plane use — TwkUpdateInfo, TwkUpdatePlan,
// TwkInstanceMotion, TwkInstanceCarry, TwkTriangleAttributes — printed from the public header ("name value" per line) for
// tests/test_vertex_update_plan_host.py to compare with the ctypes mirrors. Host only.
#include "tweeker_hip.h"

#include <cstddef>
#include <cstdio>

#define FIELD(type, field) std::printf(#type "." #field " %zu\n", offsetof(type, field))

int main()
{
  std::printf("TwkUpdateInfo.size %zu\n", sizeof(TwkUpdateInfo));
  FIELD(TwkUpdateInfo, selective); FIELD(TwkUpdateInfo, instancesMoved); FIELD(TwkUpdateInfo, treesRebuilt); FIELD(TwkUpdateInfo, topLevelRebuilt);
  FIELD(TwkUpdateInfo, nodesRequantised); FIELD(TwkUpdateInfo, slotsRewritten); FIELD(TwkUpdateInfo, instanceRecordsUploaded); FIELD(TwkUpdateInfo, keptBytes);
  FIELD(TwkUpdateInfo, milliseconds);
  std::printf("TwkUpdatePlan.size %zu\n", sizeof(TwkUpdatePlan));
  FIELD(TwkUpdatePlan, instances); FIELD(TwkUpdatePlan, flattenedInstances); FIELD(TwkUpdatePlan, directLeafInstances); FIELD(TwkUpdatePlan, enteredGeometries);
  FIELD(TwkUpdatePlan, treesRebuilt); FIELD(TwkUpdatePlan, topLevelRebuilt); FIELD(TwkUpdatePlan, numRanges); FIELD(TwkUpdatePlan, tlasBase);
  FIELD(TwkUpdatePlan, nodes); FIELD(TwkUpdatePlan, triangleSlots); FIELD(TwkUpdatePlan, nodesRequantised); FIELD(TwkUpdatePlan, slotsRewritten);
  std::printf("TwkInstanceMotion.size %zu\n", sizeof(TwkInstanceMotion));
  FIELD(TwkInstanceMotion, previousFromCurrent); FIELD(TwkInstanceMotion, moved); FIELD(TwkInstanceMotion, reserved);
  std::printf("TwkInstanceCarry.size %zu\n", sizeof(TwkInstanceCarry));
  FIELD(TwkInstanceCarry, previousObjectToWorld); FIELD(TwkInstanceCarry, deformed); FIELD(TwkInstanceCarry, positionBase); FIELD(TwkInstanceCarry, indexBase);
  FIELD(TwkInstanceCarry, reserved);
  std::printf("TwkTriangleAttributes.size %zu\n", sizeof(TwkTriangleAttributes));
  return 0;
}
