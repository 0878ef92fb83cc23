// The two pixel formats of the output, AOV and denoised buffers (twk_set_output_format): float4, and Optix7Gui's RGBA16F
// (USE_FP32_OUTPUT 0, app_config.h:57-59; Half4 of half_common.h:36-80).
#pragma once
#include "device_math.h"

namespace twk {

// alignas(8): one global_load_dwordx2 / global_store_dwordx2 per pixel (a plain struct of four _Float16 loads as a ushort plus a dword).
struct alignas(8) Half4 { _Float16 x, y, z, w; };
static_assert(sizeof(Half4) == 8, "RGBA16F pixel");

TWK_HD float4 widen(const Half4 h) { return make_float4((float) h.x, (float) h.y, (float) h.z, (float) h.w); } // exact
// f32 -> f16 round to nearest even (v_cvt_f16_f32 = __float2half; NOT v_cvt_pkrtz_f16_f32, which rounds toward zero):
// half subnormals are kept (the code object's float_denorm_mode_16_64 is 3), what exceeds 65504 rounds to +-inf.
TWK_HD Half4 narrow(const float4 v)
{
  Half4 h;
  h.x = (_Float16) v.x; h.y = (_Float16) v.y; h.z = (_Float16) v.z; h.w = (_Float16) v.w;
  return h;
}
// device_math.h pixelOf / widen say the same for float4: kernels that serve both formats are templates over the pixel type
template<> TWK_HD Half4 pixelOf<Half4>(const float4 v) { return narrow(v); }

} // namespace twk
