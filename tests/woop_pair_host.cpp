// Host build of the product's triangle tests for tests/test_woop_pair_host.py: woopIntersectPair against two woopIntersect
// calls, through the same header the kernels compile (tweeker_raytracer_amd/csrc/trace_device.h) and the stand-ins for device
// intrinsics the oracle's host build uses (oracle/host_kernels_shim.h). Compiled by the test itself.
#include "host_kernels_shim.h"
#include "trace_device.h"

using namespace twk;

// Did the single-precision edge functions of woopIntersect(p0, p1, p2) hit a zero (the double-precision fallback runs)?
static int fallsBack(const WoopConstants& w, const V3& o, const V3& p0, const V3& p1, const V3& p2)
{
  const V3 A = p0 - o, B = p1 - o, C = p2 - o;
  const WoopPermutation f = woopFlags(w.perm);
  float Akx, Aky, Akz, Bkx, Bky, Bkz, Ckx, Cky, Ckz;
  woopPermute(f, A, Akx, Aky, Akz);
  woopPermute(f, B, Bkx, Bky, Bkz);
  woopPermute(f, C, Ckx, Cky, Ckz);
  const float Ax = Akx - w.Sx * Akz, Ay = Aky - w.Sy * Akz;
  const float Bx = Bkx - w.Sx * Bkz, By = Bky - w.Sy * Bkz;
  const float Cx = Ckx - w.Sx * Ckz, Cy = Cky - w.Sy * Ckz;
  const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
  return ((U == 0.0f) | (V == 0.0f) | (W == 0.0f)) ? 1 : 0;
}

extern "C" {

// rays: 7 floats each (o.xyz, d.xyz, tmin); quads: 12 floats each (p0, p1, p2, p3). Per case and triangle (T0 = p0 p1 p2,
// T1 = p2 p3 p0): out*[8 * i + 4 * k ..] = t, beta, gamma, verdict (0 / 1 as a float); fallback[2 * i + k] = 1 when the
// triangle's own single-precision edge functions held a zero.
void woop_pair_cases(const float* rays, const float* quads, unsigned long long n, float* outSingle, float* outPair, int* fallback)
{
  for (unsigned long long i = 0; i < n; ++i)
  {
    const float* r = rays + 7 * i;
    const float* q = quads + 12 * i;
    const V3 o = v3(r[0], r[1], r[2]), d = v3(r[3], r[4], r[5]);
    const float tmin = r[6];
    const V3 p0 = v3(q[0], q[1], q[2]), p1 = v3(q[3], q[4], q[5]), p2 = v3(q[6], q[7], q[8]), p3 = v3(q[9], q[10], q[11]);
    WoopConstants w;
    woopSetup(d, w);
    float* s = outSingle + 8 * i;
    s[3] = woopIntersect(w, o, p0, p1, p2, tmin, s[0], s[1], s[2]) ? 1.0f : 0.0f;
    s[7] = woopIntersect(w, o, p2, p3, p0, tmin, s[4], s[5], s[6]) ? 1.0f : 0.0f;
    WoopPairResult pr;
    woopIntersectPair(w, o, p0, p1, p2, p3, tmin, pr);
    float* p = outPair + 8 * i;
    p[0] = pr.t0; p[1] = pr.beta0; p[2] = pr.gamma0; p[3] = pr.hit0 ? 1.0f : 0.0f;
    p[4] = pr.t1; p[5] = pr.beta1; p[6] = pr.gamma1; p[7] = pr.hit1 ? 1.0f : 0.0f;
    fallback[2 * i] = fallsBack(w, o, p0, p1, p2);
    fallback[2 * i + 1] = fallsBack(w, o, p2, p3, p0);
  }
}

} // extern "C"
