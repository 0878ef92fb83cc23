// Host build of the product's triangle tests for tests/test_triangle_exact_host.py: woopIntersect and woopIntersectPair through the
// same header the kernels compile (tweeker_raytracer_amd/csrc/trace_device.h) and the stand-ins for device intrinsics the oracle's
// host build uses (oracle/host_kernels_shim.h), and beside them the paper's form of the test (Woop, Benthin, Wald, JCGT 2013) with
// its exchange of kx and ky for d[kz] < 0, as oracle/orc_trace.h states it. Compiled by the test itself.
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

// The paper's form: integer axis indices, kx and ky exchanged when d[kz] < 0, early returns.
static bool paperIntersect(const float* o, const float* d, const float* v0, const float* v1, const float* v2, float tmin,
                           float& t, float& beta, float& gamma)
{
  const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
  int kz = (ax > ay) ? ((ax > az) ? 0 : 2) : ((ay > az) ? 1 : 2);
  int kx = (kz == 2) ? 0 : kz + 1;
  int ky = (kx == 2) ? 0 : kx + 1;
  if (d[kz] < 0.0f) { const int s = kx; kx = ky; ky = s; }
  const float Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1.0f / d[kz];

  const float Akx = v0[kx] - o[kx], Aky = v0[ky] - o[ky], Akz = v0[kz] - o[kz];
  const float Bkx = v1[kx] - o[kx], Bky = v1[ky] - o[ky], Bkz = v1[kz] - o[kz];
  const float Ckx = v2[kx] - o[kx], Cky = v2[ky] - o[ky], Ckz = v2[kz] - o[kz];

  const float Ax = Akx - Sx * Akz, Ay = Aky - Sy * Akz;
  const float Bx = Bkx - Sx * Bkz, By = Bky - Sy * Bkz;
  const float Cx = Ckx - Sx * Ckz, Cy = Cky - Sy * Ckz;

  float U = Cx * By - Cy * Bx;
  float V = Ax * Cy - Ay * Cx;
  float W = Bx * Ay - By * Ax;
  if (U == 0.0f || V == 0.0f || W == 0.0f)
  {
    const double CxBy = (double) Cx * (double) By, CyBx = (double) Cy * (double) Bx;
    U = (float) (CxBy - CyBx);
    const double AxCy = (double) Ax * (double) Cy, AyCx = (double) Ay * (double) Cx;
    V = (float) (AxCy - AyCx);
    const double BxAy = (double) Bx * (double) Ay, ByAx = (double) By * (double) Ax;
    W = (float) (BxAy - ByAx);
  }
  if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
  const float det = U + V + W;
  if (det == 0.0f) return false;
  const float Az = Sz * Akz, Bz = Sz * Bkz, Cz = Sz * Ckz;
  const float T = U * Az + V * Bz + W * Cz;
  const float rcpDet = 1.0f / det;
  const float tt = T * rcpDet;
  if (!(tt > tmin)) return false;
  t = tt; beta = V * rcpDet; gamma = W * rcpDet;
  return true;
}

extern "C" {

// rays: 7 floats each (o.xyz, d.xyz, tmin); tris: 9 floats each. out[4 * i ..] = t, beta, gamma, verdict (0 / 1 as a float) of
// woopIntersect; fallback[i] = 1 when its single-precision edge functions held a zero.
void triangle_exact_single(const float* rays, const float* tris, unsigned long long n, float* out, int* fallback)
{
  for (unsigned long long i = 0; i < n; ++i)
  {
    const float* r = rays + 7 * i;
    const float* q = tris + 9 * i;
    const V3 o = v3(r[0], r[1], r[2]), d = v3(r[3], r[4], r[5]);
    const V3 p0 = v3(q[0], q[1], q[2]), p1 = v3(q[3], q[4], q[5]), p2 = v3(q[6], q[7], q[8]);
    WoopConstants w;
    woopSetup(d, w);
    float* s = out + 4 * i;
    s[3] = woopIntersect(w, o, p0, p1, p2, r[6], s[0], s[1], s[2]) ? 1.0f : 0.0f;
    fallback[i] = fallsBack(w, o, p0, p1, p2);
  }
}

// The same cases through the paper's form. A miss leaves t, beta, gamma zero.
void triangle_exact_paper(const float* rays, const float* tris, unsigned long long n, float* out)
{
  for (unsigned long long i = 0; i < n; ++i)
  {
    const float* r = rays + 7 * i;
    const float* q = tris + 9 * i;
    float* s = out + 4 * i;
    s[0] = s[1] = s[2] = 0.0f;
    s[3] = paperIntersect(r, r + 3, q, q + 3, q + 6, r[6], s[0], s[1], s[2]) ? 1.0f : 0.0f;
  }
}

// quads: 12 floats each (p0, p1, p2, p3); out[8 * i + 4 * k ..] = t, beta, gamma, verdict of T0 = (p0 p1 p2) and T1 = (p2 p3 p0)
// from woopIntersectPair.
void triangle_exact_pair(const float* rays, const float* quads, unsigned long long n, float* out)
{
  for (unsigned long long i = 0; i < n; ++i)
  {
    const float* r = rays + 7 * i;
    const float* q = quads + 12 * i;
    const V3 o = v3(r[0], r[1], r[2]), d = v3(r[3], r[4], r[5]);
    const V3 p0 = v3(q[0], q[1], q[2]), p1 = v3(q[3], q[4], q[5]), p2 = v3(q[6], q[7], q[8]), p3 = v3(q[9], q[10], q[11]);
    WoopConstants w;
    woopSetup(d, w);
    WoopPairResult pr;
    woopIntersectPair(w, o, p0, p1, p2, p3, r[6], pr);
    float* p = out + 8 * i;
    p[0] = pr.t0; p[1] = pr.beta0; p[2] = pr.gamma0; p[3] = pr.hit0 ? 1.0f : 0.0f;
    p[4] = pr.t1; p[5] = pr.beta1; p[6] = pr.gamma1; p[7] = pr.hit1 ? 1.0f : 0.0f;
  }
}

} // extern "C"
