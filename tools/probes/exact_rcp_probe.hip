// Which fma refinement of v_rcp_f32 equals the compiler's correctly rounded 1.0f / x, over ALL 2^32 bit patterns, and whether the
// classical quotient correction on top of a correctly rounded reciprocal equals x / d (seeded pairs, |x| <= |d|). Reported per
// variant: mismatches inside the normal domain (2^-126 <= |x| <= 2^126: neither x nor 1 / x denormal), how many of them have an
// all-ones significand, and the first few. What trace_device.h exactReciprocal / woopSetup rest on (profiles/r25_exact_division.md).
// Build: hipcc -O3 -ffp-contract=off --offload-arch=gfx950 -o exact_rcp_probe exact_rcp_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

template<int V> __device__ float refined(float x)
{
  float r = __builtin_amdgcn_rcpf(x);
  for (int k = 0; k < V; ++k)
  {
    const float e = __builtin_fmaf(-x, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
  }
  return r;
}

struct Tally { unsigned long long mismatches, allOnes, outside; unsigned int first[16]; };

template<int V> __global__ void __launch_bounds__(256) sweep(Tally* tally)
{
  const unsigned int base = (blockIdx.x * 256u + threadIdx.x) << 8;
  for (unsigned int k = 0; k < 256u; ++k)
  {
    const unsigned int bits = base + k;
    const float x = __uint_as_float(bits);
    const float ax = fabsf(x);
    if (!((ax >= 0x1p-126f) & (ax <= 0x1p126f))) { if (V == 0) atomicAdd(&tally->outside, 1ull); continue; }
    const float want = 1.0f / x, got = refined<V>(x);
    if (__float_as_uint(want) != __float_as_uint(got))
    {
      const unsigned long long n = atomicAdd(&tally->mismatches, 1ull);
      if ((bits & 0x7fffffu) == 0x7fffffu) atomicAdd(&tally->allOnes, 1ull);
      if (n < 16ull) tally->first[n] = bits;
    }
  }
}

// The binades above 2^126, where 1 / x is a denormal: one refinement is NOT exact there (v_rcp_f32 flushes the denormal result:
// all but two of the 2^25 patterns miss), so "x is normal" is no range check; the flushed values make the residual e = 1, which
// is what exactReciprocal's one compare on |e| catches.
__global__ void __launch_bounds__(256) sweepDenormalResults(Tally* tally)
{
  const unsigned int k = blockIdx.x * 256u + threadIdx.x; // 2^24 patterns per sign: exponent fields 253 and 254
  for (unsigned int sign = 0u; sign < 2u; ++sign)
  {
    const unsigned int bits = (sign << 31) | (0x7e800000u + k);
    const float x = __uint_as_float(bits);
    const float want = 1.0f / x, got = refined<1>(x);
    if (__float_as_uint(want) != __float_as_uint(got))
    {
      const unsigned long long n = atomicAdd(&tally->mismatches, 1ull);
      if (n < 16ull) tally->first[n] = bits;
    }
  }
}

__device__ unsigned int mix(unsigned int h) { h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16; return h; }

// x / d from the correctly rounded reciprocal: q = x r, e = fma(-d, q, x), q' = fma(e, r, q).
// The denominator's exponent field runs over [loExp, hiExp], the numerator's lies 0..spread below it.
__global__ void __launch_bounds__(256) quotients(Tally* tally, unsigned int seed, int loExp, int hiExp, int spread, int perThread)
{
  unsigned int h = mix((blockIdx.x * 256u + threadIdx.x) ^ mix(seed));
  for (int k = 0; k < perThread; ++k)
  {
    const unsigned int a = h = mix(h + 0x9e3779b9u), b = h = mix(h + 0x9e3779b9u), c = h = mix(h + 0x9e3779b9u);
    const int ed = loExp + (int) (c % (unsigned int) (hiExp - loExp + 1));
    int ex = ed - (int) ((c >> 16) % (unsigned int) (spread + 1)); if (ex < 0) ex = 0;
    float d = __uint_as_float((a & 0x807fffffu) | ((unsigned int) ed << 23));
    float x = __uint_as_float((b & 0x807fffffu) | ((unsigned int) ex << 23));
    if (fabsf(x) > fabsf(d)) { const float s = x; x = d; d = s; }
    const float r = 1.0f / d;
    const float q = x * r;
    const float e = __builtin_fmaf(-d, q, x);
    const float got = __builtin_fmaf(e, r, q), want = x / d;
    if (__float_as_uint(want) != __float_as_uint(got))
    {
      const unsigned long long n = atomicAdd(&tally->mismatches, 1ull);
      if ((__float_as_uint(d) & 0x7fffffu) == 0x7fffffu) atomicAdd(&tally->allOnes, 1ull);
      if (n < 8ull) { tally->first[2 * n] = __float_as_uint(x); tally->first[2 * n + 1] = __float_as_uint(d); }
    }
  }
}

#define CHECK(c) do { hipError_t e_ = (c); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

template<int V> int runSweep(Tally* d)
{
  Tally h;
  CHECK(hipMemset(d, 0, sizeof(Tally)));
  sweep<V><<<65536, 256>>>(d);
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(&h, d, sizeof(Tally), hipMemcpyDeviceToHost));
  printf("v_rcp_f32 + %d refinement(s): %llu mismatches in the normal domain, %llu of them with an all-ones significand", V, h.mismatches, h.allOnes);
  if (V == 0) printf(" (%llu patterns outside the domain)", h.outside);
  printf("\n");
  for (unsigned long long k = 0; k < h.mismatches && k < 16ull; ++k) printf("  0x%08x", h.first[k]);
  if (h.mismatches) printf("\n");
  return 0;
}

int runQuotients(Tally* d, int loExp, int hiExp, int spread)
{
  Tally h;
  CHECK(hipMemset(d, 0, sizeof(Tally)));
  quotients<<<4096, 256>>>(d, 0x25u, loExp, hiExp, spread, 96); // 1.0e8 pairs
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(&h, d, sizeof(Tally), hipMemcpyDeviceToHost));
  printf("quotients, exponent field of d in [%d, %d], of x up to %d below: %llu mismatches, %llu with an all-ones d\n", loExp, hiExp, spread, h.mismatches, h.allOnes);
  for (unsigned long long k = 0; k < h.mismatches && k < 8ull; ++k) printf("  x 0x%08x d 0x%08x", h.first[2 * k], h.first[2 * k + 1]);
  if (h.mismatches) printf("\n");
  return 0;
}

int main()
{
  Tally* d;
  CHECK(hipMalloc(&d, sizeof(Tally)));
  if (runSweep<0>(d) || runSweep<1>(d) || runSweep<2>(d)) return 1;
  {
    Tally h;
    CHECK(hipMemset(d, 0, sizeof(Tally)));
    sweepDenormalResults<<<65536, 256>>>(d);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&h, d, sizeof(Tally), hipMemcpyDeviceToHost));
    printf("2^126 < |x| < 2^128 (1 / x denormal), one refinement: %llu mismatches of 33554432\n", h.mismatches);
    for (unsigned long long k = 0; k < h.mismatches && k < 16ull; ++k) printf("  0x%08x", h.first[k]);
    if (h.mismatches) printf("\n");
  }
  if (runQuotients(d, 67, 187, 60) || runQuotients(d, 100, 150, 24) || runQuotients(d, 1, 254, 200)) return 1;
  return 0;
}
