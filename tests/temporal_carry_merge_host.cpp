// A stand-alone program for tests/test_temporal_carry_host.py: the host forms of the temporal merges with a previous-position plane
// (csrc/temporal_motion_host.h — the code twk_temporal_carried_host and twk_temporal_cascade_carried_host run after their refusals:
// the Carried builds of temporalGather, rectifyReproject and temporalCascadePixel), compiled by the test with
// -fsanitize=address,undefined and run on one case it writes to a file. Nothing of it is loaded into Python.
//   temporal_carry_merge_host <case file> <result file>
// case:   int32 width, height, K, maxHistory, radius, minTaps; float32 tolerance, gamma, start, base; camera[12];
//         colour, moments, geometry, history colour, moments, geometry [n x 4 each]; layers, history layers [K x n x 4 each];
//         trust [n]; plane [n x 4]
// result: plain colour, moments [n x 4 each]; rectified colour, moments [n x 4 each], trust [n]; cascade layers, trusted cascade
//         layers [K x n x 4 each]
#include "temporal_motion_host.h"

#include <cstdio>
#include <cstdlib>

using namespace twk;

template<typename T> static std::vector<T> take(FILE* f, size_t count)
{
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "temporal_carry_merge_host: the case file is short\n"); exit(2); }
  return v;
}

template<typename T> static void put(FILE* f, const std::vector<T>& v)
{
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "temporal_carry_merge_host: cannot write the result\n"); exit(2); }
}

int main(int argc, char** argv)
{
  if (argc != 3) { fprintf(stderr, "usage: temporal_carry_merge_host <case> <result>\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "temporal_carry_merge_host: cannot open %s\n", argv[1]); return 2; }
  const std::vector<int> head = take<int>(in, 6);
  const int width = head[0], height = head[1], K = head[2], maxHistory = head[3], radius = head[4], minTaps = head[5];
  const std::vector<float> real = take<float>(in, 4);
  const std::vector<float> camera = take<float>(in, 12);
  const size_t n = (size_t) width * height, all = n * (size_t) K;
  const std::vector<float> colour = take<float>(in, 4 * n), moments = take<float>(in, 4 * n), geometry = take<float>(in, 4 * n);
  const std::vector<float> hColour = take<float>(in, 4 * n), hMoments = take<float>(in, 4 * n), hGeometry = take<float>(in, 4 * n);
  const std::vector<float> layers = take<float>(in, 4 * all), hLayers = take<float>(in, 4 * all), trust = take<float>(in, n);
  const std::vector<float> plane = take<float>(in, 4 * n);
  fclose(in);

  TemporalConstants k;
  memset(&k, 0, sizeof(k));
  k.width = width; k.height = height; k.hasHistory = 1; k.maxHistory = (float) maxHistory; k.tol2 = real[0] * real[0];
  if (!temporalCamera(camera.data(), k)) { fprintf(stderr, "temporal_carry_merge_host: a degenerate camera\n"); return 2; }
  RectifyConstants r;
  r.radius = radius; r.minTaps = minTaps; r.gamma2 = real[1] * real[1];
  TwkCascade cascade; cascade.layers = K; cascade.start = real[2]; cascade.base = real[3];
  CascadeConstants c;
  if (const char* why = cascadeConstants(cascade, c)) { fprintf(stderr, "temporal_carry_merge_host: %s\n", why); return 2; }

  const TemporalHostFrame frame(n, colour.data(), moments.data(), geometry.data(), hColour.data(), hMoments.data(), hGeometry.data());
  std::vector<float> plainColour(4 * n), plainMoments(4 * n), rectColour(4 * n), rectMoments(4 * n), rectTrust(n), merged(4 * all), mergedTrusted(4 * all);
  temporalMergeHost(k, nullptr, frame, nullptr, 0u, plainColour.data(), plainMoments.data(), nullptr, plane.data());
  temporalMergeHost(k, &r, frame, nullptr, 0u, rectColour.data(), rectMoments.data(), rectTrust.data(), plane.data());
  temporalCascadeHostLayers(k, c, layers.data(), geometry.data(), hLayers.data(), hGeometry.data(), nullptr, nullptr, 0u, merged.data(), plane.data());
  temporalCascadeHostLayers(k, c, layers.data(), geometry.data(), hLayers.data(), hGeometry.data(), trust.data(), nullptr, 0u, mergedTrusted.data(), plane.data());

  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "temporal_carry_merge_host: cannot open %s\n", argv[2]); return 2; }
  put(out, plainColour); put(out, plainMoments); put(out, rectColour); put(out, rectMoments); put(out, rectTrust); put(out, merged); put(out, mergedTrusted);
  if (fclose(out) != 0) return 2;
  return 0;
}
