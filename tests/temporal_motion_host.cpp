// A stand-alone program for tests/test_temporal_motion_host.py: the host forms of the temporal merges with a motion table
// (csrc/temporal_motion_host.h — the code twk_temporal_moving_host and twk_temporal_cascade_moving_host run after their refusals) and
// twk_instance_motion's body (csrc/temporal_motion_device.h instanceMotion), compiled by the test with -fsanitize=address,undefined
// and run on one case it writes to a file. Nothing of it is loaded into Python.
//   temporal_motion_host <case file> <result file>
// case:   int32 width, height, K, numMotion, maxHistory, radius, minTaps, pairs; float32 tolerance, gamma, start, base; camera[12];
//         colour, moments, geometry, history colour, moments, geometry [n x 4 each]; layers, history layers [K x n x 4 each];
//         trust [n]; table [numMotion x 16 words]; previous, current [pairs x 12 each]
// result: plain colour, moments [n x 4 each]; rectified colour, moments [n x 4 each], trust [n]; cascade layers, trusted cascade
//         layers [K x n x 4 each]; records [pairs x 16 words], refused [pairs int32]
#include "temporal_motion_host.h"

#include <cstdio>
#include <cstdlib>

using namespace twk;

template<typename T> static std::vector<T> take(FILE* f, size_t count)
{
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "temporal_motion_host: the case file is short\n"); exit(2); }
  return v;
}

template<typename T> static void put(FILE* f, const std::vector<T>& v)
{
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "temporal_motion_host: cannot write the result\n"); exit(2); }
}

int main(int argc, char** argv)
{
  if (argc != 3) { fprintf(stderr, "usage: temporal_motion_host <case> <result>\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "temporal_motion_host: cannot open %s\n", argv[1]); return 2; }
  const std::vector<int> head = take<int>(in, 8);
  const int width = head[0], height = head[1], K = head[2], numMotion = head[3], maxHistory = head[4], radius = head[5], minTaps = head[6], pairs = head[7];
  const std::vector<float> real = take<float>(in, 4);
  const std::vector<float> camera = take<float>(in, 12);
  const size_t n = (size_t) width * height, all = n * (size_t) K;
  const std::vector<float> colour = take<float>(in, 4 * n), moments = take<float>(in, 4 * n), geometry = take<float>(in, 4 * n);
  const std::vector<float> hColour = take<float>(in, 4 * n), hMoments = take<float>(in, 4 * n), hGeometry = take<float>(in, 4 * n);
  const std::vector<float> layers = take<float>(in, 4 * all), hLayers = take<float>(in, 4 * all), trust = take<float>(in, n);
  const std::vector<TwkInstanceMotion> table = take<TwkInstanceMotion>(in, (size_t) numMotion);
  const std::vector<float> previous = take<float>(in, 12 * (size_t) pairs), current = take<float>(in, 12 * (size_t) pairs);
  fclose(in);

  TemporalConstants k;
  memset(&k, 0, sizeof(k));
  k.width = width; k.height = height; k.hasHistory = 1; k.maxHistory = (float) maxHistory; k.tol2 = real[0] * real[0];
  if (!temporalCamera(camera.data(), k)) { fprintf(stderr, "temporal_motion_host: a degenerate camera\n"); return 2; }
  RectifyConstants r;
  r.radius = radius; r.minTaps = minTaps; r.gamma2 = real[1] * real[1];
  TwkCascade cascade; cascade.layers = K; cascade.start = real[2]; cascade.base = real[3];
  CascadeConstants c;
  if (const char* why = cascadeConstants(cascade, c)) { fprintf(stderr, "temporal_motion_host: %s\n", why); return 2; }

  const TemporalHostFrame frame(n, colour.data(), moments.data(), geometry.data(), hColour.data(), hMoments.data(), hGeometry.data());
  std::vector<float> plainColour(4 * n), plainMoments(4 * n), rectColour(4 * n), rectMoments(4 * n), rectTrust(n), merged(4 * all), mergedTrusted(4 * all);
  temporalMergeHost(k, nullptr, frame, table.data(), (unsigned int) numMotion, plainColour.data(), plainMoments.data(), nullptr);
  temporalMergeHost(k, &r, frame, table.data(), (unsigned int) numMotion, rectColour.data(), rectMoments.data(), rectTrust.data());
  temporalCascadeHostLayers(k, c, layers.data(), geometry.data(), hLayers.data(), hGeometry.data(), nullptr, table.data(), (unsigned int) numMotion, merged.data());
  temporalCascadeHostLayers(k, c, layers.data(), geometry.data(), hLayers.data(), hGeometry.data(), trust.data(), table.data(), (unsigned int) numMotion, mergedTrusted.data());
  std::vector<TwkInstanceMotion> records((size_t) pairs);
  std::vector<int> refused((size_t) pairs, 0);
  for (int i = 0; i < pairs; ++i)
    if (!instanceMotion(&previous[12 * (size_t) i], &current[12 * (size_t) i], records[(size_t) i])) { refused[(size_t) i] = 1; memset(&records[(size_t) i], 0, sizeof(TwkInstanceMotion)); }

  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "temporal_motion_host: cannot open %s\n", argv[2]); return 2; }
  put(out, plainColour); put(out, plainMoments); put(out, rectColour); put(out, rectMoments); put(out, rectTrust); put(out, merged); put(out, mergedTrusted);
  put(out, records); put(out, refused);
  if (fclose(out) != 0) return 2;
  return 0;
}
