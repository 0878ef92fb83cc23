// A stand-alone program for tests/test_light_motion_host.py: the rule that moves a light with its emitter (csrc/light_motion.h — the
// code twk_light_moved_host and the transform calls run after their own refusals), compiled with -fsanitize=address,undefined.
//   light_motion_host <case file> <result file>
// case:   int32 count; count TwkLightDefinition (80 B each); count anchor transforms (12 floats each); count transforms
// result: count TwkLightDefinition (zero bytes where refused); count int32 (0: moved, 1: refused)
#include "light_motion.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace twk;

template<typename T> static std::vector<T> readArray(FILE* f, size_t count)
{
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "light_motion_host: the case file is short\n"); exit(2); }
  return v;
}

template<typename T> static void writeArray(FILE* f, const std::vector<T>& v)
{
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "light_motion_host: cannot write the result\n"); exit(2); }
}

int main(int argc, char** argv)
{
  static_assert(sizeof(TwkLightDefinition) == 80, "LightDefinition is 80 B");
  if (argc != 3) { fprintf(stderr, "usage: light_motion_host <case> <result>\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "light_motion_host: cannot open %s\n", argv[1]); return 2; }
  const int32_t count = readArray<int32_t>(in, 1)[0];
  if (count < 0 || count > (1 << 20)) { fprintf(stderr, "light_motion_host: bad count\n"); return 2; }
  const std::vector<TwkLightDefinition> anchors = readArray<TwkLightDefinition>(in, (size_t) count);
  const std::vector<float> anchorTransforms = readArray<float>(in, 12 * (size_t) count), transforms = readArray<float>(in, 12 * (size_t) count);
  fclose(in);

  std::vector<TwkLightDefinition> moved((size_t) count);
  std::vector<int32_t> refused((size_t) count, 0);
  for (size_t k = 0; k < (size_t) count; ++k)
  {
    memset(&moved[k], 0, sizeof(TwkLightDefinition));
    refused[k] = lightMoved(anchors[k], &anchorTransforms[12 * k], &transforms[12 * k], moved[k]) ? 1 : 0;
  }

  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "light_motion_host: cannot open %s\n", argv[2]); return 2; }
  writeArray(out, moved);
  writeArray(out, refused);
  fclose(out);
  return 0;
}
