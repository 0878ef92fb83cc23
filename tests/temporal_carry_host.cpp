// A stand-alone program for tests/test_temporal_carry_host.py: the host form of the previous-position plane
// (csrc/temporal_carry_device.h previousPositionsHost — the code twk_previous_positions_host runs after its refusals), compiled by the
// test with -fsanitize=address,undefined and run on one case it writes to a file. Nothing of it is loaded into Python.
//   temporal_carry_host <case file> <result file>
// case:   int32 pixels, numIndices, numPositions, numMotion, numCarry; hits [pixels x 3 float32]; instance, primitive [pixels int32
//         each]; geometry [pixels x 4 float32]; indices [numIndices uint32]; positions [numPositions x 4 float32];
//         motion [numMotion x 16 words]; carry [numCarry x 16 words]
// result: plane [pixels x 4 float32]
#include "temporal_carry_device.h"

#include <cstdio>
#include <cstdlib>

using namespace twk;

template<typename T> static std::vector<T> take(FILE* f, size_t count)
{
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "temporal_carry_host: the case file is short\n"); exit(2); }
  return v;
}

int main(int argc, char** argv)
{
  if (argc != 3) { fprintf(stderr, "usage: temporal_carry_host <case> <result>\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "temporal_carry_host: cannot open %s\n", argv[1]); return 2; }
  const std::vector<int> head = take<int>(in, 5);
  const size_t pixels = (size_t) head[0], numIndices = (size_t) head[1], numPositions = (size_t) head[2], numMotion = (size_t) head[3], numCarry = (size_t) head[4];
  const std::vector<float> hits = take<float>(in, 3 * pixels);
  const std::vector<int> instance = take<int>(in, pixels), primitive = take<int>(in, pixels);
  const std::vector<float> geometry = take<float>(in, 4 * pixels);
  const std::vector<unsigned int> indices = take<unsigned int>(in, numIndices);
  const std::vector<float> positions = take<float>(in, 4 * numPositions);
  const std::vector<TwkInstanceMotion> motion = take<TwkInstanceMotion>(in, numMotion);
  const std::vector<TwkInstanceCarry> carry = take<TwkInstanceCarry>(in, numCarry);
  fclose(in);
  std::vector<float> plane(4 * pixels);
  previousPositionsHost(hits.data(), instance.data(), primitive.data(), geometry.data(), pixels, indices.data(), positions.data(), numPositions, motion.data(),
                        (unsigned int) numMotion, carry.data(), (unsigned int) numCarry, plane.data());
  FILE* out = fopen(argv[2], "wb");
  if (!out || fwrite(plane.data(), sizeof(float), plane.size(), out) != plane.size()) { fprintf(stderr, "temporal_carry_host: cannot write the result\n"); return 2; }
  fclose(out);
  return 0;
}
