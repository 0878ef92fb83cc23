// A stand-alone program for tests/test_vertex_frames_host.py: the host form of a positions-mode device source's frames (csrc/
// vertex_source_device.h vertexAdjacency and vertexFramesHost — the code twk_vertex_frames_host runs after the refusals of its
// arguments), compiled by the test with -fsanitize=address,undefined and run on the cases it writes to a file. Nothing of it is
// loaded into Python.
//   vertex_source_host <case file> <result file>
// case:   int32 numVertices, numIndices; positions [numVertices x 3 float32]; indices [numIndices uint32]; records before
//         [numVertices x 12 float32]
// result: records after [numVertices x 12 float32]
#include "vertex_source_device.h"

#include <cstdio>
#include <cstdlib>

using namespace twk;

template<typename T> static std::vector<T> take(FILE* f, size_t count)
{
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "vertex_source_host: the case file is short\n"); exit(2); }
  return v;
}

int main(int argc, char** argv)
{
  if (argc != 3) { fprintf(stderr, "usage: vertex_source_host <case> <result>\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "vertex_source_host: cannot open %s\n", argv[1]); return 2; }
  const std::vector<int> head = take<int>(in, 2);
  const size_t numVertices = (size_t) head[0], numIndices = (size_t) head[1];
  const std::vector<float> positions = take<float>(in, 3 * numVertices);
  const std::vector<unsigned int> indices = take<unsigned int>(in, numIndices);
  const std::vector<float> before = take<float>(in, 12 * numVertices);
  fclose(in);
  for (unsigned int i : indices) if (i >= numVertices) { fprintf(stderr, "vertex_source_host: an index is beyond the vertices\n"); return 3; }

  std::vector<float> after(12 * numVertices);
  vertexFramesHost(positions.data(), numVertices, indices.data(), numIndices, before.data(), after.data());

  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "vertex_source_host: cannot write %s\n", argv[2]); return 2; }
  if (fwrite(after.data(), sizeof(float), after.size(), out) != after.size()) { fprintf(stderr, "vertex_source_host: cannot write the result\n"); return 2; }
  fclose(out);
  return 0;
}
