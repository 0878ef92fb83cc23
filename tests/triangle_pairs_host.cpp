// Stand-alone program: bvh_build.h trianglePairs on index lists read from standard input, for tests/test_bvh_audit_host.py to compare
// with bvh_reference.build_primitives. Input: per list "t" and then 3 t indices; output per list one line: the number of pairs, then
// per build primitive its first triangle and 1 for a pair (the sign bit of primFirst), 0 for a single triangle. Host only.
#include "bvh_build.h"

#include <cstdio>
#include <vector>

int main()
{
  int t;
  while (std::scanf("%d", &t) == 1)
  {
    std::vector<unsigned int> indices(3 * (size_t) t);
    for (unsigned int& i : indices) if (std::scanf("%u", &i) != 1) return 1;
    std::vector<int> primFirst;
    const size_t pairs = twk::trianglePairs(indices.data(), t, primFirst);
    std::printf("%zu", pairs);
    for (int p : primFirst) std::printf(" %d %d", p & 0x7fffffff, p < 0 ? 1 : 0);
    std::printf("\n");
  }
  return 0;
}
