// Stand-alone driver of hanabi_sad_amd/csrc/hsad_gemm_plan.h for the CPU suite (tests/test_gemm_plan_cpu.py builds it with
// g++ -fsanitize=address,undefined and compares its output, line for line, with the Python restatement in tests/gemm_group.py).
// usage: gemm_plan_main <j_max> <split_max>.  For every K = 128 j, j = 1 .. j_max, and split_k = 1 .. split_max one line:
//   plan K split_k | core chunk count last | plain chunk count last | handed chunk count last | floats F
// core: the grouped launch's plan; plain: gemm_launch's own split for that split_k; handed: what the 128 x 128 kernel cuts when the grouped
// entry point's fallback hands it the core plan's range length; F: group_item_floats of an item M = 256 (1 + j % 3), N = 4 (1 + (j + split_k) % 7).
// Then the items the entry point refuses (0 floats), and OK.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "hsad_gemm_plan.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int j_max = std::atoi(argv[1]), split_max = std::atoi(argv[2]);
  using namespace hsad_gemm_plan;
  for (int j = 1; j <= j_max; ++j)
    for (int s = 1; s <= split_max; ++s) {
      const int K = 128 * j;
      const KPlan c = core_plan(K, s), p = plain_plan(K, s), h = plan_with_chunk(K, c.chunk);
      const int M = 256 * (1 + j % 3), N = 4 * (1 + (j + s) % 7);
      std::printf("plan %d %d | core %d %d %d | plain %d %d %d | handed %d %d %d | floats %" PRId64 "\n", K, s, c.chunk, c.count, c.last, p.chunk,
                  p.count, p.last, h.chunk, h.count, h.last, group_item_floats(M, N, K, s));
    }
  std::printf("refused %" PRId64 " %" PRId64 " %" PRId64 "\n", group_item_floats(256, 64, 64, 1), group_item_floats(256, 64, 256, 0),
              group_item_floats(256, 64, 0, 4));
  std::printf("OK\n");
  return 0;
}
