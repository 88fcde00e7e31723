// Stand-alone harness for hanabi_sad_amd/csrc/hsad_search_horizon.h (tests/test_search_horizon_cpu.py builds it with
// g++ -fsanitize=address,undefined and holds its output to the numpy restatement tests/search_horizon_ref.py, word for word).
// argv[1]: a binary file, little endian: int32 n, then n cases of { uint32 misc, uint32 board, int32 P, int32 perfect_score,
// int32 mode, float q[5] } -- the two status words of a slot as hsad_planes.h lays them out and the Q of its seats' rows.
// stdout: per case "v counted cut nonfinite", then "OK".
#include <cstdio>
#include <cstring>
#include <vector>

#include "hsad_search_horizon.h"

struct Case {
  uint32_t misc, board;
  int32_t P, perfect, mode;
  float q[5];
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 2;
  std::vector<Case> cases((size_t)n);
  if (n && fread(cases.data(), sizeof(Case), (size_t)n, f) != (size_t)n) return 2;
  fclose(f);
  for (const Case& c : cases) {
    if (c.P < 1 || c.P > 5) return 3;
    // exactly P values, so that a read past the seats of the game is the sanitizer's to find
    std::vector<float> row(c.q, c.q + c.P);
    const float* r = row.data();
    const ShValue s = sh_slot(c.misc, c.board, c.P, c.perfect, c.mode, [r](int p) { return r[p]; });
    printf("%d %d %d %d\n", (int)s.v, s.counted, s.cut, s.nonfinite);
  }
  printf("OK\n");
  return 0;
}
