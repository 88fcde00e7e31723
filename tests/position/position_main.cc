// Stand-alone harness for hanabi_sad_amd/csrc/hsad_position.h (tests/test_position_cpu.py builds it with the sanitizers).
// stdin: "P H colors ranks max_info max_life max_len shuffle_color n", then n records of 80 + 6 P H + 10 P ints.
// stdout: per record the flags hsad_env_import_state would report for it: the decoder's, then position_valid's.
#include <cstdio>
#include <vector>

#include "hsad_position.h"

static uint64_t deck_bits(int C, int R) {
  uint64_t d = 0;
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < R; ++r) d |= (uint64_t)(r == 0 ? 3 : (r == R - 1 ? 1 : 2)) << (2 * (c * 5 + r));
  return d;
}

int main() {
  PosRules r;
  int n = 0;
  if (scanf("%d %d %d %d %d %d %d %d %d", &r.P, &r.H, &r.nC, &r.nR, &r.max_info, &r.max_life, &r.max_len, &r.shuffle_color, &n) != 9) return 2;
  if (r.P < 2 || r.P > POS_MAX_PLAYERS || r.H < 1 || r.H > 5) return 2;
  r.deck_full = deck_bits(r.nC, r.nR);
  const int words = 80 + 6 * r.P * r.H + 10 * r.P;
  std::vector<int32_t> rec(words);            // exactly the record: a read past it is the sanitizer's to find
  std::vector<uint32_t> w(PL_FIXED + 6 * r.P);
  for (int k = 0; k < n; ++k) {
    for (int i = 0; i < words; ++i)
      if (scanf("%d", &rec[i]) != 1) return 2;
    for (auto& x : w) x = 0u;
    uint32_t f = pos_decode_record(rec.data(), r, w.data());
    if (!(f & (HSAD_POS_FIELD | HSAD_POS_HANDS))) f |= position_valid(w.data(), r);
    printf("%u\n", f);
  }
  return 0;
}
