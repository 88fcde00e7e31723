// Stand-alone harness for hanabi_sad_amd/csrc/hsad_behaviour.h (tests/test_behaviour_cpu.py builds it with the sanitizers).
// stdin: "P H colors ranks max_info max_life shuffle_color n", then n records of 80 + 6 P H + 10 P ints, each followed by the uid
// the seat on turn is about to play.
// stdout: per record "seat" and the HSAD_BH_NSTAT increments bh_classify gives.
#include <cstdio>
#include <vector>

#include "hsad_behaviour.h"
#include "hsad_position.h"

static uint64_t deck_bits(int C, int R) {
  uint64_t d = 0;
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < R; ++r) d |= (uint64_t)(r == 0 ? 3 : (r == R - 1 ? 1 : 2)) << (2 * (c * 5 + r));
  return d;
}

struct Words {
  const std::vector<uint32_t>* w;
  uint32_t operator()(int pl) const { return w->at((size_t)pl); }   // a plane outside the game's is the harness's to find
};

int main() {
  PosRules r;
  int n = 0;
  if (scanf("%d %d %d %d %d %d %d %d", &r.P, &r.H, &r.nC, &r.nR, &r.max_info, &r.max_life, &r.shuffle_color, &n) != 8) return 2;
  if (r.P < 2 || r.P > POS_MAX_PLAYERS || r.H < 1 || r.H > 5) return 2;
  r.max_len = 0;
  r.deck_full = deck_bits(r.nC, r.nR);
  const RbRules ru = {r.P, r.H, r.nC, r.nR, r.max_info, 2 * r.H + (r.P - 1) * (r.nC + r.nR) + 1, r.shuffle_color, r.deck_full};
  const int words = 80 + 6 * r.P * r.H + 10 * r.P;
  std::vector<int32_t> rec(words);
  std::vector<uint32_t> w(PL_FIXED + 6 * r.P), before;
  for (int k = 0; k < n; ++k) {
    for (int i = 0; i < words; ++i)
      if (scanf("%d", &rec[i]) != 1) return 2;
    long long uid = 0;
    if (scanf("%lld", &uid) != 1) return 2;
    for (auto& x : w) x = 0u;
    if (pos_decode_record(rec.data(), r, w.data()) & (HSAD_POS_FIELD | HSAD_POS_HANDS)) return 3;
    before = w;
    const int p = rec[57];
    const Words acc = {&w};
    const bh_inc inc = bh_classify(acc, ru, p, (int64_t)uid);
    if (w != before) return 4;   // the position is only read
    printf("%d", p);
    for (int q = 0; q < HSAD_BH_NSTAT; ++q) printf(" %d", bh_get(inc, q));
    printf("\n");
  }
  return 0;
}
