// Stand-alone harness for hanabi_sad_amd/csrc/hsad_rulebot.h (tests/test_rulebot_cpu.py builds it with the sanitizers).
// stdin: "P H colors ranks max_info max_life shuffle_color n_rules seed n", then n_rules pairs "code k", then n records of
// 80 + 6 P H + 10 P ints, each followed by "key counter".
// stdout: first what rb_rules_invalid says of the list; if that is 0, per record "seat uid deciding-rule" for the seat on turn.
#include <cstdio>
#include <vector>

#include "hsad_position.h"
#include "hsad_rulebot.h"

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
  int n = 0, n_rules = 0;
  unsigned long long seed = 0;
  if (scanf("%d %d %d %d %d %d %d %d %llu %d", &r.P, &r.H, &r.nC, &r.nR, &r.max_info, &r.max_life, &r.shuffle_color, &n_rules, &seed, &n) != 10)
    return 2;
  if (r.P < 2 || r.P > POS_MAX_PLAYERS || r.H < 1 || r.H > 5 || n_rules < 0 || n_rules > 64) return 2;
  r.max_len = 0;
  r.deck_full = deck_bits(r.nC, r.nR);
  std::vector<hsad_rule> rules((size_t)n_rules);   // exactly the list
  for (auto& x : rules)
    if (scanf("%d %d", &x.code, &x.k) != 2) return 2;
  const int bad = rb_rules_invalid(rules.data(), n_rules);
  printf("%d\n", bad);
  if (bad) return 0;
  // the list as bot 3 of a table, so that a row offset that is off shows
  const int bot = 3;
  std::vector<uint32_t> table(RB_TABLE_WORDS, 0u);
  for (int j = 0; j < n_rules; ++j) table[bot * HSAD_RULE_MAX_RULES + j] = rb_pack(rules[j].code, rules[j].k);
  table[HSAD_RULE_MAX_BOTS * HSAD_RULE_MAX_RULES + bot] = (uint32_t)n_rules;
  const RbRules ru = {r.P, r.H, r.nC, r.nR, r.max_info, 2 * r.H + (r.P - 1) * (r.nC + r.nR) + 1, r.shuffle_color, r.deck_full};
  const int words = 80 + 6 * r.P * r.H + 10 * r.P;
  std::vector<int32_t> rec(words);
  std::vector<uint32_t> w(PL_FIXED + 6 * r.P);
  for (int k = 0; k < n; ++k) {
    for (int i = 0; i < words; ++i)
      if (scanf("%d", &rec[i]) != 1) return 2;
    long long key = 0;
    unsigned long long counter = 0;
    if (scanf("%lld %llu", &key, &counter) != 2) return 2;
    for (auto& x : w) x = 0u;
    if (pos_decode_record(rec.data(), r, w.data()) & (HSAD_POS_FIELD | HSAD_POS_HANDS)) return 3;
    const int p = rec[57];
    int fired = -2;
    const Words acc = {&w};
    const int uid = rb_act(acc, ru, p, table.data(), bot, (uint64_t)seed, (uint64_t)key, (uint64_t)counter, &fired);
    // every other seat gets the noop
    for (int q = 0; q < r.P; ++q)
      if (q != p && rb_act(acc, ru, q, table.data(), bot, (uint64_t)seed, (uint64_t)key, (uint64_t)counter, nullptr) != ru.A - 1) return 4;
    printf("%d %d %d\n", p, uid, fired);
  }
  return 0;
}
