// Stand-alone harness for partner_layout_verdict_nets of hanabi_sad_amd/csrc/hsad_partner.h (tests/test_actor_netpartner_cpu.py builds
// it with the sanitizers).
// stdin: "n", then n layouts: "G P H vdn M n_bot has_net n_net F A", M rows, per bot "n_rules" and min(n_rules, 8) pairs "code k",
// G * P seat_bot, and when has_net: n_net pairs "in_dim num_action", then G * P seat_net (has_net 0: seat_net == NULL).
// stdout: per layout "code index value" of partner_layout_verdict_nets, then the refusal's text on a line of its own.
#include <cstdio>
#include <vector>

#include "hsad_partner.h"

int main() {
  int n = 0;
  if (scanf("%d", &n) != 1) return 2;
  for (int k = 0; k < n; ++k) {
    int G, P, H, vdn, M, n_bot, has_net, n_net, F, A;
    if (scanf("%d %d %d %d %d %d %d %d %d %d", &G, &P, &H, &vdn, &M, &n_bot, &has_net, &n_net, &F, &A) != 10) return 2;
    if (G < 1 || P < 1 || G * P > (1 << 20) || M > (1 << 20) || n_bot < 0 || n_bot > 64 || n_net < 0 || n_net > 64) return 2;
    // exactly the arrays the caller describes: a read past one of them is the sanitizer's to find
    std::vector<int32_t> rows((size_t)(M > 0 ? M : 0)), n_rules((size_t)n_bot), seat_bot((size_t)G * P);
    std::vector<hsad_rule> rules((size_t)n_bot * HSAD_RULE_MAX_RULES);
    std::vector<int32_t> in_dim((size_t)n_net), num_action((size_t)n_net), seat_net(has_net ? (size_t)G * P : 0);
    for (auto& x : rows)
      if (scanf("%d", &x) != 1) return 2;
    for (int b = 0; b < n_bot; ++b) {
      if (scanf("%d", &n_rules[b]) != 1) return 2;
      for (int j = 0; j < n_rules[b] && j < HSAD_RULE_MAX_RULES; ++j)
        if (scanf("%d %d", &rules[(size_t)b * HSAD_RULE_MAX_RULES + j].code, &rules[(size_t)b * HSAD_RULE_MAX_RULES + j].k) != 2) return 2;
    }
    for (auto& x : seat_bot)
      if (scanf("%d", &x) != 1) return 2;
    if (has_net) {
      for (int j = 0; j < n_net; ++j)
        if (scanf("%d %d", &in_dim[j], &num_action[j]) != 2) return 2;
      for (auto& x : seat_net)
        if (scanf("%d", &x) != 1) return 2;
    }
    const PartnerVerdict v = partner_layout_verdict_nets(G, P, H, vdn, rows.data(), M, rules.data(), n_rules.data(), n_bot, seat_bot.data(), F, A,
                                                         n_net, in_dim.data(), num_action.data(), has_net ? seat_net.data() : nullptr);
    char text[256];
    partner_verdict_text_nets(v, G, P, n_bot, n_net, F, A, text, sizeof(text));
    printf("%d %d %d\n%s\n", v.code, v.index, v.value, text);
  }
  return 0;
}
