// hsad_partner.h — is this a seat layout hsad_actor_create_partnered (and _partnered_nets) can run?  The one check that entry point makes on its host
// arrays before anything is allocated or launched, and the text of each refusal.  Plain C++ (no HIP types, no allocation):
// hsad_actor_partner.inc includes it under hipcc, tests/partner/partner_main.cc under g++.  Specification: include/hsad.h,
// hsad_actor_partners and hsad_actor_create_partnered (the header is the normative text; this file follows it, and
// hanabi_sad_amd/actor.py PartnerSeats.verdict restates it).
#ifndef HSAD_PARTNER_H
#define HSAD_PARTNER_H

#include <stdint.h>
#include <stdio.h>

#include "hsad.h"
#include "hsad_rulebot.h"

// why a layout is refused (0: it is not); `index` and `value` name the offending entry
enum {
  PT_OK = 0,
  PT_VDN = 1,          // cfg->vdn != 0
  PT_PLAYERS = 2,      // more than 5 players or 5 cards a hand (value = players)
  PT_M = 3,            // M outside 1 .. G * P (value = M)
  PT_ROW_RANGE = 4,    // rows[index] = value outside 0 .. G * P - 1
  PT_ROW_ORDER = 5,    // rows[index] = value is not above rows[index - 1] (unsorted or duplicated)
  PT_N_BOT = 6,        // n_bot = value outside its limits
  PT_N_RULES = 7,      // bot index has value rules
  PT_RULE_CODE = 8,    // bot index names an unknown rule code
  PT_RULE_K = 9,       // bot index: k out of range
  PT_LEARNER_BOT = 10, // seat_bot[index] = value on a learner row (must be -1)
  PT_PARTNER_BOT = 11, // seat_bot[index] = value on a partner row (must be 0 .. n_bot - 1; with network partners -1 .. n_bot - 1)
  // partner_layout_verdict_nets only (hsad_actor_create_partnered_nets)
  PT_N_NET = 12,          // n_net = value outside 1 .. HSAD_PARTNER_MAX_NETS
  PT_NET_IN_DIM = 13,     // net index has in_dim value, the env has another
  PT_NET_NUM_ACTION = 14, // net index has num_action value, the env has another
  PT_LEARNER_NET = 15,    // seat_net[index] = value on a learner row (must be -1)
  PT_NET_RANGE = 16,      // seat_net[index] = value outside -1 .. n_net - 1
  PT_BOT_NET = 17,        // seat_net[index] = value on a row that seat_bot gives to a bot
  PT_NO_OWNER = 18,       // partner row index: neither a bot's nor a net's
  PT_NET_NO_ROW = 19      // net index owns no row
};
struct PartnerVerdict {
  int code, index, value;
};

// rows [M], rules [n_bot][HSAD_RULE_MAX_RULES], n_rules [n_bot], seat_bot [G * P]: host arrays, none null (rules and n_rules may be
// when n_bot == 0).  The first refusal in the order of the enum wins; within the rows and within seat_bot, the lowest index.
inline PartnerVerdict partner_layout_verdict(int G, int P, int H, int vdn, const int32_t* rows, int M, const hsad_rule* rules,
                                             const int32_t* n_rules, int n_bot, const int32_t* seat_bot) {
  const int64_t N = (int64_t)G * P;
  if (vdn) return {PT_VDN, 0, vdn};
  if (P > 5 || H > 5) return {PT_PLAYERS, 0, P};
  if (M < 1 || (int64_t)M > N) return {PT_M, 0, M};
  for (int i = 0; i < M; ++i) {
    if (rows[i] < 0 || (int64_t)rows[i] >= N) return {PT_ROW_RANGE, i, rows[i]};
    if (i > 0 && rows[i] <= rows[i - 1]) return {PT_ROW_ORDER, i, rows[i]};
  }
  if (n_bot < 0 || n_bot > HSAD_RULE_MAX_BOTS || (n_bot == 0 && (int64_t)M != N)) return {PT_N_BOT, 0, n_bot};
  for (int b = 0; b < n_bot; ++b) {
    switch (rb_rules_invalid(rules + (size_t)b * HSAD_RULE_MAX_RULES, n_rules[b])) {
      case 1: return {PT_N_RULES, b, n_rules[b]};
      case 2: return {PT_RULE_CODE, b, 0};
      case 3: return {PT_RULE_K, b, 0};
      default: break;
    }
  }
  int next = 0;   // rows is ascending: one cursor tells the learner's rows from the partners'
  for (int64_t r = 0; r < N; ++r) {
    const bool learner = next < M && rows[next] == r;
    if (learner) {
      ++next;
      if (seat_bot[r] != -1) return {PT_LEARNER_BOT, (int)r, seat_bot[r]};
    } else if (seat_bot[r] < 0 || seat_bot[r] >= n_bot) {
      return {PT_PARTNER_BOT, (int)r, seat_bot[r]};
    }
  }
  return {PT_OK, 0, 0};
}

// the refusal as hsad_last_error shows it; it names the offending entry
inline void partner_verdict_text(const PartnerVerdict& v, int G, int P, int n_bot, char* buf, size_t cap) {
  switch (v.code) {
    case PT_VDN: snprintf(buf, cap, "cfg->vdn = %d: a partnered actor is an IQL actor (one transition per learner row)", v.value); break;
    case PT_PLAYERS: snprintf(buf, cap, "more than 5 players or 5 cards a hand (players = %d)", v.value); break;
    case PT_M: snprintf(buf, cap, "M = %d learner rows, must be 1..%d", v.value, G * P); break;
    case PT_ROW_RANGE: snprintf(buf, cap, "rows[%d] = %d, must be 0..%d", v.index, v.value, G * P - 1); break;
    case PT_ROW_ORDER: snprintf(buf, cap, "rows[%d] = %d is not above rows[%d]: rows must be strictly ascending", v.index, v.value, v.index - 1); break;
    case PT_N_BOT: snprintf(buf, cap, "n_bot = %d, must be 1..%d (0 only when every row is the learner's)", v.value, HSAD_RULE_MAX_BOTS); break;
    case PT_N_RULES: snprintf(buf, cap, "bot %d has %d rules, must be 1..%d", v.index, v.value, HSAD_RULE_MAX_RULES); break;
    case PT_RULE_CODE: snprintf(buf, cap, "bot %d names an unknown rule code", v.index); break;
    case PT_RULE_K: snprintf(buf, cap, "bot %d: k must be 0..100 for the PROBABLE rules and 0 for every other", v.index); break;
    case PT_LEARNER_BOT: snprintf(buf, cap, "seat_bot[%d] = %d on a learner row, must be -1", v.index, v.value); break;
    case PT_PARTNER_BOT: snprintf(buf, cap, "seat_bot[%d] = %d on a partner row, must be 0..%d", v.index, v.value, n_bot - 1); break;
    default: snprintf(buf, cap, "ok"); break;
  }
}

// The same question for hsad_actor_create_partnered_nets: a partner row belongs to a bot (seat_bot[r] >= 0, seat_net[r] == -1) or to
// one of n_net frozen networks (seat_net[r] = k, seat_bot[r] == -1).  F, A: the env's feature size and action count; net_in_dim,
// net_num_action [n_net]: what each net was created with (handle identity is the entry point's to check).  With n_net == 0 and
// seat_net == NULL this is partner_layout_verdict, code for code.  Otherwise: the refusals 1 .. 9 as above, in that order, except
// that n_bot == 0 is fine (a row nobody owns is found below); then n_net, then per net its in_dim and its num_action; then ONE scan
// over the rows in ascending order, the lowest offending row winning and, within a row, seat_bot before seat_net (learner row:
// LEARNER_BOT, LEARNER_NET; partner row: PARTNER_BOT, NET_RANGE, BOT_NET, NO_OWNER); last, the lowest net without a row.
inline PartnerVerdict partner_layout_verdict_nets(int G, int P, int H, int vdn, const int32_t* rows, int M, const hsad_rule* rules,
                                                  const int32_t* n_rules, int n_bot, const int32_t* seat_bot, int F, int A, int n_net,
                                                  const int32_t* net_in_dim, const int32_t* net_num_action, const int32_t* seat_net) {
  if (n_net == 0 && !seat_net) return partner_layout_verdict(G, P, H, vdn, rows, M, rules, n_rules, n_bot, seat_bot);
  const int64_t N = (int64_t)G * P;
  if (vdn) return {PT_VDN, 0, vdn};
  if (P > 5 || H > 5) return {PT_PLAYERS, 0, P};
  if (M < 1 || (int64_t)M > N) return {PT_M, 0, M};
  for (int i = 0; i < M; ++i) {
    if (rows[i] < 0 || (int64_t)rows[i] >= N) return {PT_ROW_RANGE, i, rows[i]};
    if (i > 0 && rows[i] <= rows[i - 1]) return {PT_ROW_ORDER, i, rows[i]};
  }
  if (n_bot < 0 || n_bot > HSAD_RULE_MAX_BOTS) return {PT_N_BOT, 0, n_bot};
  for (int b = 0; b < n_bot; ++b) {
    switch (rb_rules_invalid(rules + (size_t)b * HSAD_RULE_MAX_RULES, n_rules[b])) {
      case 1: return {PT_N_RULES, b, n_rules[b]};
      case 2: return {PT_RULE_CODE, b, 0};
      case 3: return {PT_RULE_K, b, 0};
      default: break;
    }
  }
  if (n_net < 1 || n_net > HSAD_PARTNER_MAX_NETS) return {PT_N_NET, 0, n_net};
  for (int k = 0; k < n_net; ++k) {
    if (net_in_dim[k] != F) return {PT_NET_IN_DIM, k, net_in_dim[k]};
    if (net_num_action[k] != A) return {PT_NET_NUM_ACTION, k, net_num_action[k]};
  }
  bool owns[HSAD_PARTNER_MAX_NETS] = {};
  int next = 0;
  for (int64_t r = 0; r < N; ++r) {
    const int32_t b = seat_bot[r], k = seat_net[r];
    if (next < M && rows[next] == r) {
      ++next;
      if (b != -1) return {PT_LEARNER_BOT, (int)r, b};
      if (k != -1) return {PT_LEARNER_NET, (int)r, k};
      continue;
    }
    if (b < -1 || b >= n_bot) return {PT_PARTNER_BOT, (int)r, b};
    if (k < -1 || k >= n_net) return {PT_NET_RANGE, (int)r, k};
    if (b >= 0 && k >= 0) return {PT_BOT_NET, (int)r, k};
    if (b < 0 && k < 0) return {PT_NO_OWNER, (int)r, 0};
    if (k >= 0) owns[k] = true;
  }
  for (int k = 0; k < n_net; ++k)
    if (!owns[k]) return {PT_NET_NO_ROW, k, 0};
  return {PT_OK, 0, 0};
}

// the refusal of partner_layout_verdict_nets as hsad_last_error shows it (the codes 0 .. 11 with n_net == 0: partner_verdict_text)
inline void partner_verdict_text_nets(const PartnerVerdict& v, int G, int P, int n_bot, int n_net, int F, int A, char* buf, size_t cap) {
  if (n_net != 0 && v.code == PT_N_BOT) {   // the two old refusals whose limits differ next to nets
    snprintf(buf, cap, "n_bot = %d, must be 0..%d", v.value, HSAD_RULE_MAX_BOTS);
    return;
  }
  if (n_net != 0 && v.code == PT_PARTNER_BOT) {
    snprintf(buf, cap, "seat_bot[%d] = %d on a partner row, must be -1..%d", v.index, v.value, n_bot - 1);
    return;
  }
  switch (v.code) {
    case PT_N_NET: snprintf(buf, cap, "n_net = %d, must be 1..%d", v.value, HSAD_PARTNER_MAX_NETS); break;
    case PT_NET_IN_DIM: snprintf(buf, cap, "net %d has in_dim %d, the env's observation has %d features", v.index, v.value, F); break;
    case PT_NET_NUM_ACTION: snprintf(buf, cap, "net %d has num_action %d, the env has %d actions", v.index, v.value, A); break;
    case PT_LEARNER_NET: snprintf(buf, cap, "seat_net[%d] = %d on a learner row, must be -1", v.index, v.value); break;
    case PT_NET_RANGE: snprintf(buf, cap, "seat_net[%d] = %d, must be -1..%d", v.index, v.value, n_net - 1); break;
    case PT_BOT_NET: snprintf(buf, cap, "seat_net[%d] = %d on a row seat_bot gives to a bot: a row has one owner", v.index, v.value); break;
    case PT_NO_OWNER: snprintf(buf, cap, "row %d is neither the learner's nor a bot's nor a net's (seat_bot[%d] = seat_net[%d] = -1)", v.index, v.index, v.index); break;
    case PT_NET_NO_ROW: snprintf(buf, cap, "net %d owns no row: every net of the table must be seated", v.index); break;
    default: partner_verdict_text(v, G, P, n_bot, buf, cap); break;
  }
}

#endif  // HSAD_PARTNER_H
