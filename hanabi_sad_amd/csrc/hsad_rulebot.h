// hsad_rulebot.h — a rule-list Hanabi bot on the env's state planes: an ordered list of at most 8 rules, the first that fires gives
// the move.  Pure integer logic on what the acting seat may see (never its own cards).  Plain C++ (no HIP types, no allocation):
// hsad_env_rulebot.inc includes it under hipcc, tests/rulebot/rulebot_main.cc under g++.  Specification: include/hsad.h,
// HSAD_RULE_* and hsad_env_policy_rule (the header is the normative text; this file follows it).
//
// The state is read through an accessor `w(pl)` = plane word pl of the game (plane numbers and bit fields: hsad_planes.h), so that a
// kernel can hand over its planes where they are (global memory or LDS) without a copy: GlobalPlanes and LdsPlanes below.
#ifndef HSAD_RULEBOT_H
#define HSAD_RULEBOT_H

#include <stdint.h>

#include "hsad.h"
#include "hsad_planes.h"

#if defined(__HIPCC__)
#define HSAD_RB_FN __host__ __device__ inline
#else
#define HSAD_RB_FN inline
#endif

#define RB_TABLE_WORDS (HSAD_RULE_MAX_BOTS * HSAD_RULE_MAX_RULES + HSAD_RULE_MAX_BOTS)

struct RbRules {
  int P, H, nC, nR, max_info, A, shuffle_color;
  uint64_t deck_full;   // the full deck's 2-bit counts
};
// the rules of an env, from its parameter struct (csrc/hsad_env.hip: EnvParams)
template <class EP>
HSAD_RB_FN RbRules rb_rules_of(const EP& ep) {
  return RbRules{ep.P, ep.H, ep.nC, ep.nR, ep.max_info, ep.A, ep.shuffle_color, ep.deck_full};
}

// a rule as one word: code [0..7] | k [8..15].  A bot table is HSAD_RULE_MAX_BOTS rows of HSAD_RULE_MAX_RULES such words followed
// by the HSAD_RULE_MAX_BOTS list lengths (RB_TABLE_WORDS words in all).
HSAD_RB_FN uint32_t rb_pack(int32_t code, int32_t k) { return (uint32_t)code | ((uint32_t)k << 8); }

// 0 when the list is one the bot runs, else which refusal: 1 n_rules outside 1..8, 2 unknown code, 3 k out of range
HSAD_RB_FN int rb_rules_invalid(const hsad_rule* rules, int n_rules) {
  if (n_rules < 1 || n_rules > HSAD_RULE_MAX_RULES) return 1;
  for (int j = 0; j < n_rules; ++j) {
    const int code = rules[j].code, k = rules[j].k;
    if (code < HSAD_RULE_PLAY_CERTAIN || code > HSAD_RULE_LEGAL_RANDOM) return 2;
    const bool has_k = code == HSAD_RULE_PLAY_PROBABLE || code == HSAD_RULE_PLAY_PROBABLE_ENDGAME || code == HSAD_RULE_DISCARD_PROBABLE_DEAD;
    if (has_k ? (k < 0 || k > 100) : (k != 0)) return 3;
  }
  return 0;
}

HSAD_RB_FN int rb_popc32(uint32_t x) {
  x = x - ((x >> 1) & 0x55555555u);
  x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
  return (int)((((x + (x >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24);
}
HSAD_RB_FN int rb_popc64(uint64_t x) { return rb_popc32((uint32_t)x) + rb_popc32((uint32_t)(x >> 32)); }
HSAD_RB_FN int rb_ctz64(uint64_t x) { return rb_popc64((x & (0ull - x)) - 1ull); }   // x != 0

// policy_pick's choice: the k-th set bit of mask, k = h % popcount (mask != 0)
HSAD_RB_FN int rb_pick(uint32_t h, uint64_t mask) {
  int k = (int)(h % (uint32_t)rb_popc64(mask));
  while (k-- > 0) mask &= mask - 1;
  return rb_ctz64(mask);
}

// bit t = colour * 5 + rank of the 25-bit type mask: colour plausible and rank plausible
HSAD_RB_FN uint32_t rb_compat(uint32_t cp, uint32_t rp) {
  uint32_t m = 0;
  for (int c = 0; c < 5; ++c) m |= ((cp >> c) & 1u) ? (rp << (5 * c)) : 0u;
  return m;
}

// sum over the types of `mask` of the 2-bit counts of q: the mask's bits are spread to the even positions, then two popcounts
HSAD_RB_FN int rb_wsum(uint64_t q, uint32_t mask) {
  uint64_t x = mask;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return rb_popc64(q & x) + 2 * rb_popc64((q >> 1) & x);
}

// uid of "the hint for" the card (colour c, rank r) in slot i of the seat at target offset o; -1 when both masks are singletons
HSAD_RB_FN int rb_hint_for(const RbRules& ru, uint32_t pm, int o, int c, int r, uint32_t cp, uint32_t rp) {
  if (rb_popc32(rp) > 1) return 2 * ru.H + (ru.P - 1) * ru.nC + (o - 1) * ru.nR + r;
  if (rb_popc32(cp) > 1) return 2 * ru.H + (o - 1) * ru.nC + (int)((pm >> (3 * c)) & 7u);
  return -1;
}

// The move of seat p.  table: RB_TABLE_WORDS words (rb_pack rows, then the lengths), bot: which row.  *fired (may be null): index
// of the rule that decided, -1 when none did (lowest legal bit) or the seat is not on turn (noop).
template <class W>
HSAD_RB_FN int rb_act(const W& w, const RbRules& ru, int p, const uint32_t* table, int bot, uint64_t seed, uint64_t key, uint64_t counter,
                      int* fired) {
  const int P = ru.P, H = ru.H;
  if (fired) *fired = -1;
  const uint32_t board = w(PL_BOARD), misc = w(PL_MISC);
  if (board_cur(board) != p) return ru.A - 1;
  const int info = board_info(board), life = board_life(board), deck_size = misc_deck_size(misc);
  const uint32_t pm = ru.shuffle_color ? (w(PLPERM(p)) & 0x7fffu) : ((1u << 3) | (2u << 6) | (3u << 9) | (4u << 12));
  const uint64_t deck = (uint64_t)w(PL_DECK_LO) | ((uint64_t)w(PL_DECK_HI) << 32);
  const uint64_t disc = (uint64_t)w(PL_DISC_LO) | ((uint64_t)w(PL_DISC_HI) << 32);
  const uint32_t hw = w(PLH(p)), kcp = w(PLKCP(p)), krp = w(PLKRP(p)), kh = w(PLKH(p));
  const int L = (int)((hw >> 25) & 7u);

  // type masks: playable, dead, and the types the full deck holds
  uint32_t playable = 0, dead = 0, exists = 0;
  for (int c = 0; c < 5; ++c) {
    const int fw = board_fw(board, c);
    bool blocked = false;
    for (int r = 0; r < 5; ++r) {
      const int t = c * 5 + r;
      const uint32_t full = cnt2(ru.deck_full, t);
      if (full) exists |= 1u << t;
      if (r < fw || blocked) dead |= 1u << t;
      if (r == fw) playable |= 1u << t;
      if (r >= fw && cnt2(disc, t) == full) blocked = true;
    }
  }

  // the legal mask (legal_mask_of's uids) with its hint bits, and the pool = deck + own hand
  uint64_t pool = deck;
  for (int i = 0; i < 5; ++i)
    if (i < L) pool += (uint64_t)1 << (2 * ((hw >> (5 * i)) & 31u));
  const uint64_t lenmask = (1ull << L) - 1ull;
  uint64_t legal = lenmask << H;
  if (info < ru.max_info) legal |= lenmask;
  if (info > 0) {
    for (int o = 1; o < P; ++o) {
      const int q = (p + o) % P;
      const uint32_t thw = w(PLH(q));
      const int tl = (int)((thw >> 25) & 7u);
      uint32_t cm = 0, rm = 0;
      for (int i = 0; i < 5; ++i) {
        const int card = (int)((thw >> (5 * i)) & 31u);
        const int c = (card * 13) >> 6, r = card - 5 * c;
        if (i < tl) {
          cm |= 1u << ((pm >> (3 * c)) & 7u);
          rm |= 1u << r;
        }
      }
      legal |= (uint64_t)cm << (2 * H + (o - 1) * ru.nC);
      legal |= (uint64_t)rm << (2 * H + (P - 1) * ru.nC + (o - 1) * ru.nR);
    }
  }
  if (!legal) return ru.A - 1;   // (a seat on turn with an empty hand: no valid position has one)
  const uint64_t discard_bits = legal & ((1ull << H) - 1ull);
  const uint64_t hint_bits = legal & ~((1ull << (2 * H)) - 1ull);

  // per own slot: n, play, dead
  int n_[5], play_[5], dead_[5];
  for (int i = 0; i < 5; ++i) {
    const uint32_t cm = rb_compat((kcp >> (5 * i)) & 31u, (krp >> (5 * i)) & 31u);
    n_[i] = rb_wsum(pool, cm);
    play_[i] = rb_wsum(pool, cm & playable);
    dead_[i] = rb_wsum(pool, cm & dead);
  }

  const uint32_t* rules = table + bot * HSAD_RULE_MAX_RULES;
  const int n_rules = (int)table[HSAD_RULE_MAX_BOTS * HSAD_RULE_MAX_RULES + bot];
  for (int j = 0; j < n_rules; ++j) {
    const int code = (int)(rules[j] & 255u), k = (int)((rules[j] >> 8) & 255u);
    int uid = -1;
    switch (code) {
      case HSAD_RULE_PLAY_CERTAIN:
      case HSAD_RULE_DISCARD_CERTAIN_DEAD: {
        const bool disc_rule = code == HSAD_RULE_DISCARD_CERTAIN_DEAD;
        if (disc_rule && info >= ru.max_info) break;
        for (int i = 4; i >= 0; --i)
          if (i < L && (disc_rule ? dead_[i] : play_[i]) == n_[i]) uid = disc_rule ? i : H + i;
        break;
      }
      case HSAD_RULE_PLAY_PROBABLE:
      case HSAD_RULE_PLAY_PROBABLE_ENDGAME:
      case HSAD_RULE_DISCARD_PROBABLE_DEAD: {
        const bool disc_rule = code == HSAD_RULE_DISCARD_PROBABLE_DEAD;
        if (disc_rule ? (info >= ru.max_info) : (life <= 1)) break;
        if (code == HSAD_RULE_PLAY_PROBABLE_ENDGAME && deck_size != 0) break;
        if (L < 1) break;
        int bx = disc_rule ? dead_[0] : play_[0], bn = n_[0], bi = 0;
        for (int i = 1; i < 5; ++i) {
          const int x = disc_rule ? dead_[i] : play_[i];
          if (i < L && x * bn > bx * n_[i]) {
            bx = x;
            bn = n_[i];
            bi = i;
          }
        }
        if (bx * 100 >= k * bn) uid = disc_rule ? bi : H + bi;
        break;
      }
      case HSAD_RULE_HINT_PLAYABLE:
      case HSAD_RULE_HINT_USEFUL:
      case HSAD_RULE_HINT_DEAD: {
        if (info <= 0) break;
        for (int o = 1; o < P && uid < 0; ++o) {
          const int q = (p + o) % P;
          const uint32_t thw = w(PLH(q)), tcp = w(PLKCP(q)), trp = w(PLKRP(q));
          const int tl = (int)((thw >> 25) & 7u);
          for (int i = 0; i < 5 && uid < 0; ++i) {
            if (i >= tl) break;
            const int card = (int)((thw >> (5 * i)) & 31u);
            const int c = (card * 13) >> 6, r = card - 5 * c;
            const uint32_t cp = (tcp >> (5 * i)) & 31u, rp = (trp >> (5 * i)) & 31u;
            const uint32_t known = rb_compat(cp, rp) & exists;
            bool hit;
            if (code == HSAD_RULE_HINT_PLAYABLE)
              hit = ((playable >> card) & 1u) && (known & ~playable) != 0u;
            else if (code == HSAD_RULE_HINT_DEAD)
              hit = ((dead >> card) & 1u) && (known & ~dead) != 0u;
            else
              hit = !((dead >> card) & 1u);
            if (hit) uid = rb_hint_for(ru, pm, o, c, r, cp, rp);
          }
        }
        break;
      }
      case HSAD_RULE_HINT_RANDOM:
        if (info > 0 && hint_bits) uid = rb_pick(policy_hash(seed, key, counter, (uint64_t)(128 + 16 * p + j)), hint_bits);
        break;
      case HSAD_RULE_DISCARD_UNHINTED_OLDEST:
        if (info >= ru.max_info) break;
        for (int i = 4; i >= 0; --i)
          if (i < L && ((kh >> (6 * i)) & 63u) == 0u) uid = i;
        break;
      case HSAD_RULE_DISCARD_OLDEST:
        if (info < ru.max_info && L >= 1) uid = 0;
        break;
      case HSAD_RULE_DISCARD_RANDOM:
        if (info < ru.max_info && discard_bits) uid = rb_pick(policy_hash(seed, key, counter, (uint64_t)(128 + 16 * p + j)), discard_bits);
        break;
      case HSAD_RULE_LEGAL_RANDOM:
        uid = rb_pick(policy_hash(seed, key, counter, (uint64_t)(128 + 16 * p + j)), legal);
        break;
      default:
        break;
    }
    if (uid >= 0) {
      if (fired) *fired = j;
      return uid;
    }
  }
  return rb_ctz64(legal);
}

#if defined(__HIPCC__)
// ---- what a kernel that runs rb_act needs around it ----------------------------------------------------------------------------------
// the bots of a launch, as a kernel argument (324 bytes): the packed rule table above, then the bot of each seat (only
// hsad_env_playout_rule gives seats; elsewhere 0).  The kernels copy it to LDS once: which row a lane reads depends on its game.
struct RuleBots {
  uint32_t table[RB_TABLE_WORDS];
  int32_t seat[8];
  int n_bot;
};
constexpr int kRuleBotWords = RB_TABLE_WORDS + 8;

__device__ __forceinline__ void stage_bots(const RuleBots& rb, uint32_t* s_rb, int tid, int nthreads) {
  for (int k = tid; k < kRuleBotWords; k += nthreads) s_rb[k] = k < RB_TABLE_WORDS ? rb.table[k] : (uint32_t)rb.seat[k - RB_TABLE_WORDS];
  __syncthreads();
}

// the accessor `w` of rb_act on planes [npl][Gpad] in global memory, and on a wave's staged planes [npl][64] in LDS
struct GlobalPlanes {
  const uint32_t* planes;
  size_t Gpad;
  int g;
  __device__ __forceinline__ uint32_t operator()(int pl) const { return planes[(size_t)pl * Gpad + g]; }
};
constexpr int kRbPlaneStride = 64;   // one lane of a wave per game (hsad_env_rulebot.inc asserts that it is hsad_env.hip's kWave)
struct LdsPlanes {
  const uint32_t* s_st;
  int lane;
  __device__ __forceinline__ uint32_t operator()(int pl) const { return s_st[pl * kRbPlaneStride + lane]; }
};
#endif  // __HIPCC__

#endif  // HSAD_RULEBOT_H
