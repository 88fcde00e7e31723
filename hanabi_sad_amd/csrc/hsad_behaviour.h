// hsad_behaviour.h — a move classifier on the env's state planes: what kind of move is the seat on turn about to make, counted in the
// HSAD_BH_* counters of a tournament (who hints and how, who plays without being sure, who loses the last copy of a card, who spends
// the last life).  Pure integer logic on the position BEFORE the move; the position is only read.  Plain C++ (no HIP types, no
// allocation): hsad_eval.hip includes it under hipcc, tests/behaviour/behaviour_main.cc under g++.  Specification: include/hsad.h,
// HSAD_BH_* and hsad_seating_behaviour (the header is the normative text; this file follows it, with the definitions of the
// rule-bot section there: pool, compat_i, n_i, play_i, dead_i, playable(t), dead(t)).
//
// The state is read through the accessor `w(pl)` of rb_act (hsad_rulebot.h), the rules come as its RbRules.
#ifndef HSAD_BEHAVIOUR_H
#define HSAD_BEHAVIOUR_H

#include <stdint.h>

#include "hsad.h"
#include "hsad_planes.h"
#include "hsad_rulebot.h"

// The increments of one move, 4 bits per counter (counter k in bits [4k, 4k + 4)): every increment is 0 or 1 except HINT_CARDS
// (at most 5 cards in a hand) and INFO_SUM (the info field of PL_BOARD is 4 bits wide).  One word, so that a kernel keeps it in
// registers; 0 = nothing counted.
typedef uint64_t bh_inc;
HSAD_RB_FN int bh_get(bh_inc inc, int k) { return (int)((inc >> (4 * k)) & 15u); }
HSAD_RB_FN bh_inc bh_put(int k, int v) { return (bh_inc)(uint32_t)v << (4 * k); }

// what seat p (the seat on turn) adds to the counters by playing uid in the position `w`
template <class W>
HSAD_RB_FN bh_inc bh_classify(const W& w, const RbRules& ru, int p, int64_t uid) {
  const int P = ru.P, H = ru.H, nC = ru.nC, nR = ru.nR;
  if (uid < 0 || uid >= (int64_t)(ru.A - 1)) return 0;   // the noop, or no uid at all
  const int u = (int)uid;
  const uint32_t board = w(PL_BOARD);
  const int info = board_info(board), life = board_life(board);
  const uint64_t disc = (uint64_t)w(PL_DISC_LO) | ((uint64_t)w(PL_DISC_HI) << 32);

  // type masks: playable and dead (rb_act's)
  uint32_t playable = 0, dead = 0;
  for (int c = 0; c < 5; ++c) {
    const int fw = board_fw(board, c);
    bool blocked = false;
    for (int r = 0; r < 5; ++r) {
      const int t = c * 5 + r;
      if (r < fw || blocked) dead |= 1u << t;
      if (r == fw) playable |= 1u << t;
      if (r >= fw && cnt2(disc, t) == cnt2(ru.deck_full, t)) blocked = true;
    }
  }
  const bh_inc moved = bh_put(HSAD_BH_MOVES, 1) | bh_put(HSAD_BH_INFO_SUM, info);

  if (u < 2 * H) {   // a discard or a play of own slot i
    const bool is_play = u >= H;
    const int i = is_play ? u - H : u;
    const uint32_t hw = w(PLH(p));
    const int L = (int)((hw >> 25) & 7u);
    if (i >= L) return 0;
    const int card = (int)((hw >> (5 * i)) & 31u);
    // the mover's own knowledge of the slot: n_i, play_i, dead_i over pool = deck + own hand
    uint64_t pool = (uint64_t)w(PL_DECK_LO) | ((uint64_t)w(PL_DECK_HI) << 32);
    for (int j = 0; j < 5; ++j)
      if (j < L) pool += (uint64_t)1 << (2 * ((hw >> (5 * j)) & 31u));
    const uint32_t cm = rb_compat((w(PLKCP(p)) >> (5 * i)) & 31u, (w(PLKRP(p)) >> (5 * i)) & 31u);
    const int n_i = rb_wsum(pool, cm);
    const bool ok = (playable >> card) & 1u;
    const bool lost = !((dead >> card) & 1u) && cnt2(disc, card) + 1u == cnt2(ru.deck_full, card);
    bh_inc inc = moved;
    if (is_play) {
      inc |= bh_put(ok ? HSAD_BH_PLAY_OK : HSAD_BH_PLAY_FAIL, 1);
      if (rb_wsum(pool, cm & playable) == n_i) inc |= bh_put(HSAD_BH_PLAY_CERTAIN, 1);
      if (!ok && lost) inc |= bh_put(HSAD_BH_LAST_COPY_LOST, 1);
      if (!ok && life == 1) inc |= bh_put(HSAD_BH_LAST_LIFE, 1);
    } else {
      inc |= bh_put(HSAD_BH_DISCARD, 1);
      if (rb_wsum(pool, cm & dead) == n_i) inc |= bh_put(HSAD_BH_DISCARD_CERTAIN_DEAD, 1);
      if (lost) inc |= bh_put(HSAD_BH_LAST_COPY_LOST, 1);
    }
    return inc;
  }

  // a hint: colour hints first, by target offset, then rank hints
  const int k = u - 2 * H;
  const bool by_rank = k >= (P - 1) * nC;
  const int kk = by_rank ? k - (P - 1) * nC : k;
  const int width = by_rank ? nR : nC;
  const int o = kk / width + 1;
  int value = kk - (o - 1) * width;
  if (!by_rank && ru.shuffle_color) {   // the uid names the colour through the actor's permutation: back to the card's colour
    const uint32_t pm = w(PLPERM(p)) & 0x7fffu;
    int truth = -1;
    for (int c = 0; c < 5; ++c)
      if ((int)((pm >> (3 * c)) & 7u) == value) truth = c;
    value = truth;
  }
  const uint32_t thw = w(PLH((p + o) % P));
  const int tl = (int)((thw >> 25) & 7u);
  int touched = 0;
  bool any_playable = false;
  for (int i = 0; i < 5; ++i) {
    const int card = (int)((thw >> (5 * i)) & 31u);
    const int c = (card * 13) >> 6, r = card - 5 * c;
    if (i < tl && (by_rank ? r : c) == value) {
      ++touched;
      if ((playable >> card) & 1u) any_playable = true;
    }
  }
  if (!touched) return 0;
  return moved | bh_put(by_rank ? HSAD_BH_HINT_RANK : HSAD_BH_HINT_COLOUR, 1) | bh_put(HSAD_BH_HINT_CARDS, touched) |
         (any_playable ? bh_put(HSAD_BH_HINT_PLAYABLE, 1) : (bh_inc)0);
}

#endif  // HSAD_BEHAVIOUR_H
