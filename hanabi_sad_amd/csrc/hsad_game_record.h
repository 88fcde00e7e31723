// hsad_game_record.h — the record of one game (include/hsad.h: HSAD_GR_*, hsad_game_log_*, hsad_env_playout_logged): its byte
// layout, the capacity of a move log, the colour mapping of a logged move and the flag byte taken from the move classifier.  Plain
// C++ (no HIP types, no allocation): hsad_eval.hip and hsad_env_record.inc include it under hipcc, tests/game_record/record_main.cc
// under g++.  include/hsad.h is the normative text; tests/game_record_ref.py restates this file in Python.
#ifndef HSAD_GAME_RECORD_H
#define HSAD_GAME_RECORD_H

#include <stdint.h>

#include "hsad.h"
#include "hsad_behaviour.h"

// ---- capacity ---------------------------------------------------------------------------------------------------------------------
// How many moves can a game have?  Let D = deck_size - P * H be the cards left after the first deal.
//   * Every play or discard made while the deck holds a card deals one, so exactly D plays + discards happen up to and including
//     the move that takes the last card; at most D of them are discards.
//   * Every hint spends an information token.  Tokens come from the initial stock (max_information_tokens), from discards (one
//     each: at most D before the deck is empty) and from completed stacks (one each: at most `colors`).  So at most
//     max_information_tokens + D + colors hints are made while the deck holds a card.
//   * Once the last card is dealt every seat moves once more: P turns, whatever they are.
// Sum: L = D + (max_information_tokens + D + colors) + P = 2 * D + max_information_tokens + colors + P.  The standard 2-player game:
// 2 * 40 + 8 + 5 + 2 = 95.  The env's step counter is 8 bits wide, so a log is refused when L > 255 (gr_capacity_ok).
HSAD_RB_FN int gr_capacity(int P, int H, int deck_size, int max_info, int colors) { return 2 * (deck_size - P * H) + max_info + colors + P; }
HSAD_RB_FN bool gr_capacity_ok(int L) { return L >= 1 && L <= 255; }

// ---- byte layout of a record (every field one byte, so the record reads the same on any host) --------------------------------------
enum : int {
  GR_OFF_VERSION = 0,    // HSAD_GR_VERSION
  GR_OFF_P = 1,
  GR_OFF_H = 2,
  GR_OFF_COLORS = 3,
  GR_OFF_RANKS = 4,
  GR_OFF_MAX_INFO = 5,
  GR_OFF_MAX_LIFE = 6,
  GR_OFF_BOMB = 7,
  GR_OFF_NMOVES = 8,
  GR_OFF_NDEALT = 9,
  GR_OFF_SCORE = 10,
  GR_OFF_LIVES = 11,
  GR_OFF_INFO = 12,
  GR_OFF_END = 13,       // HSAD_GR_END_*
  GR_OFF_CAPACITY = 14,  // L: the length of each of the three move planes
  GR_OFF_RESERVED = 15,  // 0
  GR_OFF_DECK = 16,      // 52 card types (colour * 5 + rank) in deal order, 0 past n_dealt: a deck-history row, a deal script
  GR_OFF_MOVES = 68      // move[L] | greedy[L] | flags[L], 0 past n_moves
};
HSAD_RB_FN int gr_record_bytes(int L) { return GR_OFF_MOVES + 3 * L; }

struct GrHeader {
  int version, P, H, colors, ranks, max_info, max_life, bomb, n_moves, n_dealt, score, lives, info, end, capacity;
};
HSAD_RB_FN void gr_pack_header(const GrHeader& h, uint8_t* out) {
  out[GR_OFF_VERSION] = (uint8_t)h.version;
  out[GR_OFF_P] = (uint8_t)h.P;
  out[GR_OFF_H] = (uint8_t)h.H;
  out[GR_OFF_COLORS] = (uint8_t)h.colors;
  out[GR_OFF_RANKS] = (uint8_t)h.ranks;
  out[GR_OFF_MAX_INFO] = (uint8_t)h.max_info;
  out[GR_OFF_MAX_LIFE] = (uint8_t)h.max_life;
  out[GR_OFF_BOMB] = (uint8_t)h.bomb;
  out[GR_OFF_NMOVES] = (uint8_t)h.n_moves;
  out[GR_OFF_NDEALT] = (uint8_t)h.n_dealt;
  out[GR_OFF_SCORE] = (uint8_t)h.score;
  out[GR_OFF_LIVES] = (uint8_t)h.lives;
  out[GR_OFF_INFO] = (uint8_t)h.info;
  out[GR_OFF_END] = (uint8_t)h.end;
  out[GR_OFF_CAPACITY] = (uint8_t)h.capacity;
  out[GR_OFF_RESERVED] = 0;
}
HSAD_RB_FN GrHeader gr_unpack_header(const uint8_t* in) {
  GrHeader h;
  h.version = in[GR_OFF_VERSION];
  h.P = in[GR_OFF_P];
  h.H = in[GR_OFF_H];
  h.colors = in[GR_OFF_COLORS];
  h.ranks = in[GR_OFF_RANKS];
  h.max_info = in[GR_OFF_MAX_INFO];
  h.max_life = in[GR_OFF_MAX_LIFE];
  h.bomb = in[GR_OFF_BOMB];
  h.n_moves = in[GR_OFF_NMOVES];
  h.n_dealt = in[GR_OFF_NDEALT];
  h.score = in[GR_OFF_SCORE];
  h.lives = in[GR_OFF_LIVES];
  h.info = in[GR_OFF_INFO];
  h.end = in[GR_OFF_END];
  h.capacity = in[GR_OFF_CAPACITY];
  return h;
}

// how a game ended, from its board and status words (the order of the env's own test: lives, fireworks, turns; then max_len)
HSAD_RB_FN int gr_end_reason(uint32_t board, uint32_t misc, int colors, int ranks) {
  if (!misc_started(misc) || !misc_term(misc)) return HSAD_GR_END_UNFINISHED;
  if (board_life(board) < 1) return HSAD_GR_END_LIVES;
  if (board_fw_sum(board) >= colors * ranks) return HSAD_GR_END_PERFECT;
  if (board_turns(board) <= 0) return HSAD_GR_END_DECK;
  return HSAD_GR_END_MAX_LEN;
}
// the score a record holds: the latched last score of a finished game, what the fireworks show (0 after a bomb) of a running one
HSAD_RB_FN int gr_score(uint32_t board, uint32_t misc, int bomb) {
  if (misc_started(misc) && misc_term(misc)) return misc_last_score(misc) < 0 ? 0 : misc_last_score(misc);
  return (board_life(board) <= 0 && bomb) ? 0 : board_fw_sum(board);
}

// ---- the colour of a logged colour hint ---------------------------------------------------------------------------------------------
// A uid names a colour hint's colour through the ACTOR's permutation (perm: 5 x 3 bits, entry c = what the actor calls colour c); a
// record names the cards' true colour, so that it reads the same whatever permutation the env drew.  Every other uid is unchanged.
constexpr uint32_t kGrIdentityPerm = (0u) | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12);
HSAD_RB_FN bool gr_is_colour_hint(int uid, int P, int H, int nC) { return uid >= 2 * H && uid < 2 * H + (P - 1) * nC; }
HSAD_RB_FN int gr_uid_to_true(int uid, int P, int H, int nC, uint32_t perm) {
  if (!gr_is_colour_hint(uid, P, H, nC)) return uid;
  const int k = uid - 2 * H, o = k / nC, value = k - o * nC;
  int truth = value;
  for (int c = 0; c < 5; ++c)
    if ((int)((perm >> (3 * c)) & 7u) == value) truth = c;
  return 2 * H + o * nC + truth;
}
HSAD_RB_FN int gr_uid_from_true(int uid, int P, int H, int nC, uint32_t perm) {
  if (!gr_is_colour_hint(uid, P, H, nC)) return uid;
  const int k = uid - 2 * H, o = k / nC, truth = k - o * nC;
  return 2 * H + o * nC + (int)((perm >> (3 * truth)) & 7u);
}

// ---- the flag byte of a move: eight yes / no answers read off bh_classify's increments ---------------------------------------------
HSAD_RB_FN uint8_t gr_flags(bh_inc inc) {
  if (!bh_get(inc, HSAD_BH_MOVES)) return 0;
  const bool play = bh_get(inc, HSAD_BH_PLAY_OK) || bh_get(inc, HSAD_BH_PLAY_FAIL);
  const bool hint = bh_get(inc, HSAD_BH_HINT_COLOUR) || bh_get(inc, HSAD_BH_HINT_RANK);
  uint32_t f = HSAD_GR_COUNTED;
  if (bh_get(inc, HSAD_BH_PLAY_FAIL)) f |= HSAD_GR_PLAY_FAIL;
  if (play && !bh_get(inc, HSAD_BH_PLAY_CERTAIN)) f |= HSAD_GR_PLAY_UNCERTAIN;
  if (bh_get(inc, HSAD_BH_LAST_COPY_LOST)) f |= HSAD_GR_LAST_COPY_LOST;
  if (bh_get(inc, HSAD_BH_LAST_LIFE)) f |= HSAD_GR_LAST_LIFE;
  if (hint && !bh_get(inc, HSAD_BH_HINT_PLAYABLE)) f |= HSAD_GR_HINT_NOT_PLAYABLE;
  if (bh_get(inc, HSAD_BH_DISCARD) && !bh_get(inc, HSAD_BH_DISCARD_CERTAIN_DEAD)) f |= HSAD_GR_DISCARD_UNCERTAIN;
  if (bh_get(inc, HSAD_BH_INFO_SUM) == 0) f |= HSAD_GR_NO_INFO;
  return (uint8_t)f;
}

// ---- a game against a filter (hsad_game_log_select), from what the log and the planes hold ------------------------------------------
// flag_hit: some move k of the game with ((seat_mask >> (k % P)) & 1) carries a flag of flag_mask (seat k % P makes move k: seat 0
// opens and every move passes the turn on).  The caller computes it; it is not looked at when flag_mask == 0.
HSAD_RB_FN bool gr_filter_pass(const hsad_game_filter& f, int score, int lives, int n_moves, int end, bool flag_hit) {
  if (end == HSAD_GR_END_UNFINISHED) return false;
  if (score < f.score_min || score > f.score_max) return false;
  if (lives > f.max_lives) return false;
  if (n_moves < f.moves_min || n_moves > f.moves_max) return false;
  if (f.end_mask && !((f.end_mask >> end) & 1)) return false;
  if (f.flag_mask && !flag_hit) return false;
  return true;
}

// what the log and playout kernels need of an env (hsad_internal_env_record_view, hsad_env_record.inc); not part of the public header
struct GrEnvView {
  const uint32_t* planes;     // [npl][Gpad]
  const uint8_t* deck_hist;   // [Gpad][52]
  int G, Gpad, track_dh, deck_max, max_life, bomb, device;
  RbRules ru;
};

#endif  // HSAD_GAME_RECORD_H
