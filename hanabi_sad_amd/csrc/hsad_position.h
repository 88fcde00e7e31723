// hsad_position.h — is this a Hanabi position the env's kernels can be handed?  The decoder of the canonical int32 record
// (hsad_env_export_state's layout) into the env's state-plane words, and position_valid, the one check hsad_env_import_state and
// hsad_env_restore run before a word of a game is written.  Plain C++ (no HIP types, no allocation): hsad_env_position.inc includes
// it under hipcc, tests/position/position_main.cc under g++.  Specification: include/hsad.h, HSAD_POS_* and hsad_env_import_state.
//
// Plane words of one game: index = plane number, fields as hsad_planes.h describes them.
#ifndef HSAD_POSITION_H
#define HSAD_POSITION_H

#include <stdint.h>

#include "hsad.h"
#include "hsad_planes.h"

#if defined(__HIPCC__)
#define HSAD_POS_FN __host__ __device__ inline
#else
#define HSAD_POS_FN inline
#endif

#define POS_MAX_PLAYERS 5
#define POS_MAX_PLANES (PL_FIXED + 6 * POS_MAX_PLAYERS)

struct PosRules {
  int P, H, nC, nR, max_info, max_life, max_len, shuffle_color;
  uint64_t deck_full;   // the full deck's 2-bit counts
};

// v into a field of `bits` bits, biased by `bias` (the planes store cur_player + 1, hinted colour + 1, ...); sets *bad when it does not fit
HSAD_POS_FN uint32_t pos_field(int32_t v, int bias, int bits, bool* bad) {
  const int64_t x = (int64_t)v + bias;
  if (x < 0 || x >= ((int64_t)1 << bits)) {
    *bad = true;
    return 0u;
  }
  return (uint32_t)x;
}

// The canonical record o (hsad_env_state_words() words) -> plane words w[0 .. 10 + 6 P) of a started, not terminated game.  Words
// 7..9 (generator) and the eps planes are left alone; record word 73 is not read.  Returns HSAD_POS_FIELD when a value does not
// fit the bit field that holds it, else HSAD_POS_HANDS when a hand has a hole (either is reported alone and w is not to be used:
// the record describes no planes), else HSAD_POS_STEP for num_step outside 0..255 (w then holds step 0), else 0.
// Fields the last move's type does not use, and the knowledge words of an empty slot, are not read.
HSAD_POS_FN uint32_t pos_decode_record(const int32_t* o, const PosRules& r, uint32_t* w) {
  const int P = r.P, H = r.H;
  bool bad = false;
  uint32_t flags = 0;
  uint64_t deck = 0, disc = 0;
  for (int t = 0; t < 25; ++t) {
    deck |= (uint64_t)pos_field(o[t], 0, 2, &bad) << (2 * t);
    disc |= (uint64_t)pos_field(o[25 + t], 0, 2, &bad) << (2 * t);
  }
  w[PL_DECK_LO] = (uint32_t)deck;
  w[PL_DECK_HI] = (uint32_t)(deck >> 32);
  w[PL_DISC_LO] = (uint32_t)disc;
  w[PL_DISC_HI] = (uint32_t)(disc >> 32);
  uint32_t board = 0;
  for (int c = 0; c < 5; ++c) board |= pos_field(o[50 + c], 0, 3, &bad) << (3 * c);
  board |= pos_field(o[55], 0, 4, &bad) << 15;
  board |= pos_field(o[56], 0, 2, &bad) << 19;
  board |= pos_field(o[59], 0, 3, &bad) << 21;
  board |= pos_field(o[57], 1, 3, &bad) << 24;
  board |= pos_field(o[58], 0, 3, &bad) << 27;
  w[PL_BOARD] = board;
  uint32_t misc = 1u << 15;
  if (o[60] < 0 || o[60] > 255)
    flags |= HSAD_POS_STEP;
  else
    misc |= (uint32_t)o[60];
  misc |= pos_field(o[61], 0, 6, &bad) << 8;
  misc |= pos_field(o[74], 1, 6, &bad) << 16;
  w[PL_MISC] = misc;
  uint32_t rec = pos_field(o[62], 0, 3, &bad);
  const int type = (int)rec;
  if (type) rec |= pos_field(o[63], 0, 3, &bad) << 3;
  if (type >= 3) {
    rec |= pos_field(o[64], 0, 3, &bad) << 6;
    if (type == 3) rec |= pos_field(o[65], 0, 3, &bad) << 9;
    if (type == 4) rec |= pos_field(o[66], 0, 3, &bad) << 12;
    rec |= pos_field(o[68], 0, 5, &bad) << 18;
  } else if (type) {
    rec |= pos_field(o[67], 0, 3, &bad) << 15;
    rec |= pos_field(o[69], 0, 3, &bad) << 23;
    rec |= pos_field(o[70], 0, 3, &bad) << 26;
    rec |= pos_field(o[71], 0, 1, &bad) << 29;
    rec |= pos_field(o[72], 0, 1, &bad) << 30;
  }
  w[PL_LASTMV] = rec;
  for (int p = 0; p < P; ++p) {
    uint32_t hw = 0, kcp = 0, krp = 0, kh = 0;
    int len = 0;
    bool gap = false;
    for (int i = 0; i < H; ++i) {
      const int32_t* s = o + 80 + (p * H + i) * 6;
      if (s[0] == -1) {
        gap = true;
        continue;
      }
      if (gap) {
        flags |= HSAD_POS_HANDS;
        continue;
      }
      hw |= pos_field(s[0], 0, 5, &bad) << (5 * i);
      kcp |= pos_field(s[1], 0, 5, &bad) << (5 * i);
      krp |= pos_field(s[2], 0, 5, &bad) << (5 * i);
      kh |= pos_field(s[3], 1, 3, &bad) << (6 * i);
      kh |= pos_field(s[4], 1, 3, &bad) << (6 * i + 3);
      len = i + 1;
    }
    w[PLH(p)] = hw | ((uint32_t)len << 25);
    w[PLKCP(p)] = kcp;
    w[PLKRP(p)] = krp;
    w[PLKH(p)] = kh;
    uint32_t pw = 0;
    const int base = 80 + P * H * 6;
    for (int c = 0; c < 5; ++c) {
      pw |= pos_field(o[base + p * 5 + c], 0, 3, &bad) << (3 * c);
      pw |= pos_field(o[base + P * 5 + p * 5 + c], 0, 3, &bad) << (15 + 3 * c);
    }
    w[PLPERM(p)] = pw;
  }
  if (bad) return (uint32_t)HSAD_POS_FIELD;
  if (flags & HSAD_POS_HANDS) return (uint32_t)HSAD_POS_HANDS;
  return flags;
}

// The plane words of one started game -> HSAD_POS_* flags, 0 = a live position every kernel of the env can run on.  A finished
// position gets HSAD_POS_TERMINAL and is held to what env_logic leaves behind a final move (no deal follows it: the mover's hand
// may be short over a non-empty deck with the chance player on turn, life and turns_to_play may be 0, num_step may equal max_len).
HSAD_POS_FN uint32_t position_valid(const uint32_t* w, const PosRules& r) {
  const int P = r.P, H = r.H;
  uint32_t f = 0;
  const uint64_t deck = (uint64_t)w[PL_DECK_LO] | ((uint64_t)w[PL_DECK_HI] << 32);
  const uint64_t disc = (uint64_t)w[PL_DISC_LO] | ((uint64_t)w[PL_DISC_HI] << 32);
  const uint32_t board = w[PL_BOARD], misc = w[PL_MISC], rec = w[PL_LASTMV];
  const uint32_t cmask = (1u << r.nC) - 1u, rmask = (1u << r.nR) - 1u;
  const int info = board_info(board), life = board_life(board), turns = board_turns(board);
  const int cur = board_cur(board), next = board_next(board);
  const int num_step = misc_num_step(misc), deck_size = misc_deck_size(misc);

  // ---- hands: lengths, nothing above the length, and the cards held per type ----
  int n_short = 0, short_seat = -1;
  for (int p = 0; p < P; ++p) {
    const uint32_t hw = w[PLH(p)];
    int len = (int)((hw >> 25) & 7u);
    if (len > H || len < H - 1 || (hw >> 28) != 0u) f |= HSAD_POS_HANDS;
    if (len > H) len = H;
    if (len < H) {
      n_short += 1;
      short_seat = p;
    }
    const uint32_t above5 = len >= 5 ? 0u : (0x1ffffffu >> (5 * len)) << (5 * len);
    const uint32_t above6 = len >= 5 ? 0xc0000000u : (0xffffffffu >> (6 * len)) << (6 * len);
    if (hw & above5) f |= HSAD_POS_HANDS;
    const uint32_t kcp = w[PLKCP(p)], krp = w[PLKRP(p)], kh = w[PLKH(p)];
    if ((kcp & (above5 | 0xfe000000u)) || (krp & (above5 | 0xfe000000u)) || (kh & above6)) f |= HSAD_POS_KNOWLEDGE;
    for (int i = 0; i < len; ++i) {
      const int card = (int)((hw >> (5 * i)) & 31u);
      const int c = card / 5, k = card - 5 * c;
      if (c >= r.nC || k >= r.nR) {
        f |= HSAD_POS_CONSERVATION;   // (card >= 25 is colour >= 5)
        continue;
      }
      const uint32_t cm = (kcp >> (5 * i)) & 31u, rm = (krp >> (5 * i)) & 31u;
      const int hc = (int)((kh >> (6 * i)) & 7u) - 1, hr = (int)((kh >> (6 * i + 3)) & 7u) - 1;
      if (cm == 0u || rm == 0u || (cm & ~cmask) || (rm & ~rmask) || !((cm >> c) & 1u) || !((rm >> k) & 1u)) f |= HSAD_POS_KNOWLEDGE;
      if (hc >= 0 && (hc != c || cm != (1u << c))) f |= HSAD_POS_KNOWLEDGE;
      if (hr >= 0 && (hr != k || rm != (1u << k))) f |= HSAD_POS_KNOWLEDGE;
    }
  }

  // ---- conservation, per card type ----
  int deck_n = 0, fsum = 0;
  for (int c = 0; c < 5; ++c) {
    const int fw = board_fw(board, c);
    if (c >= r.nC) {
      if (fw) f |= HSAD_POS_CONSERVATION;
    } else {
      if (fw > r.nR) f |= HSAD_POS_BOARD;
      fsum += fw;
    }
    for (int k = 0; k < 5; ++k) {
      const int t = c * 5 + k;
      int held = 0;
      for (int p = 0; p < P; ++p) {
        const uint32_t hw = w[PLH(p)];
        int len = (int)((hw >> 25) & 7u);
        if (len > H) len = H;
        for (int i = 0; i < len; ++i) held += ((int)((hw >> (5 * i)) & 31u) == t) ? 1 : 0;
      }
      const int have = (int)cnt2(deck, t) + (int)cnt2(disc, t) + held + ((c < r.nC && fw > k) ? 1 : 0);
      if (have != (int)cnt2(r.deck_full, t)) f |= HSAD_POS_CONSERVATION;   // (deck_full is 0 outside the rules' colours and ranks)
      deck_n += (int)cnt2(deck, t);
    }
  }
  if ((deck >> 50) || (disc >> 50)) f |= HSAD_POS_CONSERVATION;
  if (deck_size != deck_n) f |= HSAD_POS_CONSERVATION;

  // ---- live or finished ----
  if (r.max_len > 0 && num_step > r.max_len) f |= HSAD_POS_STEP;
  const bool term = life < 1 || fsum >= r.nC * r.nR || turns < 1 || (r.max_len > 0 && num_step == r.max_len);

  // ---- board ----
  if (info > r.max_info || life > r.max_life || turns > P || cur >= P || next >= P || (board >> 30) != 0u) f |= HSAD_POS_BOARD;
  if (deck_n > 0) {
    // a deal follows every play or discard of a live game, so its hands are full; behind a final move the mover's may be short,
    // and then the chance player is on turn (advance_player) with the seat after the mover next
    if (turns != P) f |= HSAD_POS_BOARD;
    if (n_short > (term ? 1 : 0)) f |= HSAD_POS_HANDS;
    if (term && n_short == 1) {
      if (cur != -1 || next != (short_seat + 1) % P) f |= HSAD_POS_BOARD;
    } else if (cur < 0) {
      f |= HSAD_POS_BOARD;
    }
  } else {
    // every move on an empty deck takes one turn, and only such a move can leave a hand short
    if (n_short > P - turns) f |= HSAD_POS_HANDS;
    if (cur < 0) f |= HSAD_POS_BOARD;
  }
  if (cur >= 0 && cur < P && next != (cur + 1) % P) f |= HSAD_POS_BOARD;

  // ---- last move: every field the encoder indexes with ----
  const int type = (int)(rec & 7u);
  if (type > 4 || (rec >> 31)) f |= HSAD_POS_LASTMOVE;
  if (type >= 1 && type <= 4) {
    if ((int)((rec >> 3) & 7u) >= P) f |= HSAD_POS_LASTMOVE;
    if (type >= 3) {
      const int off = (int)((rec >> 6) & 7u);
      if (off < 1 || off > P - 1) f |= HSAD_POS_LASTMOVE;
      if (type == 3 && (int)((rec >> 9) & 7u) >= r.nC) f |= HSAD_POS_LASTMOVE;
      if (type == 4 && (int)((rec >> 12) & 7u) >= r.nR) f |= HSAD_POS_LASTMOVE;
      if (((rec >> 18) & 31u) >> H) f |= HSAD_POS_LASTMOVE;
    } else {
      if ((int)((rec >> 15) & 7u) >= H) f |= HSAD_POS_LASTMOVE;
      if ((int)((rec >> 23) & 7u) >= r.nC || (int)((rec >> 26) & 7u) >= r.nR) f |= HSAD_POS_LASTMOVE;
    }
  }

  // ---- colour permutations ----
  for (int p = 0; p < P; ++p) {
    const uint32_t pw = w[PLPERM(p)];
    bool ok = (pw >> 30) == 0u;
    uint32_t seen = 0;
    for (int c = 0; c < 5 && ok; ++c) {
      const uint32_t v = (pw >> (3 * c)) & 7u;
      if (v >= 5u || ((seen >> v) & 1u)) {
        ok = false;
        break;
      }
      seen |= 1u << v;
      if (((pw >> (15 + 3 * v)) & 7u) != (uint32_t)c) ok = false;   // the inverse
      if (c >= r.nC && v != (uint32_t)c) ok = false;                 // colours the rules do not use stay where they are
      if (!r.shuffle_color && v != (uint32_t)c) ok = false;
    }
    if (!ok) f |= HSAD_POS_PERM;
  }
  return f | (term ? (uint32_t)HSAD_POS_TERMINAL : 0u);
}

#endif  // HSAD_POSITION_H
