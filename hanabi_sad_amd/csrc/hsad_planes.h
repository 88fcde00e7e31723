// hsad_planes.h — the env's state planes: which plane holds what, the bit fields of every word and their accessors, and the
// policy's counter-based hash.  The one definition: hsad_env.hip and everything that reads an env's planes (hsad_rulebot.h,
// hsad_position.h, hsad_actor_partner.inc) take the layout from here.  Plain C++ (no HIP types, no allocation): included under
// hipcc by the kernels and under g++ by the stand-alone test programs of the headers above.
//
// State lives as struct-of-arrays planes of packed u32 bit-fields, game index fastest ([plane][G]); a game's words are plane
// PL_DECK_LO .. PL_LA1, then six words per player (PLH(p) .. PLPERM(p); these macros read the player count `P` of their scope).
#ifndef HSAD_PLANES_H
#define HSAD_PLANES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HSAD_PL_FN __host__ __device__ __forceinline__
#else
#define HSAD_PL_FN inline
#endif

// ---- state planes ---------------------------------------------------------------------------
enum : int {
  PL_DECK_LO = 0,  // deck counts, 2 bits per card type (colour*5+rank), types 0..15
  PL_DECK_HI = 1,  // types 16..24
  PL_DISC_LO = 2,  // discard counts, same packing
  PL_DISC_HI = 3,
  PL_BOARD = 4,   // fireworks 5x3b [0..14] | info [15..18] | life [19..20] | turns_to_play [21..23]
                  // | cur_player+1 [24..26] | next_non_chance_player [27..29]
  PL_MISC = 5,    // num_step [0..7] | deck_size [8..13] | term [14] | started [15] | last_score+1 [16..21]
                  // | la_n [22..23] = number of buffered look-ahead RNG outputs
  PL_LASTMV = 6,  // newest non-deal move: type[0..2] player[3..5] target_off[6..8] colour[9..11]
                  // rank[12..14] card_index[15..17] reveal_mask[18..22] card_colour[23..25]
                  // card_rank[26..28] scored[29] info_token[30]
  PL_DRAWS = 7,   // raw mt19937 draws consumed so far (logical; memory is la_n draws ahead)
  PL_LA0 = 8,     // look-ahead: the next two tempered mt19937 outputs, regenerated off the critical path
  PL_LA1 = 9,
  PL_FIXED = 10
};
// then per player p: HAND(p) cards 5x5b [0..24] | len [25..27];  KCP(p) colour-plausible 5x5b;
// KRP(p) rank-plausible 5x5b;  KH(p) hints 5x6b (hinted colour+1 [0..2], hinted rank+1 [3..5]);
// EPS(p) float bits;  PERM(p) colour perm 5x3b [0..14] | inverse perm [15..29]
#define PLH(p) (PL_FIXED + (p))
#define PLKCP(p) (PL_FIXED + P + (p))
#define PLKRP(p) (PL_FIXED + 2 * P + (p))
#define PLKH(p) (PL_FIXED + 3 * P + (p))
#define PLEPS(p) (PL_FIXED + 4 * P + (p))
#define PLPERM(p) (PL_FIXED + 5 * P + (p))

// count of card type t in a packed deck / discard pile / pool
HSAD_PL_FN uint32_t cnt2(uint64_t bits, int t) { return (uint32_t)(bits >> (2 * t)) & 3u; }

// ---- PL_BOARD ----
HSAD_PL_FN int board_fw(uint32_t b, int c) { return (b >> (3 * c)) & 7; }
HSAD_PL_FN int board_fw_sum(uint32_t b) {
  return board_fw(b, 0) + board_fw(b, 1) + board_fw(b, 2) + board_fw(b, 3) + board_fw(b, 4);
}
HSAD_PL_FN int board_info(uint32_t b) { return (b >> 15) & 15; }
HSAD_PL_FN int board_life(uint32_t b) { return (b >> 19) & 3; }
HSAD_PL_FN int board_turns(uint32_t b) { return (b >> 21) & 7; }
HSAD_PL_FN int board_cur(uint32_t b) { return (int)((b >> 24) & 7) - 1; }
HSAD_PL_FN int board_next(uint32_t b) { return (b >> 27) & 7; }
HSAD_PL_FN uint32_t board_set(uint32_t b, int shift, uint32_t mask, uint32_t v) {
  return (b & ~(mask << shift)) | (v << shift);
}

// ---- PL_MISC ----
HSAD_PL_FN int misc_num_step(uint32_t m) { return (int)(m & 255u); }
HSAD_PL_FN int misc_deck_size(uint32_t m) { return (int)((m >> 8) & 63u); }
HSAD_PL_FN bool misc_term(uint32_t m) { return (m >> 14) & 1u; }
HSAD_PL_FN bool misc_started(uint32_t m) { return (m >> 15) & 1u; }
HSAD_PL_FN int misc_last_score(uint32_t m) { return (int)((m >> 16) & 63u) - 1; }
HSAD_PL_FN int misc_la_n(uint32_t m) { return (int)((m >> 22) & 3u); }
// a game the kernels step: started and not terminated
HSAD_PL_FN bool misc_live(uint32_t m) { return misc_started(m) && !misc_term(m); }

// ---- counter-based random-legal policy ---------------------------------------------------------
HSAD_PL_FN uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
HSAD_PL_FN uint32_t policy_hash(uint64_t seed, uint64_t game, uint64_t counter, uint64_t stream) {
  const uint64_t k = mix64(seed ^ mix64(game * 0xD1342543DE82EF95ull + stream));
  return (uint32_t)(mix64(k + counter) >> 32);
}

#endif  // HSAD_PLANES_H
