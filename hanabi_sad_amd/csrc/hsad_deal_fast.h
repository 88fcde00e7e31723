// hsad_deal_fast.h — the three bounded searches of the env step's logic: which card type a deal's draw picks from the packed deck,
// which legal move a policy hash picks from a legal mask, and where a mt19937 word of the reset's prefetch window lies.  Each
// replaces a scan (25 steps over the deck, up to A - 1 trips over the mask) or a division (% 624) by a fixed, short chain of
// population counts or one compare.  Plain C++ (no HIP types, no loops that depend on data, no allocation): hsad_env.hip includes it
// under hipcc, tests/deal_fast/deal_fast_main.cc under g++.  Specification: the scans themselves, restated in that test.
//
// Representation: card type t = colour * 5 + rank < 25, the deck packed two bits per type (count 0..3) in a uint64_t, types 0..15
// in the low word; a legal mask has bit uid set for every legal move.
#ifndef HSAD_DEAL_FAST_H
#define HSAD_DEAL_FAST_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HSAD_DF_FN __host__ __device__ inline
#else
#define HSAD_DF_FN inline
#endif

HSAD_DF_FN uint32_t df_popc32(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// cards in the 2-bit count fields of w: popc(w & 0x55...) + 2 popc((w >> 1) & 0x55...)
HSAD_DF_FN uint32_t df_cards32(uint32_t w) { return df_popc32(w & 0x55555555u) + 2u * df_popc32(w & 0xaaaaaaaau); }

// The smallest type t whose cumulative count C_t = cards of types 0..t is >= need, for 1 <= need <= cards in the deck (what the
// 25-step scan of deal_pick returns; that type always has a card).  One step chooses the word, four halve the sixteen types in it:
// `w` holds the candidate types from its bit 0 up, `need` counts from the first of them.
HSAD_DF_FN int df_pick(uint64_t deck, uint32_t need) {
  uint32_t w = (uint32_t)deck;
  int t = 0;
  uint32_t c = df_cards32(w);
  if (c < need) {
    need -= c;
    w = (uint32_t)(deck >> 32);
    t = 16;
  }
#define HSAD_DF_STEP(HALF)                               \
  c = df_cards32(w & ((1u << (2 * (HALF))) - 1u));       \
  if (c < need) {                                        \
    need -= c;                                           \
    w >>= 2 * (HALF);                                    \
    t += (HALF);                                         \
  }
  HSAD_DF_STEP(8)
  HSAD_DF_STEP(4)
  HSAD_DF_STEP(2)
  HSAD_DF_STEP(1)
#undef HSAD_DF_STEP
  return t;
}

// Position of the k-th set bit of mask (k = 0: the lowest), for k < popcount(mask): what `while (k-- > 0) m &= m - 1; ctz(m)`
// returns.  nbits: a bound on the mask's width known where the call is compiled (bits nbits.. are clear); 32 or less drops the
// step that chooses the word.
HSAD_DF_FN int df_select(uint64_t mask, uint32_t k, int nbits = 64) {
  uint32_t w = (uint32_t)mask;
  int pos = 0;
  uint32_t c;
  if (nbits > 32) {
    c = df_popc32(w);
    if (c <= k) {
      k -= c;
      w = (uint32_t)(mask >> 32);
      pos = 32;
    }
  }
#define HSAD_DF_STEP(HALF)                       \
  c = df_popc32(w & ((1u << (HALF)) - 1u));      \
  if (c <= k) {                                  \
    k -= c;                                      \
    w >>= (HALF);                                \
    pos += (HALF);                               \
  }
  HSAD_DF_STEP(16)
  HSAD_DF_STEP(8)
  HSAD_DF_STEP(4)
  HSAD_DF_STEP(2)
  HSAD_DF_STEP(1)
#undef HSAD_DF_STEP
  return pos;
}

// (b + j) % 624 for b < 624 and j <= 624: the indices of the reset's window, j <= 64 + 397, wrap at most once
HSAD_DF_FN uint32_t df_wrap624(uint32_t b, uint32_t j) {
  const uint32_t i = b + j;
  return i >= 624u ? i - 624u : i;
}

#endif  // HSAD_DEAL_FAST_H
