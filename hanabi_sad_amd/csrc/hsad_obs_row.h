// hsad_obs_row.h — one observer's observation bit row of the full game, assembled in registers at fixed bit positions and placed
// into the LDS bit rows with one shift.  build_rows (hsad_env.hip) places every field at a run-time bit position `base + offset`:
// a word index, a 64-bit variable shift and up to three LDS atomics per field.  For a fixed (P, H) and the full rules every offset
// within a row is a compile-time constant; only the row's own base varies per lane.  So obs_row_assemble ORs every field into a
// register image of the row that starts at bit 0 (constant shifts into constant words), and obs_row_place funnel-shifts that image
// by base & 31 and ORs it into the rows, one atomic per word.  Plain C++ (no HIP types, no allocation; every loop has constant
// bounds and is unrolled, so that row[] is only ever indexed by constants and stays in registers): hsad_env.hip includes it under
// hipcc, tests/obs_row/obs_row_main.cc under g++.  Specification: the scatter form of build_rows, restated in that test.
//
// The bits are those of build_rows for every state the game can reach.  What this relies on, and build_rows does not: a hand's
// length is at most H, discard counts are at most the deck's (3, 2, 2, 2, 1 per colour), the deck size is at most 50 - P * H,
// fireworks at most 5, information tokens at most 8, hinted colour / rank at most 5, `pm` (15 bits) is a permutation of the five
// colours, and a move record's
// fields are in range: a field never reaches past its section.
#ifndef HSAD_OBS_ROW_H
#define HSAD_OBS_ROW_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HSAD_OR_FN __host__ __device__ __forceinline__
#else
#define HSAD_OR_FN inline
#endif

// the sections of a row (hsad_env_create computes the same offsets at run time for EnvParams)
template <int P, int H>
struct ObsRowGeom {
  static constexpr int C = 5, R = 5, CR = 25, KS = 35, DW = 10, MI = 8, ML = 3, DECK = 50;
  static constexpr int MISS = P * H * CR;                     // cards of the P hands, then the P missing-card bits
  static constexpr int OB = MISS + P;                         // deck thermometer
  static constexpr int DECKW = DECK - P * H;
  static constexpr int OFW = OB + DECKW;                      // fireworks | information | life
  static constexpr int OD = OFW + CR + MI + ML;               // discards
  static constexpr int LAL = P + 4 + P + C + R + H + H + CR + 2;
  static constexpr int OL = OD + DECK;                        // last action
  static constexpr int OK = OL + LAL;                         // card knowledge
  static constexpr int F0 = OK + P * H * KS;                  // width without SAD; the greedy action's section with it
  static constexpr int FS = F0 + LAL;
  static constexpr int NW = (FS + 31) / 32;                   // words of row[]: sized for the SAD width
  static_assert(LAL <= 64 && DECKW <= 64, "a section is placed as one 64-bit value");
};

// a row's register image
template <int P, int H>
using ObsRow = uint32_t[ObsRowGeom<P, H>::NW];

constexpr uint32_t kObsIdentityPerm = (0u) | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12);

// v (bits at and above `width` clear) into the row at bit `pos`; pos and width are constants where the call is compiled
template <int NW>
HSAD_OR_FN void obs_put(uint32_t (&row)[NW], const int pos, const int width, uint64_t v) {
  const int w = pos >> 5, s = pos & 31;
  row[w] |= (uint32_t)(v << s);
  if (s + width > 32) row[w + 1] |= (uint32_t)(v >> (32 - s));
  if (s + width > 64) row[w + 2] |= (uint32_t)(v >> (64 - s));
}

// a move record (PL_LASTMV layout) as the LAL bits of the last-action section, for `observer`: encode_last_action of hsad_env.hip
template <int P, int H>
HSAD_OR_FN uint64_t obs_last_action(uint32_t rec, int observer, uint32_t pm) {
  const int type = (int)(rec & 7u);
  if (!type) return 0;
  int rel = (int)((rec >> 3) & 7u) - observer;
  if (rel < 0) rel += P;
  uint64_t m = 1ull << rel;
  m |= 1ull << (P + type - 1);
  if (type >= 3) {
    int tgt = rel + (int)((rec >> 6) & 7u);
    if (tgt >= P) tgt -= P;
    m |= 1ull << (P + 4 + tgt);
    m |= (uint64_t)((rec >> 18) & 31u) << (2 * P + 14);
  } else {
    m |= 1ull << (2 * P + 14 + H + ((rec >> 15) & 7u));
    m |= 1ull << (2 * P + 14 + 2 * H + ((pm >> (3u * ((rec >> 23) & 7u))) & 7u) * 5u + ((rec >> 26) & 7u));
  }
  if (type == 3) m |= 1ull << (2 * P + 4 + ((pm >> (3u * ((rec >> 9) & 7u))) & 7u));
  if (type == 4) m |= 1ull << (2 * P + 9 + ((rec >> 12) & 7u));
  if (type == 1) m |= (uint64_t)((rec >> 29) & 3u) << (2 * P + 39 + 2 * H);
  return m;
}

// discard thermometers of all 25 card types at once, identity colours: type t's 2-bit count n at bit 2t of disc becomes
// (1 << n) - 1 at 10 * colour + {0, 3, 5, 7, 9}[rank].  n >= 1, >= 2, >= 3 are lo | hi, hi, lo & hi of the count's two bits.
HSAD_OR_FN uint64_t obs_discards_identity(uint64_t disc) {
  const uint64_t r0 = 0x0000010040100401ull;     // rank 0 of each colour: bits 0, 10, 20, 30, 40
  const uint64_t k5 = 0x155ull * r0;             // bit 0 of each of the 25 counts
  const uint64_t r13 = 0x054ull * r0;            // ranks 1..3: bits 2, 4, 6 of each group of ten
  const uint64_t r14 = 0x154ull * r0;            // ranks 1..4
  const uint64_t lo = disc & k5, hi = (disc >> 1) & k5;
  const uint64_t ge1 = lo | hi, ge2 = hi, ge3 = lo & hi;
  return (ge1 & r0) | ((ge1 & r14) << 1) | ((ge2 & r0) << 1) | ((ge2 & r13) << 2) | ((ge3 & r0) << 2);
}

// The observer's row, from bit 0.  board, misc, disc, lastmv, greedy: the game's PL_BOARD, PL_MISC, PL_DISC_LO/HI, PL_LASTMV words
// and its greedy move record.  hand, kcp, krp, kh: the PLH, PLKCP, PLKRP, PLKH words of the players in the observer's order:
// index o is player (p + o) % P.  pm: the observer's colour permutation (the low 15 bits of PLPERM, or the identity).
template <int P, int H>
HSAD_OR_FN void obs_row_assemble(ObsRow<P, H>& row, uint32_t board, uint32_t misc, uint64_t disc, uint32_t lastmv,
                                 uint32_t greedy, const uint32_t (&hand)[P], const uint32_t (&kcp)[P], const uint32_t (&krp)[P],
                                 const uint32_t (&kh)[P], int p, uint32_t pm, bool sad) {
  using Ge = ObsRowGeom<P, H>;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < Ge::NW; ++k) row[k] = 0u;
  uint32_t pmc[5], sh5[5];   // pm[c], and where colour c's five ranks go: 5 * pm[c]
#if defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < 5; ++c) {
    pmc[c] = (pm >> (3 * c)) & 7u;
    sh5[c] = 5u * pmc[c];
  }
  // What the colours' order touches beyond a shift by sh5 is worked out for the identity and reordered in one place, which the
  // lanes of an env without colour shuffling all skip: the colour-plausible bits of a hand's cards (kc), the one-hot of a hinted
  // colour (hint_tab: five bits per value of hinted colour + 1, none for 0) and the discards' groups of ten (dm).
  uint32_t len[P], kc[P];
#if defined(__clang__)
#pragma unroll
#endif
  for (int o = 0; o < P; ++o) {
    len[o] = (hand[o] >> 25) & 7u;
    // the words of the cards the hand no longer has contribute nothing: colour-plausible 0 makes the plausibility mask 0
    kc[o] = kcp[o] & ((1u << (5u * len[o])) - 1u);
  }
  uint32_t hint_tab = (1u << 5) | (2u << 10) | (4u << 15) | (8u << 20) | (16u << 25);
  uint64_t dm = obs_discards_identity(disc);
  if (pm != kObsIdentityPerm) {
    const uint32_t each = 1u | (1u << 5) | (1u << 10) | (1u << 15) | (1u << 20);   // one bit of each of a hand's five cards
#if defined(__clang__)
#pragma unroll
#endif
    for (int o = 0; o < P; ++o) {
      uint32_t t = 0;
#if defined(__clang__)
#pragma unroll
#endif
      for (int c = 0; c < 5; ++c) t |= ((kc[o] >> c) & each) << pmc[c];
      kc[o] = t;
    }
    hint_tab = 0;
    uint64_t t = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int c = 0; c < 5; ++c) {
      hint_tab |= (1u << (5 * (c + 1))) << pmc[c];
      t |= ((dm >> (10 * c)) & 1023ull) << (2u * sh5[c]);   // colour c's ten bits to where pm sends them
    }
    dm = t;
  }

  uint32_t miss = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int o = 0; o < P; ++o) {
    const uint32_t hw = hand[o];
    miss |= (len[o] < (uint32_t)H ? 1u : 0u) << o;
    const uint32_t kr = krp[o], kk = kh[o] & ((1u << (6u * len[o])) - 1u);
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < H; ++i) {
      if (o > 0) {
        const uint32_t card = (hw >> (5 * i)) & 31u;
        const uint32_t c = (card * 13u) >> 6;
        const uint32_t pos = card + 5u * ((pm >> (3u * c)) & 7u) - 5u * c;   // pm[c] * 5 + rank
        obs_put(row, (o * H + i) * Ge::CR, Ge::CR, (uint32_t)i < len[o] ? 1u << pos : 0u);
      }
      const uint32_t cp = (kc[o] >> (5 * i)) & 31u, rp = (kr >> (5 * i)) & 31u, h6 = (kk >> (6 * i)) & 63u;
      // bit 5 * c for every plausible (reordered) colour c: the low four through copies four bits apart, which do not overlap;
      // times rp (< 32: no carries) = rp at each of them
      const uint32_t spread = (((cp & 15u) * 0x1111u) & 0x8421u) | ((cp & 16u) << 16);
      const uint32_t hint = ((hint_tab >> (5u * (h6 & 7u))) & 31u) | (((1u << (h6 >> 3)) >> 1) << 5);
      obs_put(row, Ge::OK + (o * H + i) * Ge::KS, Ge::KS, (uint64_t)(rp * spread) | ((uint64_t)hint << Ge::CR));
    }
  }
  obs_put(row, Ge::MISS, P, miss);
  obs_put(row, Ge::OB, Ge::DECKW, (1ull << ((misc >> 8) & 63u)) - 1ull);
  uint32_t fw = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < 5; ++c) fw |= ((1u << ((board >> (3 * c)) & 7u)) >> 1) << sh5[c];
  obs_put(row, Ge::OFW, Ge::CR, fw);
  const uint32_t info = (board >> 15) & 15u, life = (board >> 19) & 3u;
  obs_put(row, Ge::OFW + Ge::CR, Ge::MI + Ge::ML, ((1u << info) - 1u) | (((1u << life) - 1u) << Ge::MI));
  obs_put(row, Ge::OD, Ge::DECK, dm);
  obs_put(row, Ge::OL, Ge::LAL, obs_last_action<P, H>(lastmv, p, pm));
  if (sad) obs_put(row, Ge::F0, Ge::LAL, obs_last_action<P, H>(greedy, p, pm));
}

// ({hi, lo} >> sh) & 0xffffffff for sh < 32: one funnel shift
HSAD_OR_FN uint32_t obs_funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, sh);   // (the plain form below compiles to a 64-bit shift of a register pair)
#endif
  return (uint32_t)((((uint64_t)hi << 32) | (uint64_t)lo) >> (sh & 31u));
}

// row[k] for a constant k, 0 behind the row
template <int NW>
HSAD_OR_FN uint32_t obs_at(const uint32_t (&row)[NW], const int k) {
  return k < NW ? row[k < NW ? k : 0] : 0u;
}

// OR the row into the bit rows `bits` at bit `base` (the row's F bits: F0 or FS with sad).  Word k of the shifted image is the
// funnel {row[k], row[k-1]} >> ((32 - s) & 31) and goes to word w + k, where s = base & 31 and w = base >> 5; with s = 0 that
// funnel yields row[k-1], so there the image is written one word lower (wb = w - 1).  Only words the row has bits in are touched:
// image words 1 .. F >> 5 lie within the row whatever s is, and the one behind them, which holds bits only when s + F crosses a
// word boundary and is 0 otherwise, goes to the row's last word at the latest.
template <int P, int H, class OrFn>
HSAD_OR_FN void obs_row_place(const ObsRow<P, H>& row, uint32_t base, bool sad, OrFn or_word) {
  using Ge = ObsRowGeom<P, H>;
  constexpr int K0 = Ge::F0 >> 5, K1 = Ge::FS >> 5;   // image words 1..F >> 5 lie within the row whatever s is
  const uint32_t s = base & 31u, sh = (32u - s) & 31u;
  const uint32_t wb = (base >> 5) - (s == 0u ? 1u : 0u);
  const uint32_t last = (base + (uint32_t)(sad ? Ge::FS : Ge::F0) - 1u) >> 5;
  // the observer's own cards are not in the row: its first Z words are 0 and are left out (an OR of a constant 0 is not free:
  // it compiles to an atomic load)
  constexpr int Z = (H * Ge::CR) >> 5;
  static_assert(Z >= 1 && Z < K0, "the first image word written is an interior one");
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = Z; k <= K0; ++k) or_word(wb + k, obs_funnel(obs_at(row, k), k > Z ? obs_at(row, k - 1) : 0u, sh));
  if (sad) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = K0 + 1; k <= K1; ++k) or_word(wb + k, obs_funnel(obs_at(row, k), obs_at(row, k - 1), sh));
    const uint32_t x = wb + K1 + 1;
    or_word(x < last ? x : last, obs_funnel(obs_at(row, K1 + 1), obs_at(row, K1), sh));
  } else {
    const uint32_t x = wb + K0 + 1;
    or_word(x < last ? x : last, obs_funnel(obs_at(row, K0 + 1), obs_at(row, K0), sh));
  }
}

#endif  // HSAD_OBS_ROW_H
