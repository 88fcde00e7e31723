// hsad_hand_count.h — exact integer arithmetic on the belief over a hidden Hanabi hand: how many assignments of physical unseen cards
// to the hand's slots agree with the per-slot card knowledge, the per-slot marginals of that count, and the unranking map
// rank -> hand that gives every hand exactly its weight.  Plain C++ (no HIP types, no recursion, no allocation): the kernels of
// hsad_env_search.inc include it under hipcc, tests/hand_count/hand_count_main.cc under g++.  Specification: include/hsad.h,
// hsad_env_hand_belief / hsad_env_determinize_exact; DESIGN.md section 3g.
//
// Representation: card type t = colour * 5 + rank < 25; the pool (deck + the viewer's hand) packed two bits per type in a
// uint64_t; per slot a 25-bit mask, bit t = type t is colour- and rank-plausible for the slot.  At most HC_MAX_SLOTS slots; a set of
// slots is a bit mask below 32.
//
// Count: C({}, q) = 1;  C(S, q) = sum over B subset of S with min(S) in B of (-1)^(|B|-1) (|B|-1)! s_B(q) C(S \ B, q), where
// s_B(q) = number of cards of q plausible for every slot of B (Moebius inversion on the partition lattice: the B's are the blocks
// of "these slots were given the same physical card").  Every term stays below 2^35 in magnitude and C below 2^28 (five slots,
// fifty cards), so int64_t is exact.
#ifndef HSAD_HAND_COUNT_H
#define HSAD_HAND_COUNT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HSAD_HC_FN __host__ __device__ inline
#else
#define HSAD_HC_FN inline
#endif

#define HC_MAX_SLOTS 5
#define HC_TYPES 25
#define HC_SUBSETS 32

// per set of slots B (index = bit mask; entry 0 unused): and[B] = AND of the slots' masks, s[B] = s_B(q)
struct HcTables {
  uint32_t and_mask[HC_SUBSETS];
  int64_t s[HC_SUBSETS];
};

HSAD_HC_FN uint32_t hc_cnt(uint64_t q, int t) { return (uint32_t)(q >> (2 * t)) & 3u; }

HSAD_HC_FN uint32_t hc_and_mask(const uint32_t* cm, uint32_t B) {
  uint32_t m = 0x1ffffffu;
  for (int i = 0; i < HC_MAX_SLOTS; ++i)
    if ((B >> i) & 1u) m &= cm[i];
  return m;
}

HSAD_HC_FN int64_t hc_weight(uint64_t q, uint32_t mask) {
  int64_t z = 0;
  for (int t = 0; t < HC_TYPES; ++t) z += ((mask >> t) & 1u) ? (int64_t)hc_cnt(q, t) : 0;
  return z;
}

// the entries of every non-empty subset of S
HSAD_HC_FN void hc_tables(uint64_t q, const uint32_t* cm, uint32_t S, HcTables* T) {
  for (uint32_t B = 1; B < HC_SUBSETS; ++B) {
    if (B & ~S) continue;
    T->and_mask[B] = hc_and_mask(cm, B);
    T->s[B] = hc_weight(q, T->and_mask[B]);
  }
}

// C(S, q - e_t) from the tables of q (t < 0: C(S, q)); s_B(q - e_t) = s_B(q) - [t plausible for every slot of B].  The table over
// the subsets of S is filled in increasing order: S \ B is a smaller number than S.
HSAD_HC_FN int64_t hc_count(const uint32_t* and_mask, const int64_t* s, uint32_t S, int t) {
  int64_t C[HC_SUBSETS];
  C[0] = 1;
  for (uint32_t sub = 1; sub <= S; ++sub) {
    if (sub & ~S) continue;
    const uint32_t low = sub & (0u - sub), rest = sub ^ low;
    int64_t acc = 0;
    uint32_t b = rest;   // B = low | b, b over the subsets of rest
    for (;;) {
      const uint32_t B = low | b;
      int k = 0;
      for (int i = 0; i < HC_MAX_SLOTS; ++i) k += (int)((B >> i) & 1u);
      int64_t coef = 1;   // (-1)^(k-1) (k-1)!
      for (int j = 2; j < k; ++j) coef *= j;
      if (!(k & 1)) coef = -coef;
      const int64_t sb = s[B] - (t >= 0 ? (int64_t)((and_mask[B] >> t) & 1u) : 0);
      acc += coef * sb * C[sub ^ B];
      if (b == 0u) break;
      b = (b - 1u) & rest;
    }
    C[sub] = acc;
  }
  return C[S];
}

HSAD_HC_FN uint32_t hc_all_slots(int n) { return (1u << n) - 1u; }

// N = the number of assignments for slots 0 .. n-1
HSAD_HC_FN int64_t hc_total(uint64_t pool, const uint32_t* cm, int n) {
  HcTables T;
  hc_tables(pool, cm, hc_all_slots(n), &T);
  return hc_count(T.and_mask, T.s, hc_all_slots(n), -1);
}

// num[i][t] = pool[t] compat_i[t] C(all \ {i}, pool - e_t), from the tables of the pool over all n slots
HSAD_HC_FN int64_t hc_marginal(const uint32_t* and_mask, const int64_t* s, uint64_t pool, const uint32_t* cm, int n, int i, int t) {
  const uint32_t c = hc_cnt(pool, t);
  if (c == 0u || !((cm[i] >> t) & 1u)) return 0;
  return (int64_t)c * hc_count(and_mask, s, hc_all_slots(n) & ~(1u << i), t);
}

// the class of EncodeOwnHandTrinary for a card of rank r on a firework of height fw: 0 playable, 1 below, 2 above
HSAD_HC_FN int hc_trinary_class(int r, int fw) { return r == fw ? 0 : (r < fw ? 1 : 2); }

// rank r in [0, N) -> the hand (5 bits per slot in *cards, slot order) and the pool that is left (*q_out).  Slot by slot, types
// ascending: type t takes the next q[t] * C(slots after i, q - e_t) ranks.  Returns 0 (nothing written) when r is outside [0, N).
HSAD_HC_FN int hc_unrank(uint64_t pool, const uint32_t* cm, int n, int64_t r, uint32_t* cards, uint64_t* q_out) {
  if (r < 0) return 0;
  uint64_t q = pool;
  uint32_t hand = 0;
  HcTables T;
  for (int i = 0; i < n; ++i) {
    const uint32_t rem = hc_all_slots(n) & ~((2u << i) - 1u);
    hc_tables(q, cm, rem, &T);
    int card = -1;
    for (int t = 0; t < HC_TYPES && card < 0; ++t) {
      const uint32_t cnt = hc_cnt(q, t);
      if (cnt == 0u || !((cm[i] >> t) & 1u)) continue;
      const int64_t c = hc_count(T.and_mask, T.s, rem, t);
      const int64_t w = (int64_t)cnt * c;
      if (r < w) {
        card = t;
        r %= c;   // c > 0: r < w
      } else {
        r -= w;
      }
    }
    if (card < 0) return 0;
    q -= (uint64_t)1 << (2 * card);
    hand |= (uint32_t)card << (5 * i);
  }
  *cards = hand;
  *q_out = q;
  return 1;
}

// the rank world w of W draws from its stratum [lo, hi) of [0, N), lo = w N / W, hi = (w + 1) N / W:  lo + ((u * span) >> 64)
// for the 64-bit uniform u; lo when the stratum is empty.  N < 2^28, 0 <= w < W <= 2^20.  span < 2^28, so the high word of the
// 128-bit product is ((u >> 32) * span + (((u & 0xffffffff) * span) >> 32)) >> 32 without a wide multiply.
HSAD_HC_FN int64_t hc_stratum_rank(int64_t N, int64_t w, int64_t W, uint64_t u) {
  const int64_t lo = (w * N) / W, hi = ((w + 1) * N) / W;
  const uint64_t span = (uint64_t)(hi - lo);
  if (span == 0u) return lo;
  const uint64_t top = (u >> 32) * span + (((u & 0xffffffffull) * span) >> 32);
  return lo + (int64_t)(top >> 32);
}

#endif  // HSAD_HAND_COUNT_H
