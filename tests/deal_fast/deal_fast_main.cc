// csrc/hsad_deal_fast.h against the scans it replaces, restated here: the 25-step cumulative scan of deal_pick, the clear-lowest-bit
// loop of policy_pick and `% 624`.  Stand-alone (built with -fsanitize=address,undefined by tests/test_deal_fast_cpu.py); prints the
// number of cases of each kind, exits 1 at the first disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hsad_deal_fast.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static uint32_t cnt2(uint64_t deck, int t) { return (uint32_t)(deck >> (2 * t)) & 3u; }

static uint64_t full_deck() {
  const int cnt[5] = {3, 2, 2, 2, 1};
  uint64_t d = 0;
  for (int c = 0; c < 5; ++c)
    for (int r = 0; r < 5; ++r) d |= (uint64_t)cnt[r] << (2 * (c * 5 + r));
  return d;
}

static int deck_size(uint64_t deck) {
  int n = 0;
  for (int t = 0; t < 25; ++t) n += (int)cnt2(deck, t);
  return n;
}

// deal_pick's scan: the first type whose cumulative count reaches need
static int scan_pick(uint64_t deck, uint32_t need) {
  uint32_t acc = 0;
  int pick = -1;
  for (int t = 0; t < 25; ++t) {
    acc += cnt2(deck, t);
    if (pick < 0 && acc >= need) pick = t;
  }
  return pick;
}

static long n_decks = 0, n_picks = 0;
static bool seen_size[51];

static void check_deck(uint64_t deck, const char* what) {
  const int D = deck_size(deck);
  if (D < 1 || D > 50) {
    printf("the test's own deck has %d cards (%s)\n", D, what);
    exit(1);
  }
  seen_size[D] = true;
  ++n_decks;
  for (uint32_t need = 1; need <= (uint32_t)D; ++need) {
    const int want = scan_pick(deck, need), got = df_pick(deck, need);
    ++n_picks;
    if (got != want || cnt2(deck, got) == 0u) {
      printf("df_pick(%016llx, %u) = %d, the scan gives %d (%s)\n", (unsigned long long)deck, need, got, want, what);
      exit(1);
    }
  }
}

static uint64_t remove_random(uint64_t deck, int target) {
  int D = deck_size(deck);
  while (D > target) {
    int k = (int)(rnd() % (uint64_t)D);   // the k-th remaining card
    for (int t = 0; t < 25; ++t) {
      const int c = (int)cnt2(deck, t);
      if (k < c) {
        deck -= (uint64_t)1 << (2 * t);
        break;
      }
      k -= c;
    }
    --D;
  }
  return deck;
}

static int naive_select(uint64_t mask, uint32_t k) {
  uint64_t m = mask;
  while (k-- > 0) m &= m - 1;
  return __builtin_ctzll(m);
}

static long n_masks = 0, n_selects = 0;

static void check_mask(uint64_t mask, int nbits) {
  if (mask == 0) return;
  ++n_masks;
  const uint32_t n = (uint32_t)__builtin_popcountll(mask);
  for (uint32_t k = 0; k < n; ++k) {
    const int want = naive_select(mask, k);
    const int got = df_select(mask, k, nbits), got64 = df_select(mask, k);
    ++n_selects;
    if (got != want || got64 != want) {
      printf("df_select(%016llx, %u, %d) = %d / %d, the loop gives %d\n", (unsigned long long)mask, k, nbits, got, got64, want);
      exit(1);
    }
  }
}

int main() {
  const uint64_t full = full_deck();
  // hand-written decks: the full one; one type left (every type, every count it can have: sizes 1..3); every type once where the
  // full deck has it, and that with the lowest / highest types taken away down to two cards
  check_deck(full, "full");
  for (int t = 0; t < 25; ++t)
    for (uint32_t c = 1; c <= cnt2(full, t); ++c) check_deck((uint64_t)c << (2 * t), "one type left");
  uint64_t ones = 0;
  for (int t = 0; t < 25; ++t) ones |= (uint64_t)1 << (2 * t);
  check_deck(ones, "all counts 1");
  for (int t = 0; t < 23; ++t) {
    check_deck(ones & ~(((uint64_t)1 << (2 * t + 2)) - 1), "all counts 1, low types gone");
    check_deck(ones & (((uint64_t)1 << (50 - 2 * t)) - 1), "all counts 1, high types gone");
  }
  check_deck(((uint64_t)3 << 0) | ((uint64_t)1 << 48), "first and last type");
  check_deck(((uint64_t)2 << 30) | ((uint64_t)2 << 32), "types 15 and 16: the word boundary");
  // random decks of every size 2..50 (230 each: 11,270), by drawing cards from the full deck; half of them from the all-ones deck
  // where the size allows, so that count-1 remainders are common
  for (int size = 2; size <= 50; ++size)
    for (int rep = 0; rep < 230; ++rep) {
      const bool from_ones = (rep & 1) && size <= 25;
      check_deck(remove_random(from_ones ? ones : full, size), from_ones ? "random, counts 1" : "random");
    }
  for (int size = 2; size <= 50; ++size)
    if (!seen_size[size]) {
      printf("no deck of size %d\n", size);
      return 1;
    }

  // select: random masks of every density, then masks below the action counts of the supported games (A - 1 = 20 / 30 / 38 / 49)
  for (int rep = 0; rep < 4000; ++rep) {
    check_mask(rnd(), 64);
    check_mask(rnd() & rnd(), 64);
    check_mask(rnd() | rnd(), 64);
    check_mask(rnd() & rnd() & rnd() & rnd(), 64);
  }
  check_mask(~0ull, 64);
  for (int b = 0; b < 64; ++b) check_mask((uint64_t)1 << b, 64);
  const int widths[4] = {20, 30, 38, 49};
  for (int wi = 0; wi < 4; ++wi) {
    const uint64_t below = ((uint64_t)1 << widths[wi]) - 1;
    check_mask(below, widths[wi]);
    check_mask(below, widths[wi] + 1);
    for (int rep = 0; rep < 2000; ++rep) {
      check_mask(rnd() & below, widths[wi]);
      check_mask(rnd() & rnd() & below, widths[wi] + 1);   // the bound a kernel passes counts the noop move as well
    }
  }

  // wrapped window index
  long n_wrap = 0;
  for (uint32_t b = 0; b < 624; ++b)
    for (uint32_t j = 0; j <= 64 + 397; ++j, ++n_wrap)
      if (df_wrap624(b, j) != (b + j) % 624u) {
        printf("df_wrap624(%u, %u) = %u\n", b, j, df_wrap624(b, j));
        return 1;
      }
  printf("decks %ld picks %ld masks %ld selects %ld wraps %ld\n", n_decks, n_picks, n_masks, n_selects, n_wrap);
  return 0;
}
