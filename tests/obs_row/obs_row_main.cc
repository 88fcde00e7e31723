// csrc/hsad_obs_row.h against the scatter form it replaces, restated here: build_rows' observation part, every field ORed into a
// zeroed word array at the run-time bit position base + offset (or_bit / or_bits32 / or_bits64), with the section offsets worked out
// at run time the way hsad_env_create does.  For every fixed (P, H) instance, sad 0 / 1, identity and shuffled colours:
// obs_row_assemble + obs_row_place word for word against that form, and no word touched that the row has no bit in.  Stand-alone
// (built with -fsanitize=address,undefined by tests/test_obs_row_cpu.py); prints its counts, exits 1 at the first disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hsad_obs_row.h"

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

// ---- the specification ---------------------------------------------------------------------------------------------------------
static void or_bit(uint32_t* b, uint32_t pos) { b[pos >> 5] |= 1u << (pos & 31); }
static void or_bits32(uint32_t* b, uint32_t pos, uint32_t val) {
  const uint32_t w = pos >> 5, s = pos & 31;
  const uint64_t v = (uint64_t)val << s;
  b[w] |= (uint32_t)v;
  b[w + 1] |= (uint32_t)(v >> 32);
}
static void or_bits64(uint32_t* b, uint32_t pos, uint64_t val) {
  const uint32_t w = pos >> 5, s = pos & 31;
  const uint64_t lo = val << s;
  b[w] |= (uint32_t)lo;
  b[w + 1] |= (uint32_t)(lo >> 32);
  b[w + 2] |= ((uint32_t)(val >> 32) >> (31u - s)) >> 1;
}
static uint32_t perm_c(uint32_t pm, int c) { return (pm >> (3 * c)) & 7u; }
static uint32_t cnt2(uint64_t bits, int t) { return (uint32_t)(bits >> (2 * t)) & 3u; }

struct State {
  uint32_t board, misc, lastmv, greedy;
  uint64_t disc;
  uint32_t hand[5], kcp[5], krp[5], kh[5];   // by player
};
struct Geom {
  int P, H, F, F0, LAL, OB, OD, OL, OK, DECKW;
};
static Geom geom_of(int P, int H, int sad) {   // hsad_env_create, full rules
  Geom g;
  g.P = P;
  g.H = H;
  g.DECKW = 50 - P * H;
  g.LAL = P + 4 + P + 5 + 5 + H + H + 25 + 2;
  g.OB = P * H * 25 + P;
  g.OD = g.OB + g.DECKW + 25 + 8 + 3;
  g.OL = g.OD + 50;
  g.OK = g.OL + g.LAL;
  g.F0 = g.OK + P * H * 35;
  g.F = g.F0 + (sad ? g.LAL : 0);
  return g;
}

static uint64_t encode_last_action(int P, int H, uint32_t rec, int observer, uint32_t pm) {
  const int type = rec & 7;
  if (!type) return 0;
  int rel = (int)((rec >> 3) & 7) - observer;
  if (rel < 0) rel += P;
  uint64_t m = 1ull << rel;
  int off = P;
  m |= 1ull << (off + type - 1);
  off += 4;
  if (type >= 3) {
    int tgt = rel + (int)((rec >> 6) & 7);
    if (tgt >= P) tgt -= P;
    m |= 1ull << (off + tgt);
  }
  off += P;
  if (type == 3) m |= 1ull << (off + perm_c(pm, (rec >> 9) & 7));
  off += 5;
  if (type == 4) m |= 1ull << (off + ((rec >> 12) & 7));
  off += 5;
  if (type >= 3) m |= (uint64_t)((rec >> 18) & 31u) << off;
  off += H;
  if (type <= 2) m |= 1ull << (off + ((rec >> 15) & 7));
  off += H;
  if (type <= 2) m |= 1ull << (off + perm_c(pm, (rec >> 23) & 7) * 5 + ((rec >> 26) & 7));
  off += 25;
  if (type == 1) m |= (uint64_t)((rec >> 29) & 3u) << off;
  return m;
}

static void scatter_row(const Geom& ge, const State& st, int p, uint32_t pm, int sad, uint32_t* s_obs, uint32_t base) {
  const int P = ge.P, H = ge.H;
  const uint32_t CR = 25, RR = 5;
  const int deck_size = (st.misc >> 8) & 63;
  const int info = (st.board >> 15) & 15, life = (st.board >> 19) & 3;
  uint32_t miss = 0;
  for (int o = 0; o < P; ++o) {
    int q = p + o;
    if (q >= P) q -= P;
    const uint32_t hw = st.hand[q];
    const int len = (hw >> 25) & 7;
    if (len < H) miss |= 1u << o;
    const uint32_t kcp = st.kcp[q], krp = st.krp[q], kh = st.kh[q];
    for (int i = 0; i < H; ++i) {
      if (i < len) {
        if (o > 0) {
          const int card = (hw >> (5 * i)) & 31;
          const int c = (card * 13) >> 6, r = card - 5 * c;
          or_bit(s_obs, base + (uint32_t)((o * H + i) * 25) + perm_c(pm, c) * RR + (uint32_t)r);
        }
        const uint32_t cp = (kcp >> (5 * i)) & 31u, rp = (krp >> (5 * i)) & 31u;
        const uint32_t h6 = (kh >> (6 * i)) & 63u;
        uint64_t m = 0;
        for (int c = 0; c < 5; ++c) m |= ((cp >> c) & 1u) ? ((uint64_t)rp << (perm_c(pm, c) * RR)) : 0ull;
        if (h6 & 7u) m |= 1ull << (CR + perm_c(pm, (int)(h6 & 7u) - 1));
        if (h6 >> 3) m |= 1ull << (CR + 5u + (h6 >> 3) - 1u);
        or_bits64(s_obs, base + (uint32_t)ge.OK + (uint32_t)((o * H + i) * 35), m);
      }
    }
  }
  or_bits32(s_obs, base + (uint32_t)(P * H * 25), miss);
  or_bits64(s_obs, base + (uint32_t)ge.OB, (1ull << deck_size) - 1ull);
  uint64_t bm = 0;
  for (int c = 0; c < 5; ++c) {
    const int f = (st.board >> (3 * c)) & 7;
    bm |= (f > 0) ? (1ull << (perm_c(pm, c) * RR + (uint32_t)f - 1u)) : 0ull;
  }
  bm |= (uint64_t)((1u << info) - 1u) << CR;
  bm |= (uint64_t)((1u << life) - 1u) << (CR + 8u);
  or_bits64(s_obs, base + (uint32_t)(ge.OB + ge.DECKW), bm);
  uint64_t dm = 0;
  for (int c = 0; c < 5; ++c) {
    const uint32_t pc = perm_c(pm, c);
    for (int r = 0; r < 5; ++r) {
      const uint32_t n = cnt2(st.disc, c * 5 + r);
      const uint32_t roff = (r == 0) ? 0u : (1u + 2u * (uint32_t)r);
      dm |= (uint64_t)((1u << n) - 1u) << (pc * 10u + roff);
    }
  }
  or_bits64(s_obs, base + (uint32_t)ge.OD, dm);
  or_bits64(s_obs, base + (uint32_t)ge.OL, encode_last_action(P, H, st.lastmv, p, pm));
  if (sad) or_bits64(s_obs, base + (uint32_t)ge.F0, encode_last_action(P, H, st.greedy, p, pm));
}

// ---- states --------------------------------------------------------------------------------------------------------------------
static const int kMaxCount[5] = {3, 2, 2, 2, 1};

static uint32_t random_move(int P, int H) {
  uint32_t rec = below(5);                        // type 0..4
  rec |= below((uint32_t)P) << 3;                 // player
  rec |= (1u + below((uint32_t)P - 1u)) << 6;     // target offset 1..P-1
  rec |= below(5) << 9;                           // colour
  rec |= below(5) << 12;                          // rank
  rec |= below((uint32_t)H) << 15;                // card index
  rec |= below(1u << H) << 18;                    // reveal mask
  rec |= below(5) << 23;                          // card colour
  rec |= below(5) << 26;                          // card rank
  rec |= below(4) << 29;                          // scored, information token
  return rec;
}

static State random_state(int P, int H) {
  State st;
  memset(&st, 0, sizeof st);
  const int DECKW = 50 - P * H;
  for (int c = 0; c < 5; ++c) st.board |= below(6) << (3 * c);
  st.board |= below(9) << 15;
  st.board |= below(4) << 19;
  st.board |= (uint32_t)(rnd() & 0x7ffu) << 21;   // turns, current and next player: not part of a row
  st.misc = (uint32_t)rnd() & ~(63u << 8);
  st.misc |= below((uint32_t)DECKW + 1u) << 8;
  for (int t = 0; t < 25; ++t) st.disc |= (uint64_t)below((uint32_t)kMaxCount[t % 5] + 1u) << (2 * t);
  st.lastmv = random_move(P, H);
  st.greedy = random_move(P, H);
  for (int q = 0; q < P; ++q) {
    const uint32_t len = below(8) ? (uint32_t)H - below(2) : below((uint32_t)H + 1u);
    uint32_t hw = len << 25, kh = 0;
    for (int i = 0; i < 5; ++i) {   // the words of cards past the hand's length hold anything: neither form may read them
      hw |= below(25) << (5 * i);
      kh |= (below(6) | (below(6) << 3)) << (6 * i);
    }
    st.hand[q] = hw;
    st.kcp[q] = (uint32_t)rnd() & 0x1ffffffu;
    st.krp[q] = (uint32_t)rnd() & 0x1ffffffu;
    st.kh[q] = kh;
  }
  return st;
}

// the extremes of every section, one combination per k (k < kExtremes)
static const int kExtremes = 40;
static State extreme_state(int P, int H, int k) {
  State st = random_state(P, H);
  const int DECKW = 50 - P * H;
  const bool hi = k & 1;
  // deck empty / full, information 0 / 8, life 0 / 3, fireworks 0 / 5: together and against each other
  st.misc = (st.misc & ~(63u << 8)) | ((uint32_t)((k & 2) ? DECKW : 0) << 8);
  st.board &= ~0x1fffffu;
  for (int c = 0; c < 5; ++c) st.board |= (uint32_t)(hi ? 5 : 0) << (3 * c);
  st.board |= (uint32_t)((k & 4) ? 8 : 0) << 15;
  st.board |= (uint32_t)((k & 2) ? 0 : 3) << 19;
  if (k & 8) {   // every discard thermometer at full width
    st.disc = 0;
    for (int t = 0; t < 25; ++t) st.disc |= (uint64_t)kMaxCount[t % 5] << (2 * t);
  } else if (k & 16) {
    st.disc = 0;
  }
  for (int q = 0; q < P; ++q) {
    const uint32_t len = (k & 32) ? (uint32_t)H : (uint32_t)((q + k) % (H + 1));   // hands shorter than H, down to empty
    st.hand[q] = (st.hand[q] & ~(7u << 25)) | (len << 25);
    if (hi) {   // all knowledge bits and all hints set
      st.kcp[q] = st.krp[q] = 0x1ffffffu;
      st.kh[q] = 0;
      for (int i = 0; i < 5; ++i) st.kh[q] |= (5u | (5u << 3)) << (6 * i);
    } else if (k & 4) {
      st.kcp[q] = st.krp[q] = st.kh[q] = 0;
    }
  }
  // every last-move type, as the last move and as the greedy one, by every player and at the widest fields
  st.lastmv = (st.lastmv & ~7u) | (uint32_t)(k % 5);
  st.greedy = (st.greedy & ~7u) | (uint32_t)((k / 5) % 5);
  if (k & 2) {
    st.lastmv |= ((1u << H) - 1u) << 18;
    st.lastmv = (st.lastmv & ~(7u << 15)) | ((uint32_t)(H - 1) << 15);
    st.lastmv |= 3u << 29;
    st.greedy = (st.greedy & ~(63u << 23)) | (4u << 23) | (4u << 26);
  }
  return st;
}

static uint32_t random_perm() {
  int a[5] = {0, 1, 2, 3, 4};
  for (int i = 4; i > 0; --i) {
    const int j = (int)below((uint32_t)i + 1u);
    const int t = a[i];
    a[i] = a[j];
    a[j] = t;
  }
  uint32_t pm = 0;
  for (int c = 0; c < 5; ++c) pm |= (uint32_t)a[c] << (3 * c);
  return pm;
}

// ---- the comparison ------------------------------------------------------------------------------------------------------------
static long n_rows = 0, n_shifts_seen = 0, n_first = 0, n_last = 0, n_extreme = 0;
static bool seen_shift[32];
static const int kGuard = 4;
static const uint32_t kGuardWord = 0xA5A55A5Au;

struct Sink {
  uint32_t* bits;
  uint32_t first, last;   // the words the row has bits in
  void operator()(uint32_t w, uint32_t v) const {
    if (w < first || w > last) {
      printf("obs_row_place touched word %u (value %08x) outside the row's words %u..%u\n", w, v, first, last);
      exit(1);
    }
    bits[w] |= v;
  }
};

template <int P, int H>
static void check_row(const State& st, int p, uint32_t pm, int sad, uint32_t base, int rows, const char* what) {
  const Geom ge = geom_of(P, H, sad);
  using Gc = ObsRowGeom<P, H>;
  if (ge.F0 != Gc::F0 || ge.OB != Gc::OB || ge.OD != Gc::OD || ge.OL != Gc::OL || ge.OK != Gc::OK || ge.LAL != Gc::LAL ||
      ge.DECKW != Gc::DECKW || (sad && ge.F != Gc::FS)) {
    printf("ObsRowGeom<%d,%d> disagrees with hsad_env_create's offsets\n", P, H);
    exit(1);
  }
  const uint32_t obs_words = (uint32_t)((rows * ge.F + 31) / 32);
  // want: the scatter form, with slack behind the buffer for the zero words its or_bits64 touches; got: exactly obs_words and guards
  static std::vector<uint32_t> want, got;
  want.assign(obs_words + kGuard, 0u);
  got.assign(obs_words + kGuard, 0u);
  for (int k = 0; k < kGuard; ++k) got[obs_words + k] = kGuardWord;
  scatter_row(ge, st, p, pm, sad, want.data(), base);

  uint32_t hand[P], kcp[P], krp[P], kh[P];
  for (int o = 0; o < P; ++o) {
    const int q = (p + o) % P;
    hand[o] = st.hand[q];
    kcp[o] = st.kcp[q];
    krp[o] = st.krp[q];
    kh[o] = st.kh[q];
  }
  uint32_t row[Gc::NW];
  memset(row, 0xff, sizeof row);   // assemble owns the whole array
  obs_row_assemble<P, H>(row, st.board, st.misc, st.disc, st.lastmv, st.greedy, hand, kcp, krp, kh, p, pm, sad != 0);
  const Sink sink = {got.data(), base >> 5, (base + (uint32_t)ge.F - 1u) >> 5};
  if (sink.last >= obs_words) {
    printf("the test's own row at bit %u leaves its buffer\n", base);
    exit(1);
  }
  obs_row_place<P, H>(row, base, sad != 0, sink);

  for (uint32_t w = 0; w < obs_words; ++w)
    if (got[w] != want[w]) {
      printf("<%d,%d> sad %d pm %05x observer %d base %u (%s): word %u is %08x, the scatter form gives %08x\n", P, H, sad, pm, p,
             base, what, w, got[w], want[w]);
      exit(1);
    }
  for (int k = 0; k < kGuard; ++k)
    if (got[obs_words + k] != kGuardWord || want[obs_words + k] != 0u) {
      printf("<%d,%d> sad %d base %u (%s): guard word %d changed\n", P, H, sad, base, what, k);
      exit(1);
    }
  ++n_rows;
  seen_shift[base & 31u] = true;
  if (base == 0) ++n_first;
  if (sink.last == obs_words - 1 && ((base + (uint32_t)ge.F) & 31u) == 0u) ++n_last;
}

// one state in every placement: first, interior and last row of a buffer exactly `rows` rows long (a multiple of 32: the last row
// ends on the buffer's last word), and at all 32 shifts
template <int P, int H>
static void check_state(const State& st, int sad, uint32_t pm, bool all_shifts, const char* what) {
  const int rows = 32 * P;
  const int F = geom_of(P, H, sad).F;
  for (int p = 0; p < P; ++p) {
    check_row<P, H>(st, p, pm, sad, 0u, rows, what);
    check_row<P, H>(st, p, pm, sad, (uint32_t)((1 + (int)below((uint32_t)rows - 2u)) * F), rows, what);
    check_row<P, H>(st, p, pm, sad, (uint32_t)((rows - 1) * F), rows, what);
  }
  if (all_shifts)
    for (uint32_t s = 0; s < 32; ++s)   // any bit position, not only a row's: as far back as a row still fits
      check_row<P, H>(st, (int)below((uint32_t)P), pm, sad, 32u * below((uint32_t)((rows - 2) * F / 32)) + s, rows, what);
}

template <int P, int H>
static void check_instance(int n_random) {
  for (int sad = 0; sad < 2; ++sad)
    for (int shuffled = 0; shuffled < 2; ++shuffled) {
      for (int rep = 0; rep < n_random; ++rep)
        check_state<P, H>(random_state(P, H), sad, shuffled ? random_perm() : kObsIdentityPerm, rep % 16 == 0, "random");
      for (int k = 0; k < kExtremes; ++k, ++n_extreme)
        check_state<P, H>(extreme_state(P, H, k), sad, shuffled ? random_perm() : kObsIdentityPerm, true, "extreme");
    }
}

int main() {
  check_instance<2, 5>(1500);
  check_instance<3, 5>(1000);
  check_instance<4, 4>(1000);
  check_instance<5, 4>(1000);
  for (int s = 0; s < 32; ++s) n_shifts_seen += seen_shift[s] ? 1 : 0;
  printf("rows %ld shifts %ld first %ld last %ld extremes %ld\n", n_rows, n_shifts_seen, n_first, n_last, n_extreme);
  return 0;
}
