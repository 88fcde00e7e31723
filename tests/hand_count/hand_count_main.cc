// Stand-alone driver of hanabi_sad_amd/csrc/hsad_hand_count.h for the CPU suite (tests/test_hand_count_cpu.py builds it with
// g++ -fsanitize=address,undefined and compares its output, line for line, with the Python restatement tests/hand_belief_ref.py).
// usage: hand_count_main <number of cases>.  The cases come from the generator given in the test's docstring.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "hsad_hand_count.h"

namespace {

struct Gen {
  uint64_t x;
  uint64_t raw() {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return x;
  }
  uint32_t next() { return (uint32_t)(raw() >> 33); }
};

void print_unrank(uint64_t pool, const uint32_t* cm, int n, int64_t r) {
  uint32_t cards = 0;
  uint64_t q = 0;
  const int ok = hc_unrank(pool, cm, n, r, &cards, &q);
  std::printf("unrank %" PRId64 " %d :", r, ok);
  if (ok) {
    for (int i = 0; i < n; ++i) std::printf(" %u", (cards >> (5 * i)) & 31u);
    std::printf(" |");
    for (int t = 0; t < HC_TYPES; ++t) std::printf(" %u", hc_cnt(q, t));
  }
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 60;
  for (int c = 0; c < cases; ++c) {
    Gen g{(uint64_t)(c + 1) * 0x9E3779B97F4A7C15ull};
    const int n = 1 + (int)(g.next() % 5u);
    uint64_t pool = 0;
    for (int t = 0; t < HC_TYPES; ++t) {
      const uint32_t full = t % 5 == 0 ? 3u : (t % 5 == 4 ? 1u : 2u);
      pool |= (uint64_t)(g.next() % (full + 1u)) << (2 * t);
    }
    uint32_t cm[HC_MAX_SLOTS] = {0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
      const uint32_t cp = 1u + g.next() % 31u, rp = 1u + g.next() % 31u;
      for (int t = 0; t < HC_TYPES; ++t)
        if (((cp >> (t / 5)) & 1u) && ((rp >> (t % 5)) & 1u)) cm[i] |= 1u << t;
    }
    int fw[5];
    for (int k = 0; k < 5; ++k) fw[k] = (int)(g.next() % 6u);
    const int64_t W = 1 + (int64_t)(g.next() % 40u);
    const uint64_t u = g.raw();

    const int64_t N = hc_total(pool, cm, n);
    std::printf("case %d %d %" PRId64 "\n", c, n, N);
    HcTables T;
    hc_tables(pool, cm, hc_all_slots(n), &T);
    for (int i = 0; i < n; ++i) {
      int64_t tri[3] = {0, 0, 0};
      std::printf("num %d", i);
      for (int t = 0; t < HC_TYPES; ++t) {
        const int64_t v = hc_marginal(T.and_mask, T.s, pool, cm, n, i, t);
        tri[hc_trinary_class(t % 5, fw[t / 5])] += v;
        std::printf(" %" PRId64, v);
      }
      std::printf("\ntri %d %" PRId64 " %" PRId64 " %" PRId64 "\n", i, tri[0], tri[1], tri[2]);
    }
    if (N <= 400) {
      for (int64_t r = 0; r < N; ++r) print_unrank(pool, cm, n, r);
    } else {
      for (int64_t j = 0; j <= 17; ++j) print_unrank(pool, cm, n, j == 17 ? N - 1 : (j * N) / 17);
    }
    print_unrank(pool, cm, n, N);
    print_unrank(pool, cm, n, -1);
    std::printf("strata %" PRId64 " %" PRIu64 " :", W, u);
    for (int64_t w = 0; w < W; ++w) std::printf(" %" PRId64, hc_stratum_rank(N, w, W, u));
    std::printf("\n");
  }
  std::printf("OK\n");
  return 0;
}
