// Stand-alone driver of hanabi_sad_amd/csrc/hsad_act_sample.h for the CPU suite (tests/test_act_sample_cpu.py builds it with
// g++ -fsanitize=address,undefined and holds its output to the Python restatement tests/act_sample_ref.py).
// usage: act_sample_main <rows per case>.  Case c = 5 * (index of A in 21, 31, 49) + (index of tau in 1e-6, 0.25, 1, 4, 1e6); its rows come
// from the generator of act_sample_ref.seeded_case.  Printed per row: hh, hs, the keyed hs, the 24-bit uniforms of the two, the index the
// exploration draw takes among the legal actions (-1: it does not fire), Pick at the unkeyed and at the keyed uniform (-1: nothing legal).
// Then as_tail_row on the rows of act_sample_ref.tail_case (the seeded rows and three more: no, one and all actions legal), one "tail" line
// per row: greedy, then (a, the bits of qa) without a temperature, at tau with the unkeyed draw and at tau with the keyed one, then the bits of
// as_q_at at the greedy action.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hsad_act_sample.h"

namespace {

struct Gen {
  uint64_t x;
  uint64_t raw() {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return x;
  }
  uint32_t next() { return (uint32_t)(raw() >> 33); }
};

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

}  // namespace

int main(int argc, char** argv) {
  const int rows = argc > 1 ? std::atoi(argv[1]) : 16;
  const int As[3] = {21, 31, 49};
  const float taus[5] = {1e-6f, 0.25f, 1.f, 4.f, 1e6f};
  for (int c = 0; c < 15; ++c) {
    const int A = As[c / 5];
    const float tau = taus[c % 5];
    Gen g{(uint64_t)(c + 1) * 0x9E3779B97F4A7C15ull};
    const uint64_t seed = g.raw(), counter = g.raw(), sample_seed = g.raw();
    std::printf("case %d %d\n", c, A);
    const size_t nt = (size_t)rows + 3;
    std::vector<float> z((size_t)A), legal((size_t)A), th(nt * (A + 1)), tl(nt * A, 0.f), te(nt);
    std::vector<int64_t> tk(nt);
    float mn = 3.4e38f;
    for (int i = 0; i < rows; ++i) {
      const uint32_t mode = g.next() % 8u;
      int nlegal = 0;
      for (int j = 0; j < A; ++j) legal[(size_t)j] = mode == 2u ? 1.f : 0.f;
      if (mode == 1u) legal[(size_t)(g.next() % (uint32_t)A)] = 1.f;
      if (mode > 2u)
        for (int j = 0; j < A; ++j) legal[(size_t)j] = (float)(g.next() & 1u);
      for (int j = 0; j < A; ++j) nlegal += legal[(size_t)j] != 0.f;
      const bool big = g.next() % 4u == 0u;
      for (int j = 0; j < A; ++j) {
        const int k = (int)(g.next() & 0xFFFFFu) - 524288;
        z[(size_t)j] = big ? (float)(k * 5) * (1.f / 256.f) : (float)k * (1.f / 65536.f);
      }
      const float eps = g.next() % 3u == 0u ? 0.3f : 0.f;
      const int64_t key = (int64_t)g.raw();

      const uint64_t hh = as_eps_hash(seed, (uint64_t)i, counter);
      const uint64_t hs = as_sample_hash(hh), hsk = as_sample_hash_keyed(sample_seed, key);
      int k = -1;
      if (eps > 0.f && nlegal > 0 && as_uniform(hh) < eps) k = as_eps_index(hh, nlegal);
      const int a = as_pick(z.data(), legal.data(), A, tau, as_uniform(hs));
      const int ak = as_pick(z.data(), legal.data(), A, tau, as_uniform(hsk));
      std::printf("row %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %d %d %d\n", i, hh, hs, hsk, as_u24(hs), as_u24(hsk), k, a, ak);
      for (int j = 0; j < A; ++j) {
        th[(size_t)i * (A + 1) + j] = z[(size_t)j];
        tl[(size_t)i * A + j] = legal[(size_t)j];
        mn = z[(size_t)j] < mn ? z[(size_t)j] : mn;
      }
      te[(size_t)i] = eps;
      tk[(size_t)i] = key;
    }
    for (int e = 0; e < 3 && e < rows; ++e) {      // z and the key of rows 0, 1, 2 with no, one and all actions legal
      const size_t i = (size_t)rows + e;
      for (int j = 0; j < A; ++j) {
        th[i * (A + 1) + j] = th[(size_t)e * (A + 1) + j];
        tl[i * A + j] = e == 2 || (e == 1 && j == (7 * c + 3) % A) ? 1.f : 0.f;
      }
      te[i] = c % 2 ? 0.f : 0.3f;
      tk[i] = tk[(size_t)e];
    }
    for (size_t i = 0; i < nt; ++i) {
      float* h = &th[i * (A + 1)];
      const float* lg = &tl[i * A];
      h[A] = -h[A - 1] * 0.5f;
      const as_tail t0 = as_tail_row(h, lg, A, mn, te[i], 0.f, i, seed, counter, nullptr, sample_seed, true);
      const as_tail t1 = as_tail_row(h, lg, A, mn, te[i], tau, i, seed, counter, nullptr, sample_seed, true);
      const as_tail t2 = as_tail_row(h, lg, A, mn, te[i], tau, i, seed, counter, &tk[i], sample_seed, true);
      std::printf("tail %zu %d %d %u %d %u %d %u %u\n", i, t0.greedy, t0.act, bits(t0.qa), t1.act, bits(t1.qa), t2.act, bits(t2.qa),
                  bits(as_q_at(h, lg, A, t0.greedy)));
    }
  }
  std::printf("OK\n");
  return 0;
}
