// Stand-alone driver of hanabi_sad_amd/csrc/hsad_belief_head.h for the CPU suite (tests/test_belief_head_cpu.py builds it with
// g++ -fsanitize=address,undefined and holds its output to the fp32 restatement row_f32 of tests/belief_head_ref.py, bit for bit).
// usage: belief_head_main <file>.  The file (belief_head_ref.write_rows): int32 n, Hs, ldo; then per row int32 mode (0 score, 1 sample),
// n_sample; uint64 pool; uint32 cm [5]; int32 cards [Hs]; uint32 u [5]; float32 scale; float32 z [Hs * 25].  Every buffer handed to
// bh_row is allocated at exactly its size, so that a read or write past a row shows.  Printed per row: "row i bad cards hit hit0 grad
// nll nll0 hand q" (the two floats as their bits), then -- grad == 1 -- one "g" line with the ldo gradient values as their bits.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hsad_belief_head.h"

namespace {

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

bool read_exact(FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: belief_head_main <file>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t head[3];
  if (!read_exact(f, head, sizeof head) || head[0] < 0 || head[1] < 1 || head[1] > HC_MAX_SLOTS || head[2] < head[1] * HC_TYPES || head[2] > 8192) {
    std::fprintf(stderr, "bad header\n");
    std::fclose(f);
    return 2;
  }
  const int n = head[0], Hs = head[1], ldo = head[2];
  for (int i = 0; i < n; ++i) {
    int32_t mode[2];
    uint64_t pool;
    std::vector<uint32_t> cm(HC_MAX_SLOTS), u(HC_MAX_SLOTS);
    std::vector<int32_t> cards(Hs);
    std::vector<float> z(Hs * HC_TYPES), grad(ldo, -77.f);
    float scale;
    if (!read_exact(f, mode, sizeof mode) || !read_exact(f, &pool, 8) || !read_exact(f, cm.data(), 4 * HC_MAX_SLOTS) || !read_exact(f, cards.data(), 4 * Hs) ||
        !read_exact(f, u.data(), 4 * HC_MAX_SLOTS) || !read_exact(f, &scale, 4) || !read_exact(f, z.data(), 4 * Hs * HC_TYPES)) {
      std::fprintf(stderr, "row %d is cut short\n", i);
      std::fclose(f);
      return 2;
    }
    int stored = 0;
    float* g = grad.data();
    const bool score = mode[0] == 0;
    const bh_row_out r = bh_row(z.data(), pool, cm.data(), score ? cards.data() : nullptr, u.data(), mode[1], Hs, scale, score, ldo, [g, &stored](int j, float v) {
      g[j] = v;
      ++stored;
    });
    if (r.grad_row != (stored == ldo) || (!r.grad_row && stored != 0)) {
      std::fprintf(stderr, "row %d: %d columns stored, grad_row %d\n", i, stored, (int)r.grad_row);
      std::fclose(f);
      return 3;
    }
    std::printf("row %d %d %d %d %d %d %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", i, r.bad, r.cards, r.hit, r.hit0, (int)r.grad_row, bits(r.nll),
                bits(r.nll0), r.hand, r.q);
    if (r.grad_row) {
      std::printf("g");
      for (int j = 0; j < ldo; ++j) std::printf(" %" PRIu32, bits(grad[j]));
      std::printf("\n");
    }
  }
  std::fclose(f);
  std::printf("OK\n");
  return 0;
}
