// Stand-alone driver of hanabi_sad_amd/csrc/hsad_clone_soft.h for the CPU suite (tests/test_clone_soft_ref_cpu.py builds it with
// g++ -fsanitize=address,undefined and holds its output to the fp32 restatement row_f32 of tests/clone_soft_ref.py, bit for bit).
// usage: clone_soft_main <file>.  The file (clone_soft_ref.write_rows): int32 n, A, ldo; float32 policy_weight, value_weight; then n rows of
// h [A + 1], legal [A], pi [A] float32, act int64, ret, scale float32.  Every buffer handed to cs_row is allocated at exactly its size, so that
// a read or write past a row shows.  Printed per row: "row i bad step dec hit grad xent hub" (the two floats as their bits), then -- grad == 1 --
// one "g" line with the ldo gradient values as their bits.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hsad_clone_soft.h"

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
    std::fprintf(stderr, "usage: clone_soft_main <file>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t head[3];
  float w[2];
  if (!read_exact(f, head, sizeof head) || !read_exact(f, w, sizeof w) || head[0] < 0 || head[1] < 1 || head[1] > 4096 || head[2] < head[1] + 1 ||
      head[2] > 8192) {
    std::fprintf(stderr, "bad header\n");
    std::fclose(f);
    return 2;
  }
  const int n = head[0], A = head[1], ldo = head[2];
  for (int i = 0; i < n; ++i) {
    std::vector<float> h(A + 1), legal(A), pi(A), grad(ldo, -77.f);
    int64_t act;
    float tail[2];
    if (!read_exact(f, h.data(), 4 * (A + 1)) || !read_exact(f, legal.data(), 4 * A) || !read_exact(f, pi.data(), 4 * A) || !read_exact(f, &act, 8) ||
        !read_exact(f, tail, sizeof tail)) {
      std::fprintf(stderr, "row %d is cut short\n", i);
      std::fclose(f);
      return 2;
    }
    int stored = 0;
    float* g = grad.data();
    const cs_row_out r = cs_row(h.data(), legal.data(), pi.data(), A, act, tail[0], w[0], w[1], tail[1], true, ldo, [g, &stored](int j, float v) {
      g[j] = v;
      ++stored;
    });
    if (r.grad_row != (stored == ldo) || (!r.grad_row && stored != 0)) {
      std::fprintf(stderr, "row %d: %d columns stored, grad_row %d\n", i, stored, (int)r.grad_row);
      std::fclose(f);
      return 3;
    }
    std::printf("row %d %d %d %d %d %d %" PRIu32 " %" PRIu32 "\n", i, r.bad, r.step, r.dec, r.hit, (int)r.grad_row, bits(r.xent), bits(r.hub));
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
