// Stand-alone driver of hanabi_sad_amd/csrc/hsad_belief_world.h for the CPU suite (tests/test_belief_world_cpu.py builds it with
// g++ -fsanitize=address,undefined and holds its output to tests/belief_world_ref.py, bit for bit).  The hash is the policy's
// (hsad_planes.h) on stream BW_STREAM, as the env kernel passes it.
// usage: belief_world_main <file>.  The file: int32 n, Hs; then per case uint64 seed, group; int32 W, w, n_sample (-1: no row, the
// uniforms only); uint64 pool; uint32 cm [5]; float32 z [Hs * 25].  Printed per case: "u ok u0 .. u4 s0 .. s4" (zeros when the
// world is refused), then -- n_sample >= 0 and ok -- "row bad nll nll0 hand q" of bh_row in sample mode under those uniforms (the two
// floats as their bits).  The u and z buffers are allocated at exactly their size, so that a read or write past them shows.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hsad_belief_head.h"
#include "hsad_belief_world.h"
#include "hsad_planes.h"

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
    std::fprintf(stderr, "usage: belief_world_main <file>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t head[2];
  if (!read_exact(f, head, sizeof head) || head[0] < 0 || head[1] < 1 || head[1] > HC_MAX_SLOTS) {
    std::fprintf(stderr, "bad header\n");
    std::fclose(f);
    return 2;
  }
  const int n = head[0], Hs = head[1];
  for (int i = 0; i < n; ++i) {
    uint64_t sg[2], pool;
    int32_t ww[3];
    std::vector<uint32_t> cm(HC_MAX_SLOTS), u(BW_MAX_SLOTS, 0u), s(BW_MAX_SLOTS, 0u);
    std::vector<float> z(Hs * HC_TYPES);
    if (!read_exact(f, sg, sizeof sg) || !read_exact(f, ww, sizeof ww) || !read_exact(f, &pool, 8) || !read_exact(f, cm.data(), 4 * HC_MAX_SLOTS) ||
        !read_exact(f, z.data(), 4 * Hs * HC_TYPES)) {
      std::fprintf(stderr, "case %d is cut short\n", i);
      std::fclose(f);
      return 2;
    }
    const uint64_t seed = sg[0], group = sg[1];
    const bool ok = bw_uniforms([seed, group](uint64_t c) { return policy_hash(seed, group, c, (uint64_t)BW_STREAM); }, (int64_t)ww[0], (int64_t)ww[1],
                                u.data(), s.data());
    std::printf("u %d", (int)ok);
    for (int k = 0; k < BW_MAX_SLOTS; ++k) std::printf(" %" PRIu32, u[k]);
    for (int k = 0; k < BW_MAX_SLOTS; ++k) std::printf(" %" PRIu32, s[k]);
    std::printf("\n");
    if (ww[2] < 0 || !ok) continue;
    const bh_row_out r = bh_row(z.data(), pool, cm.data(), nullptr, u.data(), ww[2], Hs, 0.f, false, 0, [](int, float) {});
    std::printf("row %d %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", r.bad, bits(r.nll), bits(r.nll0), r.hand, r.q);
  }
  std::fclose(f);
  std::printf("OK\n");
  return 0;
}
