// hsad_gemm_plan.h — how a split-K GEMM's contraction is cut into K ranges (one fp32 slab each).  Host-only, pure integer functions, no HIP:
// csrc/hsad_r2d2.hip plans its launches with them and the CPU suite (tests/gemm_plan/gemm_plan_main.cc, tests/test_gemm_plan_cpu.py) holds
// them to a Python restatement for every K and split the entry points accept.
//
// Two plans exist for the same slabs:
//   core    the grouped launch of the 256 x 256 kernel (hsad_gemm_nt_bf16_group_splitk): every range an EVEN number of 64-deep k tiles,
//           as that kernel's k loop needs (two k tiles per trip), at least 2;
//   plain   gemm_launch's own split (hsad_gemm_nt_bf16_splitk[_acc], hsad_gemm_nt_bf16_ex): ceil(k tiles / split_k) k tiles per range.
// Both cut [0, K) into `count` ranges of `chunk` k tiles of which the last holds `last` (1 .. chunk).  The grouped entry point's fallback
// (items the core does not take) hands the CORE plan's range length to the 128 x 128 kernel (plan_with_chunk), so both of its paths cut the
// same ranges and write the same slabs.
#pragma once
#include <cstdint>

namespace hsad_gemm_plan {

constexpr int kTileK = 64;       // K per k tile (kBK of the kernels)

struct KPlan {
  int chunk;                     // k tiles per range
  int count;                     // ranges = slabs
  int last;                      // k tiles of the last range
};

// ranges of `chunk_tiles` k tiles over K (a multiple of kTileK, >= kTileK; chunk_tiles >= 1)
inline KPlan plan_with_chunk(int K, int chunk_tiles) {
  const int nk = K / kTileK;
  KPlan p;
  p.chunk = chunk_tiles;
  p.count = (nk + chunk_tiles - 1) / chunk_tiles;
  p.last = nk - (p.count - 1) * chunk_tiles;
  return p;
}

// k tiles per range of a grouped split: an even number, as the 256 x 256 core needs
inline int core_kchunk(int K, int split_k) {
  const int nk = K / kTileK;
  int c = (nk + split_k - 1) / split_k;
  c += c & 1;
  return c < 2 ? 2 : c;
}
inline KPlan core_plan(int K, int split_k) { return plan_with_chunk(K, core_kchunk(K, split_k)); }

// gemm_launch's split when no range length is handed to it (split_k >= 1)
inline KPlan plain_plan(int K, int split_k) {
  const int nk = K / kTileK;
  return plan_with_chunk(K, (nk + split_k - 1) / split_k);
}

// floats of workspace one item of a grouped launch needs: a slab of M x N per range; 0 = an item the entry point refuses
inline int64_t group_item_floats(int M, int N, int K, int split_k) {
  if (K < 2 * kTileK || split_k < 1) return 0;
  return (int64_t)core_plan(K, split_k).count * M * N;
}

}  // namespace hsad_gemm_plan
