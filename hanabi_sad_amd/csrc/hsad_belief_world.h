// hsad_belief_world.h — the per-slot stratified uniforms of the learned belief's worlds: what bh_row (hsad_belief_head.h, sample
// mode) draws slot i of world w of a root game with, so that the W worlds of a game cover every slot's conditional evenly.  Plain
// C++ (no HIP types, no allocation, integer arithmetic only: host and device agree bit for bit); the hash comes in as a functor:
// env_determinize_belief_worlds_kernel (hsad_env_belief.inc) calls it under hipcc, tests/belief_world/belief_world_main.cc under g++.
// Specification: include/hsad.h, hsad_env_determinize_belief_worlds; DESIGN.md section 3g.
//
// h(c) = the policy's hash of (seed, group, c) on stream 67, a 32-bit word; W = n_worlds in [1, 2^20], w in [0, W).  For slot i:
//   a_i : for k = 0 .. 7: cand = 1 + ((h(16 + 8 i + k) * (W - 1)) >> 32); the first cand with gcd(cand, W) == 1; none: a_i = 1
//   o_i = (h(2 i) * W) >> 32
//   s_i = (a_i * w + o_i) mod W                  the slot's stratum for this world: w -> s_i is a bijection of [0, W)
//   j_i = h((1 << 8) | i) >> 8                   24 bits of jitter, ONE per (group, slot): the same in every world of the group
//   k_i = ((s_i << 24) + j_i) / W                0 <= k_i < 2^24, and k_i W lies in [s_i 2^24, (s_i + 1) 2^24)
//   u_i = k_i << 8                               what bh_slot_pick takes: uf = k_i 2^-24, exact
// A Latin-hypercube design: the worlds of a group hit each of the W strata of every slot exactly once, the slots' permutations are
// independent over the hash, and a single world is a plain draw (its stratum and the jitter are uniform).  Within a group the W
// points of a slot are one lattice of spacing 1 / W shifted by the jitter (systematic sampling), so ANY interval of length p of
// [0, 1) holds floor(W p) or ceil(W p) of them; a jitter of its own per world would allow one more or one less.  W = 1: a_i = 1,
// o_i = 0, u_i = the jitter word with its low byte cleared.  All loops are bounded: 8 candidates, Euclid on numbers below 2^21.
#ifndef HSAD_BELIEF_WORLD_H
#define HSAD_BELIEF_WORLD_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HSAD_BW_FN __host__ __device__ inline
#else
#define HSAD_BW_FN inline
#endif

constexpr int BW_STREAM = 67;              // 64: rejection sampler, 65: stratified rank, 66: hsad_env_determinize_belief
constexpr int BW_MAX_SLOTS = 5;
constexpr uint32_t BW_MAX_WORLDS = 1u << 20;
constexpr int BW_TRIES = 8;

HSAD_BW_FN uint32_t bw_gcd(uint32_t a, uint32_t b) {
  while (b) {
    const uint32_t r = a % b;
    a = b;
    b = r;
  }
  return a;
}

// the multiplier of slot i's stratum permutation: coprime to W
template <class Hash>
HSAD_BW_FN uint32_t bw_stride(Hash h, uint32_t W, int i) {
  for (int k = 0; k < BW_TRIES; ++k) {
    const uint32_t cand = 1u + (uint32_t)(((uint64_t)h((uint64_t)(16 + BW_TRIES * i + k)) * (uint64_t)(W - 1u)) >> 32);
    if (bw_gcd(cand, W) == 1u) return cand;
  }
  return 1u;
}

template <class Hash>
HSAD_BW_FN uint32_t bw_offset(Hash h, uint32_t W, int i) {
  return (uint32_t)(((uint64_t)h((uint64_t)(2 * i)) * (uint64_t)W) >> 32);
}

HSAD_BW_FN uint32_t bw_stratum(uint32_t a, uint32_t o, uint32_t W, uint32_t w) {
  return (uint32_t)(((uint64_t)a * (uint64_t)w + (uint64_t)o) % (uint64_t)W);
}

// u[0 .. BW_MAX_SLOTS - 1] of world w of W; false (u untouched) when W or w is out of range.  strata (or NULL): the s_i.
template <class Hash>
HSAD_BW_FN bool bw_uniforms(Hash h, int64_t n_worlds, int64_t world, uint32_t* u, uint32_t* strata) {
  if (n_worlds < 1 || n_worlds > (int64_t)BW_MAX_WORLDS || world < 0 || world >= n_worlds) return false;
  const uint32_t W = (uint32_t)n_worlds, w = (uint32_t)world;
  for (int i = 0; i < BW_MAX_SLOTS; ++i) {
    const uint32_t s = bw_stratum(bw_stride(h, W, i), bw_offset(h, W, i), W, w);
    const uint32_t j = h((1ull << 8) | (uint64_t)i) >> 8;
    const uint32_t k = (uint32_t)((((uint64_t)s << 24) + (uint64_t)j) / (uint64_t)W);
    u[i] = k << 8;
    if (strata) strata[i] = s;
  }
  return true;
}

#endif  // HSAD_BELIEF_WORLD_H
