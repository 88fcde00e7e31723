// hsad_act_sample.h — the sampler core of softmax-policy acting: the counter-based draws of the acting tail and the choice of an action
// from the softmax over the legal advantages at a temperature.  Plain C++ (no HIP types, no allocation): act_sample_q_kernel of
// csrc/r2d2/act_sample.inc includes it under hipcc, tests/act_sample/act_sample_main.cc under g++.  Specification: include/hsad.h,
// hsad_act_sample_q; DESIGN.md section 3c.
//
// Draws (as_mix64 = act_mix64 of csrc/r2d2/act.inc, the same constants):
//   eps draw           hh = mix64(mix64(seed ^ K m) + counter), K = 0xD1342543DE82EF95, m the row: act_select_q_kernel's hash; its top 24
//                      bits are the exploration uniform, its low 32 bits choose the uniform legal action
//   sample draw        hs = mix64(hh ^ 0xA0761D6478BD642F)                                              without a row key
//                      hs = mix64(mix64(sample_seed ^ K (uint64) row_key[m]) ^ 0xA0761D6478BD642F)      with one: no row index and no
//                      counter in it, the caller owns uniqueness (a tournament keys by (deal, seat, move), so a deal plays the same
//                      wherever its rows lie in the batch)
//   the uniform        u = (hs >> 40) 2^-24, in [0, 1)
//
// Pick(z[0..A), legal, tau > 0, u), fp32: mx = max legal z_j; w_j = exp((z_j - mx) / tau) on legal j, 0 elsewhere; S = sum w_j in
// ascending j; walk ascending j with the running sum c and return the first legal j with c > u S; the last legal j if rounding leaves
// none.  One legal action is returned without an exponential.  At tau = 1 the distribution w_j / S is the p_j whose cross-entropy
// clone_tail_kernel (csrc/r2d2/clone_loss.inc) minimises: the softmax over the legal advantages, which is the softmax over legal Q (the
// value and the mean cancel in the dueling head).
//
// Range: z_j - mx <= 0, so no weight exceeds 1 and the maximum keeps weight 1 (S >= 1): tau down to 1e-6 lets the other weights
// underflow to 0, tau up to 1e6 makes them all ~1, |z| up to 1e4 keeps (z_j - mx) / tau finite in fp32.  Every comparison of the walk
// is false on a NaN, which then ends at the last legal j: no input gives an illegal action when one is legal.
#ifndef HSAD_ACT_SAMPLE_H
#define HSAD_ACT_SAMPLE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HSAD_AS_FN __host__ __device__ inline
#else
#define HSAD_AS_FN inline
#endif

#define HSAD_AS_ROW_MUL 0xD1342543DE82EF95ull
#define HSAD_AS_SAMPLE_XOR 0xA0761D6478BD642Full

HSAD_AS_FN uint64_t as_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// hh of row m: the exploration hash of act_select_q_kernel
HSAD_AS_FN uint64_t as_eps_hash(uint64_t seed, uint64_t m, uint64_t counter) {
  return as_mix64(as_mix64(seed ^ (HSAD_AS_ROW_MUL * m)) + counter);
}

HSAD_AS_FN uint64_t as_sample_hash(uint64_t hh) { return as_mix64(hh ^ HSAD_AS_SAMPLE_XOR); }

HSAD_AS_FN uint64_t as_sample_hash_keyed(uint64_t sample_seed, int64_t row_key) {
  return as_mix64(as_mix64(sample_seed ^ (HSAD_AS_ROW_MUL * (uint64_t)row_key)) ^ HSAD_AS_SAMPLE_XOR);
}

// the top 24 bits of a hash, and the uniform in [0, 1) they stand for (exact in fp32)
HSAD_AS_FN uint32_t as_u24(uint64_t h) { return (uint32_t)((h >> 40) & 0xFFFFFFull); }
HSAD_AS_FN float as_uniform(uint64_t h) { return (float)as_u24(h) * (1.f / 16777216.f); }

// which of the nlegal legal actions (in ascending order) the exploration draw takes
HSAD_AS_FN int as_eps_index(uint64_t hh, int nlegal) { return (int)(((hh & 0xFFFFFFFFull) * (uint64_t)nlegal) >> 32); }

// Pick: z and legal are rows of A floats (legal[j] != 0 = legal); tau > 0; u in [0, 1).  -1 when no action is legal.
HSAD_AS_FN int as_pick(const float* z, const float* legal, int A, float tau, float u) {
  float mx = 0.f;
  int nlegal = 0, last = -1;
  for (int j = 0; j < A; ++j) {
    if (legal[j] == 0.f) continue;
    if (nlegal == 0 || z[j] > mx) mx = z[j];
    ++nlegal;
    last = j;
  }
  if (nlegal <= 1) return last;
  float S = 0.f;
  for (int j = 0; j < A; ++j)
    if (legal[j] != 0.f) S += expf((z[j] - mx) / tau);
  const float thr = u * S;
  float c = 0.f;
  for (int j = 0; j < A; ++j) {
    if (legal[j] == 0.f) continue;
    c += expf((z[j] - mx) / tau);
    if (c > thr) return j;
  }
  return last;
}

#endif  // HSAD_ACT_SAMPLE_H
