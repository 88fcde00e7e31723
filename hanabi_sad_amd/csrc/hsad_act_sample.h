// hsad_act_sample.h — the row of the acting tail: what turns one row of network heads (A advantages, then the value) and its legal
// mask into the greedy action, the action played and Q(s, a).  Plain C++ (no HIP types, no allocation): the kernels of csrc/r2d2/act.inc
// call it under hipcc, tests/act_sample/act_sample_main.cc under g++ -- the acting-tail entry points are this one function on their
// rows (act_sample_q_kernel, the rows at a temperature, writes the same row out from these pieces: DESIGN.md section 3c says why).
// Specification: include/hsad.h, hsad_act_select .. hsad_act_sample_q; DESIGN.md section 3c.
//
// The row (as_tail_row), fp32, in this order of operations:
//   greedy             argmax_j (1 + h[j] - mn) * legal[j], mn the minimum advantage of the whole batch (R2D2Agent.act, pyhanabi/r2d2.py:
//                      235-277); strict >, so ties go to the lowest index and a row without a legal action gives 0
//   the draw           only when (eps > 0 or tau > 0) and an action is legal.  Exploration first: when u(hh) < eps the action is the k-th
//                      legal one, k = as_eps_index(hh, nlegal).  Otherwise, when tau > 0, Pick at u(hs).  Otherwise greedy.
//   Q(s, act)          as_q_at: h[A] + h[act] legal[act] - (sum_j h[j] legal[j]) / A, the sum in ascending j (R2D2Net's dueling head,
//                      q_head_kernel's value at one action)
//
// Draws (counter-based: the reference draws from torch's global generator, which no implementation can reproduce bit for bit):
//   eps draw           hh = mix64(mix64(seed ^ K m) + counter), K = 0xD1342543DE82EF95, m the row; its top 24 bits are the exploration
//                      uniform, its low 32 bits choose the uniform legal action
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

// hh of row m: the exploration hash
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

// Q(s, act) of a row from the sum of its legal advantages (sum_j h[j] legal[j] in ascending j)
HSAD_AS_FN float as_q_from_sum(const float* h, const float* legal, int A, int act, float sum) {
  return h[A] + h[act] * legal[act] - sum / (float)A;
}

HSAD_AS_FN float as_q_at(const float* h, const float* legal, int A, int act) {
  float sum = 0.f;
  for (int j = 0; j < A; ++j) sum += h[j] * legal[j];
  return as_q_from_sum(h, legal, A, act, sum);
}

struct as_tail {
  int greedy, act;
  float qa;   // Q(s, act) when asked for, else 0
};

// One row of the acting tail (head comment).  h: A advantages (and the value h[A], read only with want_qa); mn: the batch minimum;
// m, seed, counter: the exploration draw's key; row_key: this row's sample key or NULL (then the sample draw follows the exploration
// draw's hash and sample_seed is not read).
HSAD_AS_FN as_tail as_tail_row(const float* h, const float* legal, int A, float mn, float eps, float tau, uint64_t m, uint64_t seed,
                               uint64_t counter, const int64_t* row_key, uint64_t sample_seed, bool want_qa) {
  float best = -3.4e38f, sum = 0.f;
  int bi = 0, nlegal = 0;
  for (int j = 0; j < A; ++j) {
    const float l = legal[j];
    const float sc = (1.f + h[j] - mn) * l;
    if (sc > best) {
      best = sc;
      bi = j;
    }
    nlegal += l != 0.f;
    sum += h[j] * l;
  }
  int act = bi;
  if ((eps > 0.f || tau > 0.f) && nlegal > 0) {
    const uint64_t hh = as_eps_hash(seed, m, counter);
    if (eps > 0.f && as_uniform(hh) < eps) {
      int k = as_eps_index(hh, nlegal);
      for (int j = 0; j < A; ++j)
        if (legal[j] != 0.f && k-- == 0) {
          act = j;
          break;
        }
    } else if (tau > 0.f) {
      act = as_pick(h, legal, A, tau, as_uniform(row_key ? as_sample_hash_keyed(sample_seed, *row_key) : as_sample_hash(hh)));
    }
  }
  return as_tail{bi, act, want_qa ? as_q_from_sum(h, legal, A, act, sum) : 0.f};
}

#endif  // HSAD_ACT_SAMPLE_H
