// hsad_belief_head.h — the row of the learned hand belief: logits of a linear head plus the viewer's card knowledge -> a consistent,
// normalised distribution over the hidden hand, scored against the true hand (training) or sampled from (search).  Plain C++ (no HIP
// types, no allocation): belief_tail_kernel (csrc/r2d2/belief_tail.inc) and env_determinize_belief_kernel (hsad_env_belief.inc) call
// it under hipcc, tests/belief_head/belief_head_main.cc under g++.  Specification: include/hsad.h, hsad_belief_tail /
// hsad_env_determinize_belief; DESIGN.md section 3g.  The integer arithmetic is hsad_hand_count.h's.
//
// The model.  pool, compat_i (cm[i]) and the occupied slots 0 .. n-1 as in hsad_hand_count.h; z[i * 25 + t] the logits.  q = pool
// before slot 0; for slot i = 0 .. n-1, rem = the slots after i:
//   w[t]     = q[t] compat_i[t] C(rem, q - e_t), int64, exact (bh_weights: hc_tables of (q, rem) once, hc_count per type);
//              F = the t with w[t] != 0, wf[t] = (float)w[t]
//   bh_slot_stats, ONE pass over t ascending, fp32:
//     nfeas  = |F|;  finite = every one of the 25 logits of the slot is finite
//     mx     = max of z over F (strict >, start -3.4e38);  best0 = argmax of w over F in int64 (strict >: lowest t on ties)
//     then a second pass over t ascending:  v[t] = wf[t] * exp(z[t] - mx),  S += v[t],  S0 += wf[t];  best = argmax of v (strict >)
//   p[t]     = v[t] * (1 / S)   (bh_prob: the product wf * exp first, then the reciprocal)
//   score    c = the true card:  nll_i = (log S - log wf[c]) - (z[c] - mx),  nll0_i = log S0 - log wf[c]
//   sample   uf = (float)(u >> 8) * 2^-24, thr = uf * S; run = 0; t ascending over F: run += v[t]; c = the first t with run > thr,
//            the last t of F if there is none; nll_i / nll0_i as in score mode: the hand's log-probability is -sum_i nll_i
//   then     q[c] -= 1
// Row sums in slot order from 0.f:  nll += nll_i, nll0 += nll0_i;  cards += [nfeas >= 2], hit += [nfeas >= 2 and best == c], hit0
// likewise with best0.
// bad (score mode): n = the slots before the first card == -1; a card != -1 after it, a card outside 0..24 on an occupied slot, a
// true card outside F (w[c] == 0), or a slot whose logits are not all finite.  Sample mode: a slot with no feasible type or with
// non-finite logits.  A bad row returns all-zero results and has no gradient row.
// Gradient column i * 25 + t (score mode, want_grad, row not bad): scale * (p[t] - [t == c]) on F, 0 elsewhere; 0 for the slots
// from n on and up to ldo.  It is stored in a second walk once the row is known to be good.
// With z == 0: mx = 0, exp(0) = 1, v = wf, S = S0 (same terms, same order), nll_i = nll0_i - 0.f: the same bits; best = best0
// whenever no two weights round to the same float.
// exp / log: the device's __expf / __logf under hipcc's device pass (the siblings' functions), expf / logf of libm on the host.
#ifndef HSAD_BELIEF_HEAD_H
#define HSAD_BELIEF_HEAD_H

#include <math.h>
#include <stdint.h>

#include "hsad_hand_count.h"

#if defined(__HIPCC__)
#define HSAD_BH_FN __host__ __device__ inline
#else
#define HSAD_BH_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define HSAD_BH_EXP(x) __expf(x)
#define HSAD_BH_LOG(x) __logf(x)
#else
#define HSAD_BH_EXP(x) expf(x)
#define HSAD_BH_LOG(x) logf(x)
#endif

struct bh_slot_stats_t {
  float mx, S, S0;
  int best, best0, nfeas, last;   // last = the highest feasible t (-1: none)
  bool finite;
};

struct bh_row_out {
  float nll, nll0;           // sample mode: nll = -log-probability of the sampled hand
  int cards, hit, hit0, bad;
  uint32_t hand;             // the cards walked, 5 bits per slot (sample mode: the sample)
  uint64_t q;                // the pool they leave
  int n;                     // occupied slots
  bool grad_row;             // store() was called for every column below ldo
};

HSAD_BH_FN bool bh_finite(float x) { return x - x == 0.f; }

// w[t] for one slot from the tables of (q, rem)
HSAD_BH_FN int64_t bh_weight(const uint32_t* and_mask, const int64_t* s, uint64_t q, uint32_t cmi, uint32_t rem, int t) {
  const uint32_t c = hc_cnt(q, t);
  if (c == 0u || !((cmi >> t) & 1u)) return 0;
  return (int64_t)c * hc_count(and_mask, s, rem, t);
}

HSAD_BH_FN void bh_weights(uint64_t q, const uint32_t* cm, int n, int i, int64_t* w) {
  const uint32_t rem = hc_all_slots(n) & ~((2u << i) - 1u);
  HcTables T;
  hc_tables(q, cm, rem, &T);
  for (int t = 0; t < HC_TYPES; ++t) w[t] = bh_weight(T.and_mask, T.s, q, cm[i], rem, t);
}

HSAD_BH_FN float bh_v(float z, int64_t w, float mx) { return (float)w * HSAD_BH_EXP(z - mx); }
HSAD_BH_FN float bh_prob(float z, int64_t w, float mx, float inv) { return bh_v(z, w, mx) * inv; }

HSAD_BH_FN bh_slot_stats_t bh_slot_stats(const float* z, const int64_t* w) {
  bh_slot_stats_t st{-3.4e38f, 0.f, 0.f, -1, -1, 0, -1, true};
  int64_t w0 = 0;
  for (int t = 0; t < HC_TYPES; ++t) {
    if (!bh_finite(z[t])) st.finite = false;
    if (w[t] == 0) continue;
    ++st.nfeas;
    st.last = t;
    if (z[t] > st.mx) st.mx = z[t];
    if (w[t] > w0) w0 = w[t], st.best0 = t;
  }
  float vbest = -1.f;
  for (int t = 0; t < HC_TYPES; ++t) {
    if (w[t] == 0) continue;
    const float v = bh_v(z[t], w[t], st.mx);
    st.S += v;
    st.S0 += (float)w[t];
    if (v > vbest) vbest = v, st.best = t;
  }
  return st;
}

HSAD_BH_FN float bh_slot_nll(const bh_slot_stats_t& st, float zc, int64_t wc) {
  return (HSAD_BH_LOG(st.S) - HSAD_BH_LOG((float)wc)) - (zc - st.mx);
}
HSAD_BH_FN float bh_slot_nll0(const bh_slot_stats_t& st, int64_t wc) { return HSAD_BH_LOG(st.S0) - HSAD_BH_LOG((float)wc); }

HSAD_BH_FN int bh_slot_pick(const bh_slot_stats_t& st, const float* z, const int64_t* w, uint32_t u) {
  const float uf = (float)(u >> 8) * 5.9604644775390625e-8f;   // 2^-24
  const float thr = uf * st.S;
  float run = 0.f;
  for (int t = 0; t < HC_TYPES; ++t) {
    if (w[t] == 0) continue;
    run += bh_v(z[t], w[t], st.mx);
    if (run > thr) return t;
  }
  return st.last;
}

// the number of occupied slots of a score-mode row, -1 when a card follows an empty slot
HSAD_BH_FN int bh_occupied(const int32_t* cards, int Hs) {
  int n = 0;
  while (n < Hs && cards[n] != -1) ++n;
  for (int i = n; i < Hs; ++i)
    if (cards[i] != -1) return -1;
  return n;
}

// One row.  z: Hs * 25 logits; cm: HC_MAX_SLOTS masks.  Score mode: cards != NULL (Hs entries, -1 = empty), u and n_sample unused.
// Sample mode: cards == NULL, n_sample occupied slots, u[i] the slot's 32-bit uniform.  scale = weight[b] / B; want_grad (score mode
// only): store(j, value) for every j < ldo of a row that is not bad (the caller zero-fills rows that come back with grad_row == false).
template <class Store>
HSAD_BH_FN bh_row_out bh_row(const float* z, uint64_t pool, const uint32_t* cm, const int32_t* cards, const uint32_t* u, int n_sample, int Hs,
                             float scale, bool want_grad, int ldo, Store store) {
  bh_row_out r{0.f, 0.f, 0, 0, 0, 0, 0u, pool, 0, false};
  const bh_row_out bad{0.f, 0.f, 0, 0, 0, 1, 0u, pool, 0, false};
  const int n = cards ? bh_occupied(cards, Hs) : n_sample;
  if (n < 0 || n > Hs || Hs > HC_MAX_SLOTS) return bad;
  r.n = n;
  uint64_t q = pool;
  int64_t w[HC_TYPES];
  for (int i = 0; i < n; ++i) {
    const float* zi = z + i * HC_TYPES;
    bh_weights(q, cm, n, i, w);
    const bh_slot_stats_t st = bh_slot_stats(zi, w);
    if (!st.finite || st.nfeas == 0) return bad;
    int c;
    if (cards) {
      c = cards[i];
      if (c < 0 || c >= HC_TYPES) return bad;
      if (w[c] == 0) return bad;
    } else {
      c = bh_slot_pick(st, zi, w, u[i]);
    }
    r.nll += bh_slot_nll(st, zi[c], w[c]);
    r.nll0 += bh_slot_nll0(st, w[c]);
    if (st.nfeas >= 2) {
      ++r.cards;
      r.hit += st.best == c;
      r.hit0 += st.best0 == c;
    }
    r.hand |= (uint32_t)c << (5 * i);
    q -= (uint64_t)1 << (2 * c);
  }
  r.q = q;
  if (!(cards && want_grad)) return r;
  q = pool;
  for (int i = 0; i < n; ++i) {
    const float* zi = z + i * HC_TYPES;
    bh_weights(q, cm, n, i, w);
    const bh_slot_stats_t st = bh_slot_stats(zi, w);
    const float inv = 1.f / st.S;
    const int c = cards[i];
    for (int t = 0; t < HC_TYPES; ++t)
      store(i * HC_TYPES + t, w[t] != 0 ? scale * (bh_prob(zi[t], w[t], st.mx, inv) - (t == c ? 1.f : 0.f)) : 0.f);
    q -= (uint64_t)1 << (2 * c);
  }
  for (int j = n * HC_TYPES; j < ldo; ++j) store(j, 0.f);
  r.grad_row = true;
  return r;
}

#endif  // HSAD_BELIEF_HEAD_H
