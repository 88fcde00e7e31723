// hsad_clone_soft.h — the row of the soft-target cloning tail: cross-entropy of the softmax over one row's legal advantages against a
// TARGET DISTRIBUTION pi over the actions (search values at a temperature, a teacher's policy), next to the unchanged value term of
// csrc/r2d2/clone_value.inc.  Plain C++ (no HIP types, no allocation): clone_soft_tail_kernel (csrc/r2d2/clone_soft.inc) calls it under
// hipcc, tests/clone_soft/clone_soft_main.cc under g++.  Specification: include/hsad.h, hsad_clone_soft_tail; DESIGN.md section 3c.
//
// The row (cs_row), fp32, in this order of operations; z = h[0..A), l = legal, act = action, all of ONE valid row:
//   bad                act outside [0, A) or l[act] == 0 (clone_value_tail_kernel's rule); or any pi_j negative or NaN; or pi_j != 0 on an
//                      illegal column; or |sigma - 1| > 1e-3 with sigma = sum_{legal j} pi_j in ascending j.  A bad row contributes nothing.
//   mx, bi, S, p_j     as in clone_value_tail_kernel: mx = max legal z_j (strict >: ties keep the lowest index bi), S = sum_{legal j}
//                      exp(z_j - mx) in ascending j, p_j = exp(z_j - mx) * (1 / S); only with >= 2 legal actions (else S = 1)
//   xent               sigma log S - sum_{legal j} pi_j (z_j - mx), the sum in ascending j from 0; 0 with one legal action
//   hit, dec           dec = >= 2 legal actions, hit = dec and bi == act: still defined against the recorded action
//   value term         q = h[A] + z_act l_act - (sum_j z_j l_j) / A, e = ret - q, Huber, g = -clamp(e, -1, 1)  (only with value_weight != 0)
//   gradient column j  legal j: scale (policy_weight (sigma p_j - pi_j) [>= 2 legal] + value_weight g l_j (delta_{j, act} - 1 / A)), summed in
//                      fp32 and handed to store(j, .) once; illegal j: 0; column A: scale value_weight g; up to ldo: 0
// Where pi is the one-hot of act (1.0f and zeros) sigma is exactly 1, sigma x = x, pi_j (z_j - mx) is z_act - mx or a zero and the sum of
// those is z_act - mx: every expression then has the operands, the order and so the bits of clone_value_tail_kernel's -- with value_weight
// == 0 that of its branch without the value term, sp (p_j - delta), which is clone_tail_kernel's row at policy_weight 1.
// exp / log: the device's __expf / __logf under hipcc's device pass (the siblings' functions), expf / logf of libm on the host.
#ifndef HSAD_CLONE_SOFT_H
#define HSAD_CLONE_SOFT_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HSAD_CS_FN __host__ __device__ inline
#else
#define HSAD_CS_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define HSAD_CS_EXP(x) __expf(x)
#define HSAD_CS_LOG(x) __logf(x)
#else
#define HSAD_CS_EXP(x) expf(x)
#define HSAD_CS_LOG(x) logf(x)
#endif

#define HSAD_CS_MASS_TOL 1e-3f      // a condition on the input (|sigma - 1| beyond it: a bad row), not an accuracy tolerance

struct cs_row_out {
  float xent, hub;            // the row's cross-entropy and Huber term (0 where it has none)
  int hit, dec, bad, step;    // 0 / 1 each
  bool grad_row;              // store() was called for every column below ldo
};

// One valid row.  h: A advantages (and the value h[A], read only with value_weight != 0); pi: the target row; ret: the row's return (read
// only with value_weight != 0); scale = weight[b] / B; want_grad: call store(j, value) for every j < ldo of a row that has a gradient (the
// caller zero-fills the rows that come back with grad_row == false).
template <class Store>
HSAD_CS_FN cs_row_out cs_row(const float* h, const float* legal, const float* pi, int A, int64_t act64, float ret, float policy_weight,
                             float value_weight, float scale, bool want_grad, int ldo, Store store) {
  cs_row_out r{0.f, 0.f, 0, 0, 0, 0, false};
  const int act = (act64 >= 0 && act64 < A) ? (int)act64 : -1;
  const bool with_value = value_weight != 0.f;
  float mx = -3.4e38f, sigma = 0.f;
  int bi = 0, nlegal = 0;
  bool target_ok = true;
  for (int j = 0; j < A; ++j) {
    const float pj = pi[j];
    if (!(pj >= 0.f)) target_ok = false;      // (negative or NaN)
    if (legal[j] != 0.f) {
      ++nlegal;
      sigma += pj;
      if (h[j] > mx) mx = h[j], bi = j;       // (strict: a tie keeps the lowest index)
    } else if (pj != 0.f) {
      target_ok = false;
    }
  }
  if (!(fabsf(sigma - 1.f) <= HSAD_CS_MASS_TOL)) target_ok = false;
  if (act < 0 || legal[act] == 0.f || !target_ok) {
    r.bad = 1;
    return r;
  }
  r.step = 1;
  const bool multi = nlegal >= 2;
  float s = 1.f;
  if (multi) {
    s = 0.f;
    float dot = 0.f;
    for (int j = 0; j < A; ++j)
      if (legal[j] != 0.f) {
        s += HSAD_CS_EXP(h[j] - mx);
        dot += pi[j] * (h[j] - mx);
      }
    r.xent = sigma * HSAD_CS_LOG(s) - dot;
    r.dec = 1;
    r.hit = bi == act;
  }
  if (!with_value) {
    if (want_grad && multi) {      // clone_tail_kernel's row, its expression
      const float sp = scale * policy_weight;
      const float inv = 1.f / s;
      for (int j = 0; j < A; ++j) store(j, legal[j] != 0.f ? sp * (sigma * (HSAD_CS_EXP(h[j] - mx) * inv) - pi[j]) : 0.f);
      for (int j = A; j < ldo; ++j) store(j, 0.f);
      r.grad_row = true;
    }
    return r;
  }
  float mean = 0.f;
  for (int j = 0; j < A; ++j) mean += h[j] * legal[j];
  mean /= (float)A;
  const float q = h[A] + h[act] * legal[act] - mean;
  const float e = ret - q;
  const float ae = fabsf(e);
  r.hub = ae < 1.f ? 0.5f * e * e : ae - 0.5f;
  if (want_grad) {
    const float g = -fminf(fmaxf(e, -1.f), 1.f);
    const float inv = 1.f / s;
    const float invA = 1.f / (float)A;
    for (int j = 0; j < A; ++j) {
      const float d = j == act ? 1.f : 0.f;
      const float pol = multi ? policy_weight * (sigma * (HSAD_CS_EXP(h[j] - mx) * inv) - pi[j]) : 0.f;
      store(j, legal[j] != 0.f ? scale * (pol + value_weight * g * legal[j] * (d - invA)) : 0.f);
    }
    store(A, (scale * value_weight) * g);
    for (int j = A + 1; j < ldo; ++j) store(j, 0.f);
    r.grad_row = true;
  }
  return r;
}

#endif  // HSAD_CLONE_SOFT_H
