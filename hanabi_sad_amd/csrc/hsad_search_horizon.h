// hsad_search_horizon.h — what one slot of a depth-limited search is worth at its horizon: the score so far plus the blueprint's own
// Q, in fixed point (units of 1 / HSAD_SEARCH_VALUE_SCALE), so that the sums over a job's worlds stay integers: exact and order-free.
// Plain C++ (no HIP types, no allocation): horizon_stats_kernel (hsad_search.hip) calls it under hipcc,
// tests/search_horizon/horizon_main.cc under g++; tests/search_horizon_ref.py restates it in numpy.  Specification: include/hsad.h,
// hsad_search_horizon_stats; DESIGN.md section 3g.
//
// A slot is read through its two status words (PL_MISC, PL_BOARD of hsad_planes.h) and the accessor q(p) = Q of seat p's row:
//   finished (started and terminated)   v = misc_last_score * S              the latched score job_stats_kernel sums; not cut
//   live (started, not terminated)      score = the fireworks of PL_BOARD summed (HSAD_Q_SCORE of a live board: lives are left)
//                                       q     = MOVER: q(num_step % P), the seat on turn as replay_actions_kernel finds it
//                                               TEAM:  q(0) + q(1) + .. + q(P - 1) in fp32, in that order (VDN's joint value)
//                                       b     = (int)rintf(min(max(q, -64), 64) * S), round-half-even; a q that is not finite
//                                               gives b = 0 and is counted
//                                       v     = min(max(score * S + b, 0), perfect_score * S); cut
//   neither (never started)             nothing is counted
// S = 256 and |q| <= 64 after the clamp: q * S is exact in fp32 and |b| <= 16,384.
#ifndef HSAD_SEARCH_HORIZON_H
#define HSAD_SEARCH_HORIZON_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "hsad.h"
#include "hsad_planes.h"

#if defined(__HIPCC__)
#define HSAD_SH_FN __host__ __device__ inline
#else
#define HSAD_SH_FN inline
#endif

struct ShValue {
  int32_t v;       // the slot's value in units of 1 / HSAD_SEARCH_VALUE_SCALE
  int counted;     // 1: the slot adds (v, v * v, 1) to its job
  int cut;         // 1: valued at the horizon, not at the end of its game
  int nonfinite;   // 1: cut with a Q that was NaN or infinite (taken as 0)
};

HSAD_SH_FN bool sh_finite(float x) {   // by the bits: the same answer under any floating-point flags
  uint32_t u;
  memcpy(&u, &x, sizeof(u));
  return (u & 0x7f800000u) != 0x7f800000u;
}

HSAD_SH_FN int32_t sh_bootstrap(float q) {
  return (int32_t)rintf(fminf(fmaxf(q, -64.f), 64.f) * (float)HSAD_SEARCH_VALUE_SCALE);
}

template <class Q>
HSAD_SH_FN ShValue sh_slot(uint32_t misc, uint32_t board, int P, int perfect_score, int mode, const Q& q) {
  ShValue r = {0, 0, 0, 0};
  if (!misc_started(misc)) return r;
  r.counted = 1;
  if (misc_term(misc)) {
    r.v = (int32_t)misc_last_score(misc) * HSAD_SEARCH_VALUE_SCALE;
    return r;
  }
  r.cut = 1;
  float qv;
  if (mode == HSAD_SEARCH_HORIZON_TEAM) {
    qv = q(0);
    for (int p = 1; p < P; ++p) qv = qv + q(p);
  } else {
    qv = q(misc_num_step(misc) % P);
  }
  int32_t b = 0;
  if (sh_finite(qv))
    b = sh_bootstrap(qv);
  else
    r.nonfinite = 1;
  const int32_t top = (int32_t)perfect_score * HSAD_SEARCH_VALUE_SCALE;
  int32_t v = (int32_t)board_fw_sum(board) * HSAD_SEARCH_VALUE_SCALE + b;
  v = v < 0 ? 0 : v;
  r.v = v > top ? top : v;
  return r;
}

#endif  // HSAD_SEARCH_HORIZON_H
