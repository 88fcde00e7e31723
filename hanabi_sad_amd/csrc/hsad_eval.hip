// hsad_eval.hip — the seat kernels of a tournament batch (include/hsad.h: hsad_seat_gather / hsad_seat_scatter / hsad_seating_stats /
// hsad_seating_behaviour).
//
// What they serve: the cross-play measurement of the reference (pyhanabi/tools/eval_model.py, models/op_raw_data.txt) as ONE
// batched run.  An env object holds S seatings x n deals (hsad_env_reseed with period n: every seating plays the same deals);
// seat p of the games of seating s is played by model seatings[s][p].  Per step each model of the pool acts ONCE, on the rows it
// owns:
//   gather   rows[i] = g * P + p  ->  that model's operands, row i: the observation (bf16, as the env's packed output holds it, or
//            cast from / copied as the float32 one) and the legal-move row
//   scatter  its chosen actions back into a / greedy_a [G, P]; finished games receive the noop uid
//   stats    per seating: sum score, sum score^2, perfect and finished games (integers), and the ONE word a host loop waits for,
//            the number of games still running
//   behaviour (on request) per seating and seat: the HSAD_BH_* counters of the moves about to be stepped (csrc/hsad_behaviour.h)
// The first three stream each byte once and need no cross-workgroup communication beyond one integer atomic per workgroup (stats).
// The bf16 rows are whole 16-byte vectors (row length a multiple of 8, base 16-byte aligned); the float32 observation rows
// (838 floats) and the legal-move rows (21 floats = 84 B) are not 16-byte aligned and move as dwords.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "hsad.h"
#include "hsad_behaviour.h"

extern "C" int hsad_internal_set_error(int code, const char* msg);
extern "C" int hsad_internal_env_status(const hsad_env* e, const uint32_t** misc, int* G, int* P, int* A, int* perfect_score);
extern "C" int hsad_internal_env_rulebot_view(const hsad_env* e, const uint32_t** planes, uint32_t** act_count, int* G, int* Gpad, RbRules* ru);

namespace {

int efail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return hsad_internal_set_error(code, buf);
}
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return efail(HSAD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define CK(expr)            \
  do {                      \
    const int rc_ = (expr); \
    if (rc_) return rc_;    \
  } while (0)

constexpr int kGatherThreads = 128;   // 896 bf16 = 112 vectors of 16 B per row: one pass of a 128-thread workgroup
constexpr int kStatsThreads = 256;
constexpr int kBhThreads = 256;
constexpr int kBhMaxPlayers = 5;

__device__ __forceinline__ uint32_t f2bf_bits(float f) {   // round to nearest even: the rounding of hsad_cast_pad_bf16
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

// a game counts as finished once it was started and has terminated (PL_MISC of hsad_env.hip: started [15], term [14])
__device__ __forceinline__ bool game_finished(uint32_t misc) { return ((misc >> 15) & 1u) && ((misc >> 14) & 1u); }

// one workgroup per listed row.  KIND 0: bf16 row copy; 1: fp32 -> bf16 cast + zero pad; 2: fp32 row copy
template <int KIND>
__global__ __launch_bounds__(kGatherThreads) void seat_gather_kernel(const int32_t* __restrict__ rows, int num_rows,
                                                                     const void* __restrict__ obs_src, int F, int Kp,
                                                                     const float* __restrict__ legal, int A,
                                                                     void* __restrict__ obs_out, float* __restrict__ legal_out) {
  const int i = blockIdx.x;
  const int r = rows[i];
  if (r < 0 || r >= num_rows) return;
  const int t = threadIdx.x;
  if (KIND == 0) {
    const uint4* s = reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(obs_src) + (size_t)r * Kp);
    uint4* d = reinterpret_cast<uint4*>(static_cast<unsigned short*>(obs_out) + (size_t)i * Kp);
    for (int c = t; c < (Kp >> 3); c += kGatherThreads) d[c] = s[c];
  } else if (KIND == 1) {
    const float* s = static_cast<const float*>(obs_src) + (size_t)r * F;
    uint4* d = reinterpret_cast<uint4*>(static_cast<unsigned short*>(obs_out) + (size_t)i * Kp);
    for (int c = t; c < (Kp >> 3); c += kGatherThreads) {
      uint32_t h[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = 8 * c + e < F ? f2bf_bits(s[8 * c + e]) : 0u;
      d[c] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
  } else {
    const float* s = static_cast<const float*>(obs_src) + (size_t)r * F;
    float* d = static_cast<float*>(obs_out) + (size_t)i * F;
    for (int c = t; c < F; c += kGatherThreads) d[c] = s[c];
  }
  for (int c = t; c < A; c += kGatherThreads) legal_out[(size_t)i * A + c] = legal[(size_t)r * A + c];
}

__global__ void seat_scatter_kernel(const uint32_t* __restrict__ misc, int num_rows, int P, int noop, const int32_t* __restrict__ rows,
                                    int n, const int64_t* __restrict__ a_src, const int64_t* __restrict__ g_src,
                                    int64_t* __restrict__ a, int64_t* __restrict__ ga) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = rows[i];
  if (r < 0 || r >= num_rows) return;
  const uint32_t m = misc[r / P];
  const bool live = ((m >> 15) & 1u) && !((m >> 14) & 1u);   // hsad_env_query word 0 == 0
  a[r] = live ? a_src[i] : (int64_t)noop;
  ga[r] = live ? g_src[i] : (int64_t)noop;
}

// one workgroup per seating; the five integer partial sums meet in LDS
__global__ __launch_bounds__(kStatsThreads) void seating_stats_kernel(const uint32_t* __restrict__ misc, int n_per, int perfect_score,
                                                                      long long* __restrict__ stats, int* __restrict__ unfinished) {
  __shared__ long long part[5][kStatsThreads];
  const int s = blockIdx.x, t = threadIdx.x;
  long long sum = 0, sq = 0, perfect = 0, fin = 0, open = 0;
  for (int k = t; k < n_per; k += kStatsThreads) {
    const uint32_t m = misc[(size_t)s * n_per + k];
    if (game_finished(m)) {
      const long long sc = (long long)((m >> 16) & 63u) - 1;
      sum += sc;
      sq += sc * sc;
      perfect += sc == perfect_score ? 1 : 0;
      fin += 1;
    } else {
      open += 1;
    }
  }
  part[0][t] = sum;
  part[1][t] = sq;
  part[2][t] = perfect;
  part[3][t] = fin;
  part[4][t] = open;
  __syncthreads();
  for (int w = kStatsThreads / 2; w > 0; w >>= 1) {
    if (t < w)
      for (int q = 0; q < 5; ++q) part[q][t] += part[q][t + w];
    __syncthreads();
  }
  if (t < 4) stats[(size_t)s * 4 + t] = part[t][0];
  if (t == 0 && part[4][0]) atomicAdd(unfinished, (int)part[4][0]);
}

// grid (ceil(n_per / kBhThreads), S): one thread per game of seating blockIdx.y.  The P x 13 partial sums meet in LDS (32-bit: a
// workgroup adds at most 256 x 15 to a counter), then one 64-bit atomic per non-zero counter per workgroup goes to HBM.
__global__ __launch_bounds__(kBhThreads) void seating_behaviour_kernel(const uint32_t* __restrict__ planes, size_t Gpad, RbRules ru,
                                                                       int n_per, const int64_t* __restrict__ a,
                                                                       unsigned long long* __restrict__ counts) {
  __shared__ unsigned int part[kBhMaxPlayers * HSAD_BH_NSTAT];
  const int t = threadIdx.x, s = blockIdx.y, k = blockIdx.x * kBhThreads + t;
  const int cells = ru.P * HSAD_BH_NSTAT;
  if (t < cells) part[t] = 0u;
  __syncthreads();
  if (k < n_per) {
    const int g = s * n_per + k;
    const GlobalPlanes w{planes, Gpad, g};
    if (misc_live(w(PL_MISC))) {
      const int p = board_cur(w(PL_BOARD));
      if (p >= 0 && p < ru.P) {
        const bh_inc inc = bh_classify(w, ru, p, a[(size_t)g * ru.P + p]);
#pragma unroll
        for (int q = 0; q < HSAD_BH_NSTAT; ++q) {
          const int v = bh_get(inc, q);
          if (v) atomicAdd(&part[p * HSAD_BH_NSTAT + q], (unsigned int)v);
        }
      }
    }
  }
  __syncthreads();
  if (t < cells && part[t]) atomicAdd(&counts[(size_t)s * cells + t], (unsigned long long)part[t]);
}

}  // namespace

extern "C" {

int hsad_seat_gather(const int32_t* rows, int n, int num_rows, int obs_kind, const void* obs_src, int F, int Kp, const float* legal_move,
                     int A, void* obs_out, float* legal_out, void* stream) {
  if (!rows || !obs_src || !legal_move || !obs_out || !legal_out) return efail(HSAD_ERR_INVALID, "hsad_seat_gather: null argument");
  if (n < 1 || num_rows < 1 || F < 1 || A < 1) return efail(HSAD_ERR_INVALID, "hsad_seat_gather: n, num_rows, F and A must be >= 1");
  if (obs_kind < 0 || obs_kind > 2) return efail(HSAD_ERR_INVALID, "hsad_seat_gather: obs_kind must be 0 (bf16 rows), 1 (cast) or 2 (fp32 rows)");
  if (obs_kind != 2 && (Kp < F || (Kp & 7) || ((uintptr_t)obs_out & 15u) || (obs_kind == 0 && ((uintptr_t)obs_src & 15u))))
    return efail(HSAD_ERR_INVALID, "hsad_seat_gather: bf16 rows must be 16-byte aligned and a multiple of 8 values >= F long");
  const dim3 grid(n), block(kGatherThreads);
  hipStream_t st = (hipStream_t)stream;
  if (obs_kind == 0)
    hipLaunchKernelGGL(seat_gather_kernel<0>, grid, block, 0, st, rows, num_rows, obs_src, F, Kp, legal_move, A, obs_out, legal_out);
  else if (obs_kind == 1)
    hipLaunchKernelGGL(seat_gather_kernel<1>, grid, block, 0, st, rows, num_rows, obs_src, F, Kp, legal_move, A, obs_out, legal_out);
  else
    hipLaunchKernelGGL(seat_gather_kernel<2>, grid, block, 0, st, rows, num_rows, obs_src, F, Kp, legal_move, A, obs_out, legal_out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_seat_scatter(const hsad_env* env, const int32_t* rows, int n, const int64_t* a_src, const int64_t* greedy_src, int64_t* a,
                      int64_t* greedy_a, void* stream) {
  if (!rows || !a_src || !greedy_src || !a || !greedy_a) return efail(HSAD_ERR_INVALID, "hsad_seat_scatter: null argument");
  if (n < 1) return efail(HSAD_ERR_INVALID, "hsad_seat_scatter: n must be >= 1");
  const uint32_t* misc;
  int G, P, A, perfect;
  CK(hsad_internal_env_status(env, &misc, &G, &P, &A, &perfect));
  hipLaunchKernelGGL(seat_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, misc, G * P, P, A - 1, rows, n, a_src,
                     greedy_src, a, greedy_a);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_seating_stats(const hsad_env* env, int games_per_seating, int64_t* stats, int32_t* unfinished, void* stream) {
  if (!stats || !unfinished) return efail(HSAD_ERR_INVALID, "hsad_seating_stats: null argument");
  const uint32_t* misc;
  int G, P, A, perfect;
  CK(hsad_internal_env_status(env, &misc, &G, &P, &A, &perfect));
  if (games_per_seating < 1 || G % games_per_seating)
    return efail(HSAD_ERR_INVALID, "hsad_seating_stats: %d games are no whole number of seatings of %d", G, games_per_seating);
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(unfinished, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(seating_stats_kernel, dim3(G / games_per_seating), dim3(kStatsThreads), 0, st, misc, games_per_seating, perfect,
                     reinterpret_cast<long long*>(stats), reinterpret_cast<int*>(unfinished));
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_seating_behaviour(const hsad_env* env, int games_per_seating, const int64_t* a, int64_t* counts, void* stream) {
  if (!env || !a || !counts) return efail(HSAD_ERR_INVALID, "hsad_seating_behaviour: null argument");
  const uint32_t* planes;
  uint32_t* act_count;
  int G, Gpad;
  RbRules ru;
  CK(hsad_internal_env_rulebot_view(env, &planes, &act_count, &G, &Gpad, &ru));
  if (games_per_seating < 1 || G % games_per_seating)
    return efail(HSAD_ERR_INVALID, "hsad_seating_behaviour: %d games are no whole number of seatings of %d", G, games_per_seating);
  if (ru.P > kBhMaxPlayers) return efail(HSAD_ERR_INVALID, "hsad_seating_behaviour: %d players, at most %d", ru.P, kBhMaxPlayers);
  const dim3 grid((games_per_seating + kBhThreads - 1) / kBhThreads, G / games_per_seating);
  hipLaunchKernelGGL(seating_behaviour_kernel, grid, dim3(kBhThreads), 0, (hipStream_t)stream, planes, (size_t)Gpad, ru, games_per_seating,
                     a, reinterpret_cast<unsigned long long*>(counts));
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

}  // extern "C"

// the device log of a tournament's games: append, select, gather (hsad_game_log_*)
#include "hsad_game_log.inc"
