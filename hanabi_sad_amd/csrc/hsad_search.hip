// hsad_search.hip — the glue kernels of blueprint-policy search (include/hsad.h: hsad_search_fork_state / hsad_search_actions /
// hsad_search_job_stats; search.PolicySearch drives them).
//
// What they serve: SPARTA-style single-agent search.  A search env holds `capacity` slots; slot j plays one (root game, candidate
// action, sampled world) job: hsad_env_fork + hsad_env_determinize put the world there, the R2D2 agent acts for every seat of every
// slot per step (hsad_r2d2_act), and the loop stays on the device:
//   fork_state  the agent's carried LSTM state of root game src_index[j] -> the rows of slot j (all layers, all seats), with the bf16
//               copy of h that the fused cell reads for 1,024 rows or more
//   actions     what act returned for the G*P rows -> a / greedy_a [G, P] of hsad_env_step: the noop for finished games, and the
//               candidate action forced on the searcher's seat (first move only: the caller passes no override afterwards).
//               greedy_a keeps the agent's greedy action -- what SAD shows the partner when the searcher deviates
//   job_stats   the finished slots' scores summed per job (sum, sum of squares, count) with integer atomics: exact and order-free
// All three are launch-only, one pass and HBM-bound.  The state rows move as 16-byte vectors (H % 4 == 0; with H % 8 == 0 the bf16
// row is written as 16-byte vectors too).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "hsad.h"

extern "C" int hsad_internal_set_error(int code, const char* msg);
extern "C" int hsad_internal_env_status(const hsad_env* e, const uint32_t** misc, int* G, int* P, int* A, int* perfect_score);

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

constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t f2bf_bits(float f) {   // round to nearest even: the rounding of hsad_cast_pad_bf16
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

// PL_MISC of hsad_env.hip: term [14] | started [15] | last_score + 1 [16..21]
__device__ __forceinline__ bool game_live(uint32_t misc) { return ((misc >> 15) & 1u) && !((misc >> 14) & 1u); }   // hsad_env_query word 0 == 0
__device__ __forceinline__ bool game_finished(uint32_t misc) { return ((misc >> 15) & 1u) && ((misc >> 14) & 1u); }

// one thread per V consecutive values of one destination row (V = 4 | 8, H % V == 0); rows = L * G_dst * P
template <int V>
__global__ __launch_bounds__(kThreads) void fork_state_kernel(const int32_t* __restrict__ src_index, int G_dst, int G_src, int P, int H,
                                                              long long total, const float* __restrict__ h_src,
                                                              const float* __restrict__ c_src, float* __restrict__ h_dst,
                                                              float* __restrict__ c_dst, unsigned short* __restrict__ h16_dst) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int per_row = H / V;
  const long long row = i / per_row;           // (l, j * P + p) of the destination
  const int v = (int)(i - row * per_row);
  const long long rows_dst = (long long)G_dst * P;
  const int l = (int)(row / rows_dst);
  const int rem = (int)(row - (long long)l * rows_dst);
  const int j = rem / P, p = rem - j * P;
  const int s = src_index[j];
  if (s < 0 || s >= G_src) return;             // -1 and anything else out of range: the rows of game j stay as they are
  const size_t so = (((size_t)l * G_src + s) * P + p) * H + (size_t)v * V;
  const size_t dst = (size_t)row * H + (size_t)v * V;
  float4 hv[V / 4];
#pragma unroll
  for (int k = 0; k < V / 4; ++k) {
    hv[k] = *reinterpret_cast<const float4*>(h_src + so + 4 * k);
    const float4 cv = *reinterpret_cast<const float4*>(c_src + so + 4 * k);
    *reinterpret_cast<float4*>(h_dst + dst + 4 * k) = hv[k];
    *reinterpret_cast<float4*>(c_dst + dst + 4 * k) = cv;
  }
  if (h16_dst) {
    uint32_t w[V / 2];
#pragma unroll
    for (int k = 0; k < V / 4; ++k) {
      w[2 * k] = f2bf_bits(hv[k].x) | (f2bf_bits(hv[k].y) << 16);
      w[2 * k + 1] = f2bf_bits(hv[k].z) | (f2bf_bits(hv[k].w) << 16);
    }
    if (V == 8)
      *reinterpret_cast<uint4*>(h16_dst + dst) = make_uint4(w[0], w[1], w[V / 2 - 2], w[V / 2 - 1]);
    else
      *reinterpret_cast<uint2*>(h16_dst + dst) = make_uint2(w[0], w[1]);
  }
}

// one thread per (game, seat) row
__global__ __launch_bounds__(kThreads) void search_actions_kernel(const uint32_t* __restrict__ misc, int num_rows, int P, int noop,
                                                                  const int64_t* __restrict__ a_src, const int64_t* __restrict__ g_src,
                                                                  const int32_t* __restrict__ player, const int64_t* __restrict__ override_a,
                                                                  int64_t* __restrict__ a, int64_t* __restrict__ ga) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= num_rows) return;
  const int g = r / P, p = r - g * P;
  if (!game_live(misc[g])) {
    a[r] = (int64_t)noop;
    ga[r] = (int64_t)noop;
    return;
  }
  int64_t act = a_src[r];
  if (override_a) {
    const int64_t o = override_a[g];
    if (o >= 0 && player[g] == p) act = o;     // p is in [0, P): a player outside that range matches no seat
  }
  a[r] = act;
  ga[r] = g_src[r];
}

// one thread per slot; three integer atomics per finished slot with a valid job
__global__ __launch_bounds__(kThreads) void job_stats_kernel(const uint32_t* __restrict__ misc, int G, const int32_t* __restrict__ job,
                                                             int n_job, unsigned long long* __restrict__ stats) {
  const int g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= G) return;
  const int j = job[g];
  if (j < 0 || j >= n_job) return;
  const uint32_t m = misc[g];
  if (!game_finished(m)) return;
  // the score latched when the game ended: (life <= 0 && bomb) ? 0 : sum of fireworks, i.e. HSAD_Q_SCORE of the final board
  const long long sc = (long long)((m >> 16) & 63u) - 1;
  unsigned long long* s = stats + (size_t)j * 3;
  atomicAdd(s + 0, (unsigned long long)sc);
  atomicAdd(s + 1, (unsigned long long)(sc * sc));
  atomicAdd(s + 2, 1ull);
}

}  // namespace

extern "C" {

int hsad_search_fork_state(const int32_t* src_index, int G_dst, int G_src, int P, int L, int H, const float* h_src, const float* c_src,
                           float* h_dst, float* c_dst, void* h16_dst, void* stream) {
  if (!src_index || !h_src || !c_src || !h_dst || !c_dst) return efail(HSAD_ERR_INVALID, "hsad_search_fork_state: null argument");
  if (G_dst < 1 || G_src < 1 || P < 1 || L < 1 || H < 1)
    return efail(HSAD_ERR_INVALID, "hsad_search_fork_state: G_dst, G_src, P, L and H must be >= 1");
  if (H % 4) return efail(HSAD_ERR_INVALID, "hsad_search_fork_state: H = %d is no multiple of 4 (rows move as 16-byte vectors)", H);
  const int V = (H % 8 == 0) ? 8 : 4;
  if ((((uintptr_t)h_src | (uintptr_t)c_src | (uintptr_t)h_dst | (uintptr_t)c_dst) & 15u) || ((uintptr_t)h16_dst & (size_t)(2 * V - 1)))
    return efail(HSAD_ERR_INVALID, "hsad_search_fork_state: the state tensors must be 16-byte aligned");
  const long long total = (long long)L * G_dst * P * (H / V);
  const long long blocks = (total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL) return efail(HSAD_ERR_INVALID, "hsad_search_fork_state: %lld values are too many for one launch", total * V);
  hipStream_t st = (hipStream_t)stream;
  unsigned short* h16 = static_cast<unsigned short*>(h16_dst);
  if (V == 8)
    hipLaunchKernelGGL(fork_state_kernel<8>, dim3((unsigned)blocks), dim3(kThreads), 0, st, src_index, G_dst, G_src, P, H, total, h_src,
                       c_src, h_dst, c_dst, h16);
  else
    hipLaunchKernelGGL(fork_state_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, st, src_index, G_dst, G_src, P, H, total, h_src,
                       c_src, h_dst, c_dst, h16);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_search_actions(const hsad_env* env, const int64_t* a_src, const int64_t* greedy_src, const int32_t* player,
                        const int64_t* override_a, int64_t* a, int64_t* greedy_a, void* stream) {
  if (!a_src || !greedy_src || !a || !greedy_a) return efail(HSAD_ERR_INVALID, "hsad_search_actions: null argument");
  if (override_a && !player) return efail(HSAD_ERR_INVALID, "hsad_search_actions: an override needs the player it is for");
  const uint32_t* misc;
  int G, P, A, perfect;
  CK(hsad_internal_env_status(env, &misc, &G, &P, &A, &perfect));
  const int n = G * P;
  hipLaunchKernelGGL(search_actions_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, misc, n, P, A - 1,
                     a_src, greedy_src, player, override_a, a, greedy_a);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_search_job_stats(const hsad_env* env, const int32_t* job, int n_job, int64_t* stats, void* stream) {
  if (!job || !stats) return efail(HSAD_ERR_INVALID, "hsad_search_job_stats: null argument");
  if (n_job < 1) return efail(HSAD_ERR_INVALID, "hsad_search_job_stats: n_job must be >= 1");
  const uint32_t* misc;
  int G, P, A, perfect;
  CK(hsad_internal_env_status(env, &misc, &G, &P, &A, &perfect));
  hipLaunchKernelGGL(job_stats_kernel, dim3((G + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, misc, G, job, n_job,
                     reinterpret_cast<unsigned long long*>(stats));
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

}  // extern "C"
