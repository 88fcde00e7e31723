// hsad_search.hip — the glue kernels of blueprint-policy search (include/hsad.h: hsad_search_fork_state / hsad_search_actions /
// hsad_search_job_stats / hsad_search_horizon_stats / hsad_search_world_scores / hsad_search_round; search.PolicySearch drives them).
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
//   horizon_stats  the same for a depth-limited search: live slots are valued as score so far + the blueprint's Q in 1/256 points
//               (the row function is hsad_search_horizon.h), still integer atomics only
//   belief_rows the searcher's rows of the top layer's h after the root act -> the bf16 operand of the learned belief's head
//               (hsad_search_belief_rows; belief.BeliefSampler, sampler = "learned")
// and, for the replay stage that rebuilds every sampled world's LSTM states from the game's history (PolicySearch(replay=True)):
//   world_script    the root's deal order with the viewer's current cards replaced by the world's sampled hand: what
//                   hsad_env_rewind_scripted takes, so that the world can be played again from its first move
//   replay_actions  the root's logged moves as the a / greedy_a rows of the replay step, and the count of partner moves at which the
//                   blueprint in this world would have shown another greedy action than the one observed
// and, for the search in rounds (PolicySearch.search(rounds = ...)), which compares actions world by world and drops hopeless ones:
//   world_scores    the finished slots' scores, one byte per (pair, world)
//   round           per searched game: raw sums, the leader, paired sums against the leader's and the blueprint's row, pruning --
//                   one workgroup per game, integer arithmetic only, no atomics
// All are launch-only, one pass and HBM-bound.  The state rows move as 16-byte vectors (H % 4 == 0; with H % 8 == 0 the bf16
// row is written as 16-byte vectors too).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "hsad.h"
#include "hsad_rulebot.h"
#include "hsad_search_horizon.h"

extern "C" int hsad_internal_set_error(int code, const char* msg);
extern "C" int hsad_internal_env_status(const hsad_env* e, const uint32_t** misc, int* G, int* P, int* A, int* perfect_score);
extern "C" int hsad_internal_env_hands(const hsad_env* e, const uint32_t** hand0, int* G, int* Gpad, int* P, int* H);
extern "C" int hsad_internal_env_legal_bits(const hsad_env* e, const unsigned long long** legal_bits);
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

// one thread per slot, laid out as job_stats_kernel: the slot's value at the horizon (sh_slot, hsad_search_horizon.h) from its two
// status words and its P rows of Q; up to five 64-bit integer atomics and one 16-bit store per counted slot with a valid job
__global__ __launch_bounds__(kThreads) void horizon_stats_kernel(const uint32_t* __restrict__ planes, int G, int Gpad, int P, int perfect,
                                                                 const int32_t* __restrict__ job, int n_job, const float* __restrict__ q_rows,
                                                                 int mode, unsigned long long* __restrict__ stats,
                                                                 unsigned long long* __restrict__ cut, unsigned long long* __restrict__ nonfinite,
                                                                 const int32_t* __restrict__ world, int worlds,
                                                                 uint16_t* __restrict__ world_values) {
  const int g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= G) return;
  const int j = job[g];
  if (j < 0 || j >= n_job) return;
  const uint32_t misc = planes[(size_t)PL_MISC * Gpad + g], board = planes[(size_t)PL_BOARD * Gpad + g];
  const float* row = q_rows + (size_t)g * P;
  const ShValue r = sh_slot(misc, board, P, perfect, mode, [row](int p) { return row[p]; });
  if (!r.counted) return;
  const long long v = r.v;
  unsigned long long* s = stats + (size_t)j * 3;
  atomicAdd(s + 0, (unsigned long long)v);
  atomicAdd(s + 1, (unsigned long long)(v * v));
  atomicAdd(s + 2, 1ull);
  if (r.cut) atomicAdd(cut + j, 1ull);
  if (r.nonfinite) atomicAdd(nonfinite, 1ull);
  if (world_values) {
    const int w = world[g];
    if (w >= 0 && w < worlds) world_values[(size_t)j * worlds + w] = (uint16_t)r.v;
  }
}

// one thread per world slot.  The env's move uids (HanabiGame::GetMove order): discard slot i = i, play slot i = H + i, hints above.
// hand0: the world env's hand planes, word of seat p and game j at hand0[p * Gpad + j] = cards 5 x 5 bits | length [25..27]
__global__ __launch_bounds__(kThreads) void world_script_kernel(const uint32_t* __restrict__ hand0, int G_w, int Gpad_w, int P, int H,
                                                                const int32_t* __restrict__ src_index, const int32_t* __restrict__ viewer,
                                                                const uint8_t* __restrict__ root_dh, const int32_t* __restrict__ root_count,
                                                                int G_root, const int64_t* __restrict__ log_a, int n_moves,
                                                                uint8_t* __restrict__ script_out, int32_t* __restrict__ count_out) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= G_w) return;
  uint8_t* out = script_out + (size_t)j * 52;
  const int s = src_index[j], v = viewer[j];
  int n = 0;
  int slot[5] = {0, 0, 0, 0, 0}, len = 0;
  bool ok = s >= 0 && s < G_root && v >= 0 && v < P;
  if (ok) {
    n = root_count[s];
    ok = n >= P * H && n <= 50;
  }
  if (ok) {
    len = H;
    for (int i = 0; i < H; ++i) slot[i] = v * H + i;
    int d = P * H;   // the running deal index
    for (int t = 0; t < n_moves; ++t) {
      const int m = t % P;
      const int64_t uid = log_a[((size_t)t * G_root + s) * P + m];
      if (uid < 0 || uid >= 2 * H) continue;   // a hint or the noop: no card moves
      const int idx = (int)(uid < H ? uid : uid - H);
      if (m == v) {
        if (idx >= len) {
          ok = false;
          break;
        }
        for (int i = idx; i + 1 < len; ++i) slot[i] = slot[i + 1];
        len -= 1;
      }
      if (d < n) {
        if (m == v) slot[len++] = d;   // len < H here: a slot was just freed
        d += 1;
      }
    }
    // the log must lead to the hand the world holds
    const uint32_t hw = hand0[(size_t)v * Gpad_w + j];
    ok = ok && (int)((hw >> 25) & 7u) == len;
    if (ok) {
      const uint8_t* dh = root_dh + (size_t)s * 52;
      for (int i = 0; i < 52; ++i) out[i] = i < n ? dh[i] : (uint8_t)0;
      for (int k = 0; k < len; ++k) out[slot[k]] = (uint8_t)((hw >> (5 * k)) & 31u);   // slot[k] < d <= n <= 50
    }
  }
  if (!ok) {
    for (int i = 0; i < 52; ++i) out[i] = 0;
    n = 0;
  }
  count_out[j] = n;
}

// one thread per slot of the replaying env; misc: its status plane (num_step [0..7]: movers rotate from seat 0); legal: its legal-move
// masks [G, P], bit uid.  The logged MOVE is legal in every world the sampler can give (a hint that was made touched cards, and the
// knowledge the sampler obeys says so); the logged GREEDY action is hypothetical and need not be -- a hint that touches no card of the
// hand this world gave the viewer.  The step would refuse it (sad = 1), so the mover then shows its move instead; the world is
// counted as a mismatch anyway, since act never returns an illegal greedy action.
__global__ __launch_bounds__(kThreads) void replay_actions_kernel(const uint32_t* __restrict__ misc,
                                                                  const unsigned long long* __restrict__ legal, int G, int P, int noop,
                                                                  const int32_t* __restrict__ src_index, const int32_t* __restrict__ viewer,
                                                                  const int64_t* __restrict__ log_a_t, const int64_t* __restrict__ log_g_t,
                                                                  int G_root, const int64_t* __restrict__ greedy_src, int64_t* __restrict__ a,
                                                                  int64_t* __restrict__ ga, int32_t* __restrict__ mismatch) {
  const int g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= G) return;
  const int s = src_index[g];
  const uint32_t m = misc[g];
  if (s < 0 || s >= G_root || !game_live(m)) {
    for (int p = 0; p < P; ++p) a[(size_t)g * P + p] = ga[(size_t)g * P + p] = (int64_t)noop;
    return;
  }
  const int mover = (int)(m & 255u) % P;
  const int64_t shown = log_g_t[(size_t)s * P + mover];
  const bool differs = mover != viewer[g] && greedy_src[(size_t)g * P + mover] != shown;   // read before a / ga (may alias) are written
  const bool possible = shown >= 0 && shown < 64 && ((legal[(size_t)g * P + mover] >> shown) & 1ull);
  for (int p = 0; p < P; ++p) {
    const int64_t act = log_a_t[(size_t)s * P + p];
    a[(size_t)g * P + p] = act;
    ga[(size_t)g * P + p] = (p == mover && !possible) ? act : log_g_t[(size_t)s * P + p];
  }
  if (differs) mismatch[g] += 1;
}

// one thread per slot; one byte store per finished slot with a valid (pair, world): a (pair, world) is played at most once, so no
// two slots of a launch name the same byte
__global__ __launch_bounds__(kThreads) void world_scores_kernel(const uint32_t* __restrict__ misc, int G, const int32_t* __restrict__ pair,
                                                                const int32_t* __restrict__ world, int n_pair, int worlds,
                                                                uint8_t* __restrict__ scores) {
  const int g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= G) return;
  const int p = pair[g], w = world[g];
  if (p < 0 || p >= n_pair || w < 0 || w >= worlds) return;
  const uint32_t m = misc[g];
  if (!game_finished(m)) return;
  scores[(size_t)p * worlds + w] = (uint8_t)(((m >> 16) & 63u) - 1u);   // the score job_stats_kernel sums, 0..25
}

constexpr int kRoundWorlds = 4096;     // the longest row hsad_search_round takes: with it every product below stays under 2^56
constexpr int kRoundLdsPairs = 32;     // raw sums of a game's first pairs are kept in LDS; later pairs are read back from raw_out
constexpr uint8_t kAbsent = 0xFF;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// is the raw mean (s_a / n_a) of pair a ahead of that of pair b?  n = 0 is behind everything; ties go to the lower pair index
__device__ __forceinline__ bool leads(int s_a, int n_a, int i_a, int s_b, int n_b, int i_b) {
  if (n_a == 0 || n_b == 0) return n_a != 0 || (n_b == 0 && i_a < i_b);
  const long long l = (long long)s_a * n_b, r = (long long)s_b * n_a;
  return l > r || (l == r && i_a < i_b);
}

// one workgroup of four waves per searched game; waves take the game's pairs round-robin, the lanes of a wave stride over the worlds
// of a row (byte loads from consecutive addresses).  Per-lane and per-wave sums fit int32: |d| <= 25, d^2 <= 625, worlds <= 4096.
__global__ __launch_bounds__(kThreads) void search_round_kernel(const uint8_t* __restrict__ scores, int n_pair, int worlds,
                                                                const int32_t* __restrict__ first_pair, const int32_t* __restrict__ bp_pair,
                                                                long long z2_num, long long z2_den, int min_n, uint8_t* __restrict__ alive,
                                                                int32_t* __restrict__ leader_out, long long* __restrict__ raw_out,
                                                                long long* __restrict__ paired_ref_out,
                                                                long long* __restrict__ paired_bp_out) {
  __shared__ int raw_s[kRoundLdsPairs], raw_n[kRoundLdsPairs];
  __shared__ uint8_t ref_row[kRoundWorlds], bp_row[kRoundWorlds];
  __shared__ int leader_sh;
  const int k = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p0 = first_pair[k], p1 = first_pair[k + 1];
  if (p0 < 0 || p1 > n_pair || p0 >= p1) {      // no pairs, or a list that leaves the tables: nothing of this game is read or written
    if (threadIdx.x == 0) leader_out[k] = -1;
    return;
  }
  int bp = bp_pair[k];
  if (bp < p0 || bp >= p1) bp = -1;             // no blueprint pair: its table stays (0, 0, 0), and nothing is exempt on its account
  // phase 1: raw sums
  for (int p = p0 + wave; p < p1; p += 4) {
    const uint8_t* row = scores + (size_t)p * worlds;
    int s = 0, n = 0;
    for (int w = lane; w < worlds; w += 64) {
      const uint8_t v = row[w];
      if (v != kAbsent) {
        s += v;
        n += 1;
      }
    }
    s = wave_sum(s);
    n = wave_sum(n);
    if (lane == 0) {
      raw_out[(size_t)p * 2 + 0] = s;
      raw_out[(size_t)p * 2 + 1] = n;
      if (p - p0 < kRoundLdsPairs) {
        raw_s[p - p0] = s;
        raw_n[p - p0] = n;
      }
    }
  }
  __syncthreads();      // the raw sums of every pair, in LDS and (workgroup scope) in raw_out
  // the leader: wave 0, every lane the best of its pairs, then a butterfly over (sum, n, index)
  if (wave == 0) {
    int bs = 0, bn = 0, bi = 0x7fffffff;
    for (int p = p0 + lane; p < p1; p += 64) {
      if (alive[p] == 0) continue;
      const int i = p - p0;
      const int s = i < kRoundLdsPairs ? raw_s[i] : (int)raw_out[(size_t)p * 2 + 0];
      const int n = i < kRoundLdsPairs ? raw_n[i] : (int)raw_out[(size_t)p * 2 + 1];
      if (n > 0 && leads(s, n, p, bs, bn, bi)) bs = s, bn = n, bi = p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int os = __shfl_xor(bs, o, 64), on = __shfl_xor(bn, o, 64), oi = __shfl_xor(bi, o, 64);
      if (leads(os, on, oi, bs, bn, bi)) bs = os, bn = on, bi = oi;
    }
    if (lane == 0) {
      leader_sh = bn > 0 ? bi : bp;
      leader_out[k] = leader_sh;
    }
  }
  __syncthreads();
  const int leader = leader_sh;
  // the two reference rows into LDS: every pair of the game is compared with them
  for (int w = threadIdx.x; w < worlds; w += kThreads) {
    ref_row[w] = leader >= 0 ? scores[(size_t)leader * worlds + w] : kAbsent;
    bp_row[w] = bp >= 0 ? scores[(size_t)bp * worlds + w] : kAbsent;
  }
  __syncthreads();
  // phase 2: paired sums against both rows, and the pruning rule on the leader's
  for (int p = p0 + wave; p < p1; p += 4) {
    const uint8_t* row = scores + (size_t)p * worlds;
    int D = 0, Q = 0, n = 0, Db = 0, Qb = 0, nb = 0;
    for (int w = lane; w < worlds; w += 64) {
      const uint8_t v = row[w], r = ref_row[w], b = bp_row[w];
      if (v != kAbsent && r != kAbsent) {
        const int d = (int)v - (int)r;
        D += d;
        Q += d * d;
        n += 1;
      }
      if (v != kAbsent && b != kAbsent) {
        const int d = (int)v - (int)b;
        Db += d;
        Qb += d * d;
        nb += 1;
      }
    }
    D = wave_sum(D), Q = wave_sum(Q), n = wave_sum(n);
    Db = wave_sum(Db), Qb = wave_sum(Qb), nb = wave_sum(nb);
    if (lane == 0) {
      long long* o = paired_ref_out + (size_t)p * 3;
      o[0] = D, o[1] = Q, o[2] = n;
      o = paired_bp_out + (size_t)p * 3;
      o[0] = Db, o[1] = Qb, o[2] = nb;
      if (alive[p] != 0 && p != leader && p != bp && n >= min_n && D < 0) {
        // mean + z * sem < 0 with mean = D / n, sem^2 = (n Q - D^2) / n^3 and D < 0  <=>  D^2 n > z^2 (n Q - D^2)
        const long long D2 = (long long)D * D;
        if (D2 * n * z2_den > z2_num * ((long long)n * Q - D2)) alive[p] = 0;
      }
    }
  }
}

// one thread per 8 consecutive values of one output row (H % 8 == 0): two 16-byte loads of the searcher's fp32 row, one 16-byte
// store of its bf16 image; a game whose player is out of range gets a zero row.  Columns H .. ldo - 1 are not written.
__global__ __launch_bounds__(kThreads) void belief_rows_kernel(const float* __restrict__ h_top, const int32_t* __restrict__ player, int G, int P,
                                                               int H, unsigned short* __restrict__ out, int ldo) {
  const int per_row = H / 8;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (long long)G * per_row) return;
  const int g = (int)(i / per_row);
  const int v = (int)(i - (long long)g * per_row);
  const int p = player[g];
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (p >= 0 && p < P) {
    const float* src = h_top + ((size_t)g * P + p) * H + (size_t)v * 8;
    const float4 a = *reinterpret_cast<const float4*>(src);
    const float4 b = *reinterpret_cast<const float4*>(src + 4);
    w = make_uint4(f2bf_bits(a.x) | (f2bf_bits(a.y) << 16), f2bf_bits(a.z) | (f2bf_bits(a.w) << 16), f2bf_bits(b.x) | (f2bf_bits(b.y) << 16),
                   f2bf_bits(b.z) | (f2bf_bits(b.w) << 16));
  }
  *reinterpret_cast<uint4*>(out + (size_t)g * ldo + (size_t)v * 8) = w;
}

}  // namespace

extern "C" {

int hsad_search_belief_rows(const float* h_top, const int32_t* player, int G, int P, int H, void* out_bf16, int ldo, void* stream) {
  if (!h_top || !player || !out_bf16) return efail(HSAD_ERR_INVALID, "hsad_search_belief_rows: null argument");
  if (G < 1 || P < 1 || H < 8 || H % 8) return efail(HSAD_ERR_INVALID, "hsad_search_belief_rows: G and P must be >= 1, H a positive multiple of 8");
  if (ldo < H || ldo % 8) return efail(HSAD_ERR_INVALID, "hsad_search_belief_rows: ldo = %d must be a multiple of 8 and at least H = %d", ldo, H);
  if (((uintptr_t)h_top | (uintptr_t)out_bf16) & 15u) return efail(HSAD_ERR_INVALID, "hsad_search_belief_rows: the tensors must be 16-byte aligned");
  const long long total = (long long)G * (H / 8);
  const long long blocks = (total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL) return efail(HSAD_ERR_INVALID, "hsad_search_belief_rows: %lld values are too many for one launch", total * 8);
  hipLaunchKernelGGL(belief_rows_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, h_top, player, G, P, H,
                     static_cast<unsigned short*>(out_bf16), ldo);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

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

int hsad_search_horizon_stats(const hsad_env* env, const int32_t* job, int n_job, const float* q_rows, int mode, int64_t* stats,
                              int64_t* cut, int64_t* nonfinite, const int32_t* world, int worlds, uint16_t* world_values, void* stream) {
  if (!job || !q_rows || !stats || !cut || !nonfinite) return efail(HSAD_ERR_INVALID, "hsad_search_horizon_stats: null argument");
  if (n_job < 1) return efail(HSAD_ERR_INVALID, "hsad_search_horizon_stats: n_job must be >= 1");
  if (mode != HSAD_SEARCH_HORIZON_MOVER && mode != HSAD_SEARCH_HORIZON_TEAM)
    return efail(HSAD_ERR_INVALID, "hsad_search_horizon_stats: mode = %d is neither HSAD_SEARCH_HORIZON_MOVER nor _TEAM", mode);
  if (world_values && !world) return efail(HSAD_ERR_INVALID, "hsad_search_horizon_stats: world_values needs the world of every slot");
  if (world_values && worlds < 1) return efail(HSAD_ERR_INVALID, "hsad_search_horizon_stats: worlds must be >= 1 with world_values");
  const uint32_t* planes;
  uint32_t* act_count;
  int G, Gpad;
  RbRules ru;
  CK(hsad_internal_env_rulebot_view(env, &planes, &act_count, &G, &Gpad, &ru));
  hipLaunchKernelGGL(horizon_stats_kernel, dim3((G + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, planes, G, Gpad, ru.P,
                     ru.nC * ru.nR, job, n_job, q_rows, mode, reinterpret_cast<unsigned long long*>(stats),
                     reinterpret_cast<unsigned long long*>(cut), reinterpret_cast<unsigned long long*>(nonfinite), world, worlds,
                     world_values);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_search_world_script(const hsad_env* world_env, const int32_t* src_index, const int32_t* viewer, const uint8_t* root_deck_hist,
                             const int32_t* root_count, int G_root, const int64_t* log_a, int n_moves, uint8_t* script_out,
                             int32_t* count_out, void* stream) {
  if (!src_index || !viewer || !root_deck_hist || !root_count || !script_out || !count_out)
    return efail(HSAD_ERR_INVALID, "hsad_search_world_script: null argument");
  if (G_root < 1 || n_moves < 0) return efail(HSAD_ERR_INVALID, "hsad_search_world_script: G_root must be >= 1 and n_moves >= 0");
  if (n_moves > 0 && !log_a) return efail(HSAD_ERR_INVALID, "hsad_search_world_script: n_moves > 0 needs the move log");
  const uint32_t* hand0;
  int G, Gpad, P, H;
  CK(hsad_internal_env_hands(world_env, &hand0, &G, &Gpad, &P, &H));
  hipLaunchKernelGGL(world_script_kernel, dim3((G + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, hand0, G, Gpad, P, H,
                     src_index, viewer, root_deck_hist, root_count, G_root, log_a, n_moves, script_out, count_out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_search_replay_actions(const hsad_env* env, const int32_t* src_index, const int32_t* viewer, const int64_t* log_a_t,
                               const int64_t* log_greedy_t, int G_root, const int64_t* greedy_src, int64_t* a, int64_t* greedy_a,
                               int32_t* mismatch, void* stream) {
  if (!src_index || !viewer || !log_a_t || !log_greedy_t || !greedy_src || !a || !greedy_a || !mismatch)
    return efail(HSAD_ERR_INVALID, "hsad_search_replay_actions: null argument");
  if (G_root < 1) return efail(HSAD_ERR_INVALID, "hsad_search_replay_actions: G_root must be >= 1");
  const uint32_t* misc;
  int G, P, A, perfect;
  CK(hsad_internal_env_status(env, &misc, &G, &P, &A, &perfect));
  const unsigned long long* legal;
  CK(hsad_internal_env_legal_bits(env, &legal));
  hipLaunchKernelGGL(replay_actions_kernel, dim3((G + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, misc, legal, G, P, A - 1,
                     src_index, viewer, log_a_t, log_greedy_t, G_root, greedy_src, a, greedy_a, mismatch);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_search_world_scores(const hsad_env* env, const int32_t* pair, const int32_t* world, int n_pair, int worlds, uint8_t* scores,
                             void* stream) {
  if (!pair || !world || !scores) return efail(HSAD_ERR_INVALID, "hsad_search_world_scores: null argument");
  if (n_pair < 1 || worlds < 1) return efail(HSAD_ERR_INVALID, "hsad_search_world_scores: n_pair and worlds must be >= 1");
  const uint32_t* misc;
  int G, P, A, perfect;
  CK(hsad_internal_env_status(env, &misc, &G, &P, &A, &perfect));
  hipLaunchKernelGGL(world_scores_kernel, dim3((G + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, misc, G, pair, world,
                     n_pair, worlds, scores);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_search_round(const uint8_t* scores, int n_pair, int worlds, const int32_t* first_pair, int n_game, const int32_t* bp_pair,
                      int z2_num, int z2_den, int min_n, uint8_t* alive, int32_t* leader_out, int64_t* raw_out, int64_t* paired_ref_out,
                      int64_t* paired_bp_out, void* stream) {
  if (!scores || !first_pair || !bp_pair || !alive || !leader_out || !raw_out || !paired_ref_out || !paired_bp_out)
    return efail(HSAD_ERR_INVALID, "hsad_search_round: null argument");
  if (n_pair < 1 || n_game < 1) return efail(HSAD_ERR_INVALID, "hsad_search_round: n_pair and n_game must be >= 1");
  if (worlds < 1 || worlds > kRoundWorlds)
    return efail(HSAD_ERR_INVALID, "hsad_search_round: worlds = %d is outside [1, %d]", worlds, kRoundWorlds);
  if (z2_den < 1 || z2_den > 1024 || z2_num < 0 || z2_num > 16384)
    return efail(HSAD_ERR_INVALID, "hsad_search_round: z^2 = %d / %d is outside [0, 16384] / [1, 1024] (the int64 bounds)", z2_num, z2_den);
  if (min_n < 1) return efail(HSAD_ERR_INVALID, "hsad_search_round: min_n must be >= 1");
  hipLaunchKernelGGL(search_round_kernel, dim3(n_game), dim3(kThreads), 0, (hipStream_t)stream, scores, n_pair, worlds, first_pair, bp_pair,
                     (long long)z2_num, (long long)z2_den, min_n, alive, leader_out, reinterpret_cast<long long*>(raw_out),
                     reinterpret_cast<long long*>(paired_ref_out), reinterpret_cast<long long*>(paired_bp_out));
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

}  // extern "C"
